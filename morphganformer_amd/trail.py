"""What mgf_select_best reports about improvements: the flag slot both projection engines hand it, and the literal loop's improvement
trail -- the scored image of every improvement, the drivers' `{step:06d}_{loss:04f}.png` files (...sqz_MSE.py:186-195) -- built on it."""
from __future__ import annotations

import warnings

import torch


class ImprovementSlot:
    """The improvement-flag arguments of mgf_select_best for `candidates` candidates per launch and `slots` trail slots: take[j] = the slot
    candidate j's improvement went to, or -1; count = improvements so far; steps / losses = step and loss of the improvement in each slot
    (past `slots` improvements the last slot is overwritten).  One candidate and one slot make a plain flag: take[0] = 0 where this step
    improved (GradientProjectionEngine(optimize_noise=True) keeps the noise maps of such a step)."""

    def __init__(self, candidates, slots, device):
        self.slots = int(slots)
        self.steps = torch.full([self.slots], -1, dtype=torch.int32, device=device)
        self.losses = torch.zeros(self.slots, dtype=torch.float64, device=device)
        self.count = torch.zeros(1, dtype=torch.int32, device=device)
        self.take = torch.full([candidates], -1, dtype=torch.int32, device=device)

    def state(self, with_take=False):
        """(tensor, reset value) rows for the engine's state table.  `take` is rewritten by every launch: state only for an engine that reads
        it outside the launch that wrote it."""
        return [(self.count, 0), (self.steps, -1), (self.losses, 0)] + ([(self.take, -1)] if with_take else [])


class ImprovementTrail(ImprovementSlot):
    """A trail of up to `keep` scored images ([C, R, R] each) for an engine that launches `batch` candidates per sequence, filled inside the
    launch sequence (select_best names the slot, mgf_keep_improvements copies the image) and spilled to host memory between sequences
    whenever the NEXT one could overflow the slots -- a sequence improves at most `batch` times -- so with keep >= batch every improvement of
    a run of any length keeps its image, for keep x 12.6 MB of device memory at 1024^2 instead of one slot per step."""

    def __init__(self, keep, batch, image_shape, device):
        super().__init__(batch, keep, device)
        self.batch, self.device = int(batch), device
        c, r = image_shape
        self.image_shape = (c, r, r)
        self.imgs = torch.empty(self.slots, c * r * r, dtype=torch.float32, device=device)
        if self.slots < self.batch:
            warnings.warn(f"ProjectionEngine: keep_images={self.slots} < batch={self.batch}: one launch sequence can improve more often than "
                          "there are trail slots, and then only the latest improvement of the overflow keeps its image (the reference "
                          "writes a PNG at every improvement); use keep_images >= batch", stacklevel=3)
        self.forget()

    def forget(self):
        """The host side back to an empty trail (the engine's rewind() resets the device side through its state table)."""
        self.spilled, self.since_spill, self.lost = [], 0, 0

    def before_sequence(self):
        """In front of every launch sequence: spill if this one could overflow the slots."""
        if self.since_spill > 0 and (self.since_spill + 1) * self.batch > self.slots:
            self.spill()
        self.since_spill += 1

    def spill(self):
        """Move the filled slots to host memory and empty the device trail (between launch sequences; one host sync)."""
        torch.cuda.synchronize(self.device)
        total = int(self.count.item())
        n = min(total, self.slots)
        self.lost += total - n
        if n:
            steps, losses = self.steps[:n].cpu().numpy(), self.losses[:n].cpu().numpy()
            imgs = self.imgs[:n].cpu()
            self.spilled += [(int(steps[i]), float(losses[i]), imgs[i].view(self.image_shape)) for i in range(n)]
        self.count.zero_()
        self.steps.fill_(-1)
        self.since_spill = 0

    def listing(self):
        """[(step, loss, image [C,R,R])] in the order the improvements happened: the spilled ones (CPU tensors), then those still on the device."""
        torch.cuda.synchronize(self.device)
        total = int(self.count.item())
        n = min(total, self.slots)
        lost = self.lost + total - n
        if lost:
            warnings.warn(f"ProjectionEngine: {lost} improvement image(s) were overwritten: keep_images={self.slots} < batch={self.batch} "
                          "(the reference writes one PNG per improvement)", stacklevel=3)
        steps, losses = self.steps.cpu().numpy(), self.losses.cpu().numpy()
        return list(self.spilled) + [(int(steps[i]), float(losses[i]), self.imgs[i].view(self.image_shape)) for i in range(n)]
