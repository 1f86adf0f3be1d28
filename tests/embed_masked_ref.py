"""The masked float64 restatement of the IResNet and FaceNet embedders (tests/test_hip_embed_blocks.py, tests/test_embed_blocks_host.py).

A float32 implementation and float64 disagree on the branch of a PReLU / ReLU unit whose pre-activation lies within float32 rounding of zero, and
the whole gradient behind that unit moves: the max-norm error of a CORRECT float32 gradient against free float64 autograd is 1e-2.  Here the
float64 network is evaluated as the piecewise-linear map the implementation itself selected: every non-linearity is replaced by its linear branch,
chosen from outside (`Masked`), through the hook of oracle/embed_ref.py -- the topology is stated there, once.  Under the implementation's own
masks a correct float32 gradient is within 1e-5 of float64 at every block boundary, and `gate_rows` holds it to that:

    max|got_b - ref64_b| / max|ref64_b|  <=  max(8 r_b, 1e-5),     r_b = the same quantity for this restatement in float32 on the CPU

(8 and 1e-5: test_hip_mobilefacenet.py::test_backward_matches_the_float64_gradient).  The reference gradient is plain autograd; the only things
written by hand are the three linear branches below and the gradient hooks of `FAULTS`, which exist to show that the gate rejects them.
"""
import numpy as np
import torch
import torch.nn.functional as F

from morphganformer_amd.facenet import STEM
from morphganformer_amd.iresnet import block_table
from oracle.embed_ref import inception_resnet_v1_ref, iresnet_ref

GATE_FACTOR, GATE_FLOOR = 8.0, 1e-5
FLIP_PRE, FLIP_SHARE = 1e-4, 1e-5            # a disagreeing unit: |pre-activation| <= 1e-4 max|pre-activation| of its layer; <= 1e-5 of all units


def first_max_indices(x):
    """The window index a 3x3 / stride-2 / floor-mode max-pool routes its gradient to under the FIRST-MAXIMUM rule of include/mgf.h
    (mgf_maxpool_s2_floor_bwd_f32): of the window elements equal to the window's maximum, the first in row-major window order (top row left to
    right, then the next row).  Stated here with unfold and an explicit minimum over the positions of the maxima -- no library's tie-breaking is
    relied on (windows of post-ReLU maps tie at exact zeros).  x [n,c,h,w] -> int64 [n,c,oh,ow] of flat indices y * w + x into the h*w plane."""
    n, c, h, w = x.shape
    oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    u = F.unfold(x.detach().reshape(n * c, 1, h, w), 3, stride=2)                       # [nc, 9, oh*ow], window positions in row-major order
    is_max = u == u.max(dim=1, keepdim=True).values
    pos = torch.arange(9).reshape(1, 9, 1)
    k = torch.where(is_max, pos, torch.full_like(pos, 9)).min(dim=1).values               # first position holding the maximum
    assert int(k.max()) < 9
    k = k.reshape(n, c, oh, ow)
    oy, ox = torch.arange(oh).reshape(1, 1, oh, 1), torch.arange(ow).reshape(1, 1, 1, ow)
    return (2 * oy + k // 3) * w + (2 * ox + k % 3)


class Recorder:
    """The free network (F.prelu, F.relu, the first-maximum pool) that records what it decided: masks[name] = output > 0 (what the HIP backward
    reads off its kept outputs; a value of exactly 0 is `False`: the slope branch, the zero branch), pre[name] = the pre-activation, pool_idx /
    pool_x[name] = the indices the pool chose and its input; taps[name] = the marked tensors (gradients retained when they carry any)."""

    def __init__(self, keep_pre=True):
        self.masks, self.pre, self.pool_idx, self.pool_x, self.taps, self.keep_pre = {}, {}, {}, {}, {}, keep_pre

    def act(self, name, x, slope):
        y = F.relu(x) if slope is None else F.prelu(x, slope)
        self.masks[name] = y.detach() > 0
        if self.keep_pre:
            self.pre[name] = x.detach()
        return y

    def pool(self, name, x):
        y = F.max_pool2d(x, 3, stride=2)
        self.pool_idx[name], self.pool_x[name] = first_max_indices(x), x.detach()
        return y

    def tap(self, name, x):
        if x.requires_grad:
            x.retain_grad()
        self.taps[name] = x
        return x

    def conv_in(self, name, x):
        return x

    def conv_out(self, name, y):
        return y


# faults of tests/test_embed_blocks_host.py: kind -> where it acts.  Each is a gradient hook (or a detached forward correction), never a forward change.
FAULT_KINDS = ("last_row", "last_col", "ring", "last_channel", "no_mask", "roll_slope")


class Masked:
    """Every non-linearity replaced by the linear branch `masks` / `pool_idx` name:  PReLU: x * where(mask, 1, slope_c);  ReLU: x * mask;
    max-pool: a gather at the given window indices.  faults {layer name: kind}: the backward of that layer is mutated, the forward is not."""

    def __init__(self, masks, pool_idx, faults=None):
        self.masks, self.pool_idx, self.taps, self.faults = masks, pool_idx, {}, dict(faults or {})
        assert all(k in FAULT_KINDS for k in self.faults.values())
        self.hit = set()

    def act(self, name, x, slope):
        m = self.masks[name]
        assert tuple(m.shape) == tuple(x.shape) and m.dtype == torch.bool, (name, tuple(m.shape), tuple(x.shape))
        one = torch.ones((), dtype=x.dtype)
        f = m.to(x.dtype) if slope is None else torch.where(m, one, slope.reshape(1, -1, 1, 1))
        y = x * f
        kind = self.faults.get(name)
        if kind == "no_mask":                               # the ReLU mask omitted in the backward: d(x) = d(y)
            self.hit.add(name)
            return x + (y - x).detach()
        if kind == "roll_slope":                            # the slope vector rolled by one channel in the backward
            self.hit.add(name)
            wrong = x * torch.where(m, one, slope.roll(1).reshape(1, -1, 1, 1))
            return wrong + (y - wrong).detach()
        return y

    def pool(self, name, x):
        idx = self.pool_idx[name]
        n, c = x.shape[:2]
        assert idx.shape[:2] == (n, c)
        return x.reshape(n, c, -1).gather(2, idx.reshape(n, c, -1)).reshape(idx.shape)

    tap = Recorder.tap

    def conv_in(self, name, x):
        kind = self.faults.get(name)
        if kind not in ("last_row", "last_col", "ring"):
            return x
        self.hit.add(name)

        def lose(g):
            g = g.clone()
            if kind in ("last_row", "ring"):
                g[:, :, -1] = 0
            if kind in ("last_col", "ring"):
                g[:, :, :, -1] = 0
            if kind == "ring":
                g[:, :, 0] = 0
                g[:, :, :, 0] = 0
            return g

        x = x.clone()
        x.register_hook(lose)
        return x

    def conv_out(self, name, y):
        if self.faults.get(name) != "last_channel":
            return y
        self.hit.add(name)

        def lose(g):
            g = g.clone()
            g[:, -1] = 0
            return g

        y = y.clone()
        y.register_hook(lose)
        return y


def state(sd_np, dtype):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd_np.items()}


def forward(net, sd, img, hook):
    """net "facenet" (the un-resized image) or "iresnet<depth>" (bilinear resize to 112x112 unless the image has that size).  The image is
    the tap "img"; for the IResNets the 112x112 input is "x112"."""
    x = hook.tap("img", img)
    if net == "facenet":
        return inception_resnet_v1_ref(sd, x, hook=hook)
    if tuple(x.shape[2:]) != (112, 112):
        x = F.interpolate(x, size=(112, 112), mode="bilinear", align_corners=False)
    return iresnet_ref(sd, hook.tap("x112", x), int(net[len("iresnet"):]), hook=hook)


def boundaries(net):
    """The compared tensors, the deepest (closest to the embedding) first, the image last."""
    if net == "facenet":
        names = ["pre", "mean", "in:block8"] + [f"in:repeat_3.{r}" for r in range(4, -1, -1)] + ["in:mixed_7a"]
        names += [f"in:repeat_2.{r}" for r in range(9, -1, -1)] + ["in:mixed_6a"] + [f"in:repeat_1.{r}" for r in range(4, -1, -1)]
        return names + ["in:" + name for name, _ in reversed(STEM[1:])] + ["img"]
    return ["top"] + ["in:" + row[0] for row in reversed(block_table(int(net[len("iresnet"):])))] + ["x112", "img"]


def _seed(emb, demb):
    """The scalar whose gradient is taken: <embedding, demb> for a seed gradient demb [n, 512], or demb(embedding) for a loss."""
    return demb(emb) if callable(demb) else (emb * demb.to(emb.dtype)).sum()


def free_run(net, sd_np, img, dtype, demb=None, keep_pre=True):
    """The free network in `dtype`: -> (embedding, Recorder, {boundary: gradient} or None)."""
    rec = Recorder(keep_pre)
    x = img.detach().to(dtype)
    if demb is None:
        with torch.no_grad():
            return forward(net, state(sd_np, dtype), x, rec).double(), rec, None
    emb = forward(net, state(sd_np, dtype), x.requires_grad_(True), rec)
    _seed(emb, demb).backward()
    return emb.detach().double(), rec, {k: rec.taps[k].grad.double() for k in boundaries(net)}


def masked_gradients(net, sd_np, img, demb, masks, pool_idx, dtype, faults=None):
    """d <embedding, demb> / d(every boundary) of the masked restatement in `dtype` (demb: a seed gradient, or a function embedding -> scalar loss),
    as float64 tensors; -> (embedding, {boundary: gradient})."""
    hook = Masked(masks, pool_idx, faults)
    x = img.detach().to(dtype).requires_grad_(True)
    emb = forward(net, state(sd_np, dtype), x, hook)
    _seed(emb, demb).backward()
    assert hook.hit == set(hook.faults), ("a fault names no layer of this network", set(hook.faults) - hook.hit)
    return emb.detach().double(), {k: hook.taps[k].grad.double() for k in boundaries(net)}


def gate_rows(net, got, ref64, ref32):
    """One row per boundary, the deepest first: r_b (the restatement's own float32 distance), the error of `got`, the bound, the worst element."""
    rows = []
    for name in boundaries(net):
        ref = ref64[name]
        g = got[name].detach().double().cpu()
        assert tuple(g.shape) == tuple(ref.shape), (name, tuple(g.shape), tuple(ref.shape))
        scale = float(ref.abs().max())
        assert scale > 0, name
        d = (g - ref).abs()
        r = float((ref32[name] - ref).abs().max()) / scale
        bound = max(GATE_FACTOR * r, GATE_FLOOR)
        rows.append(dict(name=name, r=r, err=float(d.max()) / scale, bound=bound, worst=tuple(int(i) for i in np.unravel_index(int(d.argmax()), d.shape)),
                         median=float((d / scale).median()), rms=float((d / scale).square().mean().sqrt())))
    return rows


def failing(rows):
    return [r["name"] for r in rows if not r["err"] <= r["bound"]]


def check_gate(rows, label):
    """Print the table; on failure name the deepest failing boundary and its worst element."""
    print(f"--- embedder gradient gate: {label}")
    print(f"{'boundary':>16} {'r_b':>10} {'error':>10} {'bound':>10} {'error/r_b':>10} {'head-room':>10}")
    for r in rows:
        print(f"{r['name']:>16} {r['r']:10.3e} {r['err']:10.3e} {r['bound']:10.3e} {r['err'] / max(r['r'], 1e-300):10.3g} {r['bound'] / max(r['err'], 1e-300):10.3g}")
    big = max(rows, key=lambda r: r["err"] / max(r["r"], 1e-300))
    print(f"    largest error / r_b: {big['err'] / max(big['r'], 1e-300):.3g} at {big['name']}")
    bad = [r for r in rows if not r["err"] <= r["bound"]]
    if bad:
        d = bad[0]                                                                      # rows are ordered from the embedding to the image
        raise AssertionError(f"{label}: {len(bad)} of {len(rows)} boundaries fail; the deepest is {d['name']}: error {d['err']:.3e} > bound "
                             f"{d['bound']:.3e} (r_b {d['r']:.3e}), worst element (n, c, y, x) = {d['worst']}")


def check_masks(imposed_masks, imposed_pool_idx, free):
    """The imposed masks must not hide a wrong forward: against the FREE float64 run (a Recorder), a unit whose imposed branch differs from float64's
    has |pre-activation| <= 1e-4 max|pre-activation| of its layer, a pool window whose imposed element is not a float64 maximiser misses the
    maximum by <= 1e-4 max|input|, and both together are at most 1e-5 of all units.  -> (disagreeing, total)."""
    flips = total = 0
    assert set(imposed_masks) == set(free.masks) and set(imposed_pool_idx) == set(free.pool_idx)
    for name, m64 in free.masks.items():
        m = imposed_masks[name].cpu()
        assert tuple(m.shape) == tuple(m64.shape), name
        diff = m != m64
        total += m.numel()
        k = int(diff.sum())
        if k:
            pre = free.pre[name].abs()
            assert float(pre[diff].max()) <= FLIP_PRE * float(pre.max()), (name, k, float(pre[diff].max()), float(pre.max()))
            flips += k
    for name, x64 in free.pool_x.items():
        idx = imposed_pool_idx[name].cpu()
        n, c = x64.shape[:2]
        assert int(idx.min()) >= 0 and int(idx.max()) < x64.shape[2] * x64.shape[3]
        v = x64.reshape(n, c, -1).gather(2, idx.reshape(n, c, -1)).reshape(idx.shape)
        top = F.max_pool2d(x64, 3, stride=2)
        # the imposed element lies in its own window: first_max_indices of the float64 input differs from it by less than a window
        own = first_max_indices(x64)
        w = x64.shape[3]
        assert int((idx // w - own // w).abs().max()) <= 2 and int((idx % w - own % w).abs().max()) <= 2, name
        miss = v < top
        total += idx.numel()
        k = int(miss.sum())
        if k:
            assert float((top - v)[miss].max()) <= FLIP_PRE * float(x64.abs().max()), (name, k)
            flips += k
    assert flips <= FLIP_SHARE * total, (flips, total)
    return flips, total
