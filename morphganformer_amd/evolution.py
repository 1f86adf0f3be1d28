"""Evolution-strategy mode: the literal loop with a mean that moves.

The literal loop (projection.py) is best-of-N noisy sampling around a `latent_mean` that never changes; gradient mode moves the latent, but only
along terms that have a backward pass.  `EvolutionProjectionEngine` is the (mu/mu_w, lambda) evolution strategy between the two: every batch of
candidates the literal loop evaluates is one GENERATION, and once it is scored the mean moves to a weighted average of its best mu candidates,

    latent_n[j] = mean + eps[s0 + j] * sigma[s0 + j]              j < batch        (mgf_latent_perturb, unchanged)
    totals      = the literal loop's objective of G(latent_n)                      (every term of ProjectionEngine, mgf_select_best, unchanged)
    mean       <- mean + mean_lr * (sum_{r < mu} w_r latent_n[j_r] - mean)         (mgf_es_recombine_f32; j_r: the r-th best valid candidate)

so a term needs no gradient to steer the latent: Wing on a detector's landmarks, the uint8 DSSIM, PSNR, LBP, pool_above.  sigma stays the
drivers' schedule (no step-size adaptation).  All of it is one device-resident launch sequence, replayed as a hipGraph like every engine.

    python -m morphganformer_amd.evolution --model net.pkl --image face.png [--landmarks lm.npz] --lpips-backbone sq.pth --batch 32 --elite 8
                                           (writes <path_to_gen>/<stem>.mat and the improvement trail, like `cli project`)
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np
import torch

from . import _lib
from .projection import ProjectionArgs, ProjectionEngine

ES_MAX_BATCH = 1024         # mgf_es_recombine_f32 ranks a generation in LDS (include/mgf.h)


def recombination_weights(mu, kind="log"):
    """The mu recombination weights, float64, best candidate first, summing to 1.  "log": ln(mu + 1/2) - ln(r) for r = 1..mu, normalised (the
    usual (mu/mu_w, lambda) choice: strictly decreasing, all positive); "equal": 1 / mu each."""
    mu = int(mu)
    if mu < 1:
        raise _lib.MgfError(f"evolution: the number of elite candidates must be >= 1 (got {mu})")
    if kind == "log":
        w = math.log(mu + 0.5) - np.log(np.arange(1, mu + 1, dtype=np.float64))
    elif kind == "equal":
        w = np.ones(mu, dtype=np.float64)
    else:
        raise _lib.MgfError(f"evolution: es_weights must be 'log' or 'equal' (got {kind!r})")
    return w / w.sum()


class EvolutionProjectionEngine(ProjectionEngine):
    """The literal engine with a moving mean.  `batch` is the generation size (lambda), `elite` the number of candidates that are recombined (mu,
    default max(1, batch // 4)), `es_weights` their weights ("log" or "equal", recombination_weights), `mean_lr` in (0, 1] the step towards the
    recombined point.  A generation's invalid candidates ("no face" steps, non-finite totals) never steer the mean; with fewer valid candidates
    than `elite` the valid ones are recombined with the head of the weight table renormalised, with none the mean stays.  Every objective, the
    landmark detectors, the improvement trail, retarget() and the graph replay are the literal engine's own.

    result() is the literal engine's: the best candidate ever SCORED (the mean itself is never rendered).  `mean` is where the search stands,
    `elite_used()` how many candidates each generation recombined.

    Refused: pipeline=True, latent_copies > 1, batch < 2 (and > 1024), elite outside 1..batch, mean_lr outside (0, 1], an unknown es_weights."""

    def __init__(self, G, target, latent_mean, latent_std, args: ProjectionArgs = None, elite=None, es_weights="log", mean_lr=1.0, batch=2,
                 pipeline=False, **kw):
        args = args or ProjectionArgs()
        batch = int(batch)
        if pipeline:
            raise _lib.MgfError("evolution: pipeline=True overlaps one generation's losses with the next generation's generator, whose "
                                "candidates depend on those losses (the mean they are drawn around); the update would be one generation stale")
        if int(args.latent_copies) > 1:
            raise _lib.MgfError(f"evolution: latent_copies > 1 (got {args.latent_copies}) is the v2 driver's averaged copies: the generator sees a "
                                "mean of draws, not a draw, and recombining those is another algorithm")
        if not 2 <= batch <= ES_MAX_BATCH:
            raise _lib.MgfError(f"evolution: batch is the generation size and must lie in 2..{ES_MAX_BATCH} (got {batch}): one candidate per "
                                "generation has nothing to select from")
        elite = max(1, batch // 4) if elite is None else int(elite)
        if not 1 <= elite <= batch:
            raise _lib.MgfError(f"evolution: elite must lie in 1..batch = 1..{batch} (got {elite})")
        mean_lr = float(mean_lr)
        if not 0.0 < mean_lr <= 1.0:
            raise _lib.MgfError(f"evolution: mean_lr must lie in (0, 1] (got {mean_lr}): 0 never moves the mean, above 1 steps past the recombined point")
        self.es_weight_table = recombination_weights(elite, es_weights)       # (raises on an unknown kind, before anything is allocated)
        self.elite, self.es_weights, self.mean_lr = elite, es_weights, mean_lr
        super().__init__(G, target, latent_mean, latent_std, args, batch=batch, pipeline=False, **kw)

    def _init_state(self, nt, latent_mean, latent_std, eps, seed, lm_target, lm_steps, lm_valid):
        super()._init_state(nt, latent_mean, latent_std, eps, seed, lm_target, lm_steps, lm_valid)
        dev = self.device
        self._reg(self.latent_in)                                   # the mean moves: loop state (rewind() puts it back on the start, below)
        self.start_mean = self.latent_in.clone()
        self.weights_dev = torch.as_tensor(self.es_weight_table, dtype=torch.float64, device=dev)
        # the step counter as it stands in front of select_best, which advances it: what the recombination indexes the loss table with
        self.gen_step = self._reg(torch.zeros(1, dtype=torch.int32, device=dev), 0)
        self.used = self._reg(torch.zeros(-(-self.steps // self.batch), dtype=torch.int32, device=dev), 0)

    # ------------------------------------------------------------------ one generation
    def _recombine(self, latent_n):
        _lib.check(_lib.lib().mgf_es_recombine_f32(self.latent_in.data_ptr(), latent_n.data_ptr(), self.losses.data_ptr(), self.gen_step.data_ptr(),
                                                   self.weights_dev.data_ptr(), self.elite, self.batch, self.steps, self.numel, self.mean_lr,
                                                   self.used.data_ptr(), _lib.stream_ptr()), "es_recombine")

    def _gen_phase(self, latent_n, ctr):
        self.gen_step.copy_(ctr)
        return super()._gen_phase(latent_n, ctr)

    def _loss_phase(self, img, latent_n):
        """The literal loss phase, then the recombination as the sequence's last launch (in the two-graph callback form: the end of phase B)."""
        super()._loss_phase(img, latent_n)
        self._recombine(latent_n)

    # ------------------------------------------------------------------ state
    def retarget(self, target, *args, latent_mean=None, **kw):
        """ProjectionEngine.retarget; a new latent_mean replaces the START of the search too (rewind() returns there)."""
        if latent_mean is not None:
            self.start_mean.copy_(latent_mean.detach().reshape(self.start_mean.shape))
        return super().retarget(target, *args, latent_mean=latent_mean, **kw)

    def rewind(self):
        super().rewind()
        self.latent_in.copy_(self.start_mean)
        return self

    @property
    def mean(self):
        """The current mean [1, *latent shape] (a copy, on the device)."""
        return self.latent_in.clone()

    def elite_used(self):
        """[ceil(steps / batch)] int32 numpy: how many candidates each generation recombined (0: the mean stayed, or the generation has not run)."""
        torch.cuda.synchronize(self.device)
        return self.used.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------- module entry
def build_parser():
    from . import cli
    ap = argparse.ArgumentParser(prog="python -m morphganformer_amd.evolution",
                                 description="Project one face image with the evolution-strategy loop: the literal loop's candidates, and a mean "
                                             "that moves to the weighted average of every generation's best")
    ap.add_argument("--model", type=str, default="models/ffhq-snapshot-1024_v2.pkl")
    ap.add_argument("--image", type=str, required=True)
    ap.add_argument("--landmarks", type=str, default=None, help=".npz with `target` [68,2] and `steps` [steps,68,2], like `cli project`")
    ap.add_argument("--path_to_gen", type=str, default="images/projection/", help="output directory: <stem>.mat and the improvement trail's PNG files")
    ap.add_argument("--batch", type=int, default=32, help="candidates per generation (lambda) = loop steps per generator forward")
    ap.add_argument("--elite", type=int, default=None, help="candidates recombined per generation (mu); default max(1, batch // 4)")
    ap.add_argument("--es-weights", choices=["log", "equal"], default="log", help="recombination weights: ln(mu + 1/2) - ln(rank), or uniform")
    ap.add_argument("--mean-lr", type=float, default=1.0, help="step of the mean towards the recombined point, in (0, 1]")
    ap.add_argument("--pixel-term", choices=["mse", "psnr", "dssim", "msssim"], default="mse",
                    help="the pixel term, as the literal loop scores it (dssim: of the uint8 images)")
    ap.add_argument("--noise-mode", choices=["random", "const", "keyed"], default="random",
                    help="the generator's per-layer noise: fresh draws in launch order (random), the checkpoint's constant maps (const), or draws "
                         "keyed by --seed and the step number (keyed: a run replays bit for bit and the best image can be re-rendered)")
    ap.add_argument("--noise_ramp", type=float, default=0.75)
    ap.add_argument("--truncation_psi", type=float, default=0.7)
    ap.add_argument("--min-loss-init", type=float, default=100.0)
    ap.add_argument("--pool-above", type=int, default=0, help="block-average generated images taller than this before the image-space losses")
    ap.add_argument("--keep-images", type=int, default=64, help="device slots of the improvement trail (raised to --batch if smaller)")
    ap.add_argument("--ratio", type=float, default=1.0, help="height / width of the largest centred rectangle an image is cropped to when written")
    cli._objective_arguments(ap)
    cli._lpips_pool_argument(ap)
    ap.add_argument("--gpus", type=str, default="0", help="the visible device(s)")
    return ap


def main(argv=None):
    from . import cli
    a = build_parser().parse_args(argv)
    what = "evolution"
    if a.batch < 2:
        raise SystemExit(f"{what}: --batch is the generation size, at least 2 (got {a.batch})")
    if a.elite is not None and not 1 <= a.elite <= a.batch:
        raise SystemExit(f"{what}: --elite must lie in 1..--batch (got {a.elite}, batch {a.batch})")
    if not 0.0 < a.mean_lr <= 1.0:
        raise SystemExit(f"{what}: --mean-lr must lie in (0, 1] (got {a.mean_lr})")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("CUDA_VISIBLE_DEVICES", a.gpus)
    from . import drivers, loader
    print("Loading networks...")
    G = loader.load_network(a.model, device="cuda")["Gs"]
    args = cli._projection_args(a, noise_ramp=a.noise_ramp, truncation_psi=a.truncation_psi, min_loss_init=a.min_loss_init, pool_above=a.pool_above)
    percept = None if a.no_lpips else cli._lpips_term(a, what, device=G.device)
    biometric = cli._biometric_term(a, what, n=a.batch, device=G.device)
    if percept is None and a.no_mse and biometric is None and not a.landmarks:
        raise SystemExit(f"{what}: every term of the objective is switched off")
    tsize = a.size // args.pool_factor(a.size)
    target = drivers.image_transform(a.image, size=tsize, device=G.device)
    lm_t = lm_s = None
    if a.landmarks:
        lm = np.load(a.landmarks)
        lm_t, lm_s = lm["target"], lm["steps"]
        if lm_s.shape[0] < a.step:
            raise SystemExit(f"--landmarks holds {lm_s.shape[0]} steps, --step is {a.step}")
    stem = os.path.splitext(os.path.basename(a.image))[0]
    res = drivers.project_image(G, target, lm_t, lm_s, args=args, percept=percept, biometric=biometric, gamma=a.gamma, use_mse=not a.no_mse,
                                seed=a.seed, batch=a.batch, mode="evolution", noise_mode=a.noise_mode, elite=a.elite, es_weights=a.es_weights, mean_lr=a.mean_lr,
                                keep_images=a.keep_images, out_prefix=os.path.join(a.path_to_gen, stem), path_to_gen=a.path_to_gen)
    moved = int((res["elite_used"] > 0).sum())
    print(f"best step {res['step']}  loss {res['loss']:.6f}  (the mean moved in {moved} of {len(res['elite_used'])} generations)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
