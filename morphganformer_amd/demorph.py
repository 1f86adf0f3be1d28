"""Reference-based latent de-morphing in gradient mode: given a suspected morph and ONE trusted image of a contributing subject, restore the
other contributor with the same generator (the defence side of "Transformer-based Face Morphing and De-Morphing"; the reference tree has no
such script -- the method follows from merge_morph's own definition, w_M = (1 - alpha) w_A + alpha w_B).

`drivers.demorph_latent` is the closed form w_B = (w_M - (1 - alpha) w_A) / alpha on two independent projections, whose errors it amplifies by
1 / alpha.  `DemorphEngine` is the coupled descent: two latent parameters p_A, p_B move together so that G((1 - alpha) p_A + alpha p_B) matches
the morph and G(p_A) the trusted image; the restored face is G(p_B).  The clean reference pins p_A, the morph then determines p_B.

    python -m morphganformer_amd.demorph --model net.pkl --morph morph.png --reference a.png [--w-morph m.mat --w-ref a.mat] --alpha 0.5 --out out/case
                                         (writes <out>_restored.mat / .png and <out>_reference.mat)
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from . import _lib
from .gradient_projection import GradientProjectionEngine
from .projection import ProjectionArgs, _as_latent, _wing_into


class DemorphEngine(GradientProjectionEngine):
    """The coupled descent.  Two lockstep generator rows, scored by the per-row terms of lockstep targets [morph, reference] (LPIPS, the pixel
    term and the biometric term against the row's own target, Wing with lm_target [2,68,2]), that are linear mixes of two parameters:

        latent_n = [p_A, p_B] + eps_i * sigma_i                                     (mgf_latent_perturb, unchanged)
        rows     = [[1 - alpha, alpha], [1, 0]] latent_n                            (mgf_latent_mix_f32; row 0 is merge_morph's blend bit for bit)
        total    = row_weight[0] * total(G(rows[0]), morph) + row_weight[1] * total(G(rows[1]), reference)
        d total / d [p_A, p_B] = the transposed mix of the weighted row gradients    (mgf_latent_mix_bwd_f32)
        p_A, p_B <- Adam (own moments each, one step counter);  keep (latent_n, i) if total < min_loss

    latent_in[0] = p_A and latent_in[1] = p_B; `start_a` / `start_b` are their starts ([k,D] or [1,k,D]; W+: [k,num_ws,D], or [k,D] broadcast over
    the slots), eps is [steps, 2, *latent] (row 0 perturbs p_A).  There is ONE job: one step counter, one `valid` table [steps] (a skipped step
    moves neither parameter), one min_loss / best_step, and the kept candidate is the perturbed parameter PAIR -- row 0 of the two-row loop state
    of the lockstep engine is this job's, row 1 of step_ctr / min_loss / best_step / losses stays unused.  `row_losses` [2, steps] holds every
    row's own unweighted total.  All of it is one device-resident launch sequence, replayed as a hipGraph like every engine.

    Not built (refused): optimize_noise, mdf, target_b, landmark detectors, retarget; an identity-separation term on G(p_B), several jobs in
    lockstep and more than two contributors."""

    def __init__(self, G, morph, reference, start_a, start_b, latent_std, args: ProjectionArgs = None, alpha=0.5, row_weight=(1.0, 1.0),
                 percept=None, biometric=None, gamma=1.0, use_mse=True, lm_target=None, lm_steps=None, lm_valid=None, eps=None, latent_space="z",
                 region_weight=None, face_crop=None, face_crop_target=None, face_crop_filter="area", use_graph=True, betas=(0.9, 0.999),
                 adam_eps=1e-8, weight_decay=0.0, noise_mode="random", seed=0, optimize_noise=False, mdf=None, target_b=None, landmark_fn=None,
                 landmark_model=None, wing_kind="wing"):
        alpha = float(alpha)
        if not 0.0 < alpha <= 1.0:
            raise ValueError(f"DemorphEngine: alpha must lie in (0, 1] (got {alpha}): the morph row is (1 - alpha) p_A + alpha p_B, and at alpha = 0 "
                             "p_B receives no gradient -- nothing would be restored")
        rw = np.asarray(row_weight, dtype=np.float64).reshape(-1)
        if rw.size != 2 or not np.all(np.isfinite(rw)) or rw[0] <= 0.0 or rw[1] < 0.0:
            raise ValueError(f"DemorphEngine: row_weight must be (morph weight > 0, reference weight >= 0) (got {row_weight!r}): p_B's only gradient "
                             "comes through the morph row")
        if optimize_noise:
            raise _lib.MgfError("DemorphEngine: optimize_noise=True is not built here (the noise maps are one set per engine, shared by both rows: "
                                "maps fitted to the morph and the reference at once would not belong to the restored face)")
        if noise_mode == "keyed" and not optimize_noise:
            raise _lib.MgfError("DemorphEngine: noise_mode='keyed' is not built here (its two generator rows share ONE step counter, and the keyed "
                                "launch of lockstep rows reads a counter per row); use 'random' or 'const'")
        if mdf is not None:
            raise _lib.MgfError("DemorphEngine: mdf= is not built here (the MDF objective runs with one target per engine; the two rows would need "
                                "per-row discriminator activations)")
        if target_b is not None:
            raise _lib.MgfError("DemorphEngine: target_b (morph refinement) does not combine with de-morphing: every row already has its own target, "
                                "`morph` and `reference`")
        if landmark_fn is not None or landmark_model is not None:
            raise _lib.MgfError("DemorphEngine: landmark detectors are wired for one target per engine; pass the rows' landmarks as tables "
                                "(lm_target [2,68,2], lm_steps [2,steps,68,2])")
        _lib.require_gpu(morph, reference, start_a, start_b)
        if tuple(morph.shape) != tuple(reference.shape) or morph.ndim != 4 or morph.shape[0] != 1:
            raise ValueError(f"DemorphEngine: morph and reference must both be [1,3,S,S] (got {tuple(morph.shape)} and {tuple(reference.shape)})")
        self.alpha = alpha
        ls = (G.cfg.k, G.cfg.num_ws, G.cfg.w_dim) if latent_space == "w+" else (G.cfg.k, G.cfg.z_dim)
        start = torch.stack([_as_latent(start_a, ls), _as_latent(start_b, ls)])
        target = torch.cat([morph.detach().float(), reference.detach().float()])
        # lm_valid stays out of the two-row state: this job has one [steps] table (below)
        super().__init__(G, target, start, latent_std, args, percept=percept, use_mse=use_mse, lm_target=lm_target, lm_steps=lm_steps, lm_valid=None,
                         eps=eps, noise_mode=noise_mode, seed=seed, use_graph=use_graph, biometric=biometric, gamma=gamma, wing_kind=wing_kind,
                         betas=betas, adam_eps=adam_eps, weight_decay=weight_decay, latent_space=latent_space, region_weight=region_weight,
                         face_crop=face_crop, face_crop_target=face_crop_target, face_crop_filter=face_crop_filter)
        dev = self.device
        if lm_valid is not None:
            self.valid = torch.as_tensor(np.asarray(lm_valid), dtype=torch.int32, device=dev).reshape(-1).contiguous()
            if self.valid.numel() < self.steps:
                raise ValueError(f"DemorphEngine: lm_valid is one table of {self.steps} steps (got {self.valid.numel()} entries)")
        # merge_morph's float32 coefficients (drivers._blend_latents) over the perturbed pair, and p_A itself
        self.coef = torch.as_tensor(np.array([[np.float32(1.0 - alpha), np.float32(alpha)], [1.0, 0.0]], dtype=np.float32), device=dev)
        self.row_weight = torch.as_tensor(rw.astype(np.float32), device=dev)
        self.rows = torch.zeros_like(self.latent_n)                      # the generator's input
        self.dparams = torch.zeros_like(self.latent_in)
        self.p_joint = torch.zeros(1, dtype=torch.float32, device=dev)
        self.w_joint = torch.zeros(1, dtype=torch.float64, device=dev)
        self.mse_joint = torch.zeros(1, dtype=torch.float32, device=dev)
        self.row_losses = self._reg(torch.full([2, self.steps], float("nan"), dtype=torch.float64, device=dev), float("nan"))

    def retarget(self, *args, **kw):
        raise _lib.MgfError("DemorphEngine: a de-morphing engine is not re-targeted (its two rows and their coupling belong to one morph / reference "
                            "pair); build a fresh one")

    def _make_rows(self):
        super()._make_rows()                                             # latent_n = [p_A, p_B] + eps * sigma
        _lib.check(_lib.lib().mgf_latent_mix_f32(self.rows.data_ptr(), self.latent_n.data_ptr(), self.coef.data_ptr(), 2, 2, self.numel,
                                                 _lib.stream_ptr()), "latent_mix")
        return self.rows

    def _apply_row_gradients(self, drows):
        _lib.check(_lib.lib().mgf_latent_mix_bwd_f32(self.dparams.data_ptr(), drows.data_ptr(), self.coef.data_ptr(), self.row_weight.data_ptr(),
                                                     2, 2, self.numel, _lib.stream_ptr()), "latent_mix_bwd")
        return self.dparams

    def _bookkeeping(self, dz, has_p):
        """Adam per parameter (both read the counter before select_best advances it), the rows' Wing terms, the joint slots, ONE best-of."""
        L, st, a, ctr, valid = _lib.lib(), _lib.stream_ptr(), self.args, self.step_ctr, self.valid
        for p in range(2):
            _lib.check(L.mgf_adam_step_f32(self.latent_in[p:].data_ptr(), self.exp_avg[p:].data_ptr(), self.exp_avg_sq[p:].data_ptr(),
                                           self.adam_t[p:].data_ptr(), dz[p:].data_ptr(), self.lr_table.data_ptr(), ctr.data_ptr(),
                                           _lib.ptr(valid), self.numel, self.steps, float(self.betas[0]), float(self.betas[1]),
                                           self.adam_eps, self.weight_decay, st), "adam_step")
        if self.use_wing:
            for b in range(2):
                _wing_into(self.wing_kind, self.w_loss[b:], self.lm_tables[b], self.lm_target[b], 1, ctr)
        p_loss, w_loss, mse_loss = (self.p_loss if has_p else None), (self.w_loss if self.use_wing else None), (self.mse_loss if self.use_mse else None)
        joint = lambda slot, src: None if src is None else slot
        _lib.check(L.mgf_joint_losses_f32(_lib.ptr(joint(self.p_joint, p_loss)), _lib.ptr(joint(self.w_joint, w_loss)),
                                          _lib.ptr(joint(self.mse_joint, mse_loss)), self.row_losses.data_ptr(), _lib.ptr(p_loss), _lib.ptr(w_loss),
                                          _lib.ptr(mse_loss), self.row_weight.data_ptr(), float(a.lamda), float(a.beta), ctr.data_ptr(),
                                          _lib.ptr(valid), 2, self.steps, st), "joint_losses")
        self._select_best(self.latent_n, 1, None, row=0, valid=valid, has_p=has_p, numel=2 * self.numel,
                          loss_slots=(self.p_joint, self.w_joint, self.mse_joint))

    def result(self):
        """dict(w_a, w_b: the best step's perturbed parameters, [1,k,D] or [1,k,num_ws,D] cpu; best_step; best_loss; losses [steps], the joint
        total; row_losses [2,steps], every row's own).  Raises like every engine when no step improved on min_loss_init."""
        torch.cuda.synchronize(self.device)
        bs = int(self.best_step[0].item())
        if bs < 0:
            raise IndexError("demorph: no iteration improved on the initial min_loss")
        best = self.best_latent.cpu().clone()
        return dict(w_a=best[0:1], w_b=best[1:2], best_step=bs, best_loss=float(self.min_loss[0].item()),
                    losses=self.losses[0].cpu().numpy(), row_losses=self.row_losses.cpu().numpy())

    def restored(self, truncation_psi=0.7, noise_mode="const"):
        """The restored accomplice: G(w_b), rendered like drivers.render_latent."""
        from .drivers import render_latent
        return render_latent(self.G, self.result()["w_b"], truncation_psi, noise_mode)


# ----------------------------------------------------------------------------------------------------------------- module entry
def build_parser():
    from . import cli
    ap = argparse.ArgumentParser(prog="python -m morphganformer_amd.demorph",
                                 description="Restore the second contributor of a suspected morph from one trusted image of the first (coupled "
                                             "latent descent, gradient mode)")
    ap.add_argument("--model", type=str, default="models/ffhq-snapshot-1024_v2.pkl")
    ap.add_argument("--morph", type=str, required=True, help="the suspected morph (image file)")
    ap.add_argument("--reference", type=str, required=True, help="the trusted image of one contributing subject")
    ap.add_argument("--w-morph", type=str, default=None, help=".mat latent of an earlier projection of --morph (with --w-ref: the start of the descent)")
    ap.add_argument("--w-ref", type=str, default=None, help=".mat latent of an earlier projection of --reference")
    ap.add_argument("--alpha", type=float, default=0.5, help="the morph's blend weight of the contributor to restore, in (0, 1]")
    ap.add_argument("--out", type=str, required=True, help="output prefix: <out>_restored.mat / .png, <out>_reference.mat")
    ap.add_argument("--row-weights", type=str, default="1,1", help="weights of the morph row and the reference row in the joint objective")
    ap.add_argument("--w_plus", action="store_true", help="descend W+ latents [k, num_ws, D] (follows the shape of --w-morph / --w-ref where given)")
    ap.add_argument("--pixel-term", choices=["mse", "dssim", "msssim"], default="mse", help="the pixel term, of the unquantised pixels")
    ap.add_argument("--ratio", type=float, default=1.0, help="height / width of the largest centred rectangle the restored image is cropped to")
    cli._objective_arguments(ap)
    cli._lpips_pool_argument(ap)
    ap.add_argument("--gpus", type=str, default="0", help="the visible device(s)")
    return ap


def main(argv=None):
    from . import cli
    a = build_parser().parse_args(argv)
    what = "demorph"
    if (a.w_morph is None) != (a.w_ref is None):
        raise SystemExit(f"{what}: --w-morph and --w-ref come together (the closed-form start needs both projections)")
    if not 0.0 < a.alpha <= 1.0:
        raise SystemExit(f"{what}: --alpha must lie in (0, 1] (got {a.alpha})")
    try:
        row_weight = tuple(float(v) for v in a.row_weights.split(","))
    except ValueError:
        raise SystemExit(f"{what}: --row-weights takes two numbers, e.g. 1,1 (got {a.row_weights!r})") from None
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("CUDA_VISIBLE_DEVICES", a.gpus)
    from . import drivers, loader
    print("Loading networks...")
    G = loader.load_network(a.model, device="cuda")["Gs"]
    args = cli._projection_args(a)
    percept = None if a.no_lpips else cli._lpips_term(a, what, device=G.device)
    biometric = cli._biometric_term(a, what, n=2, device=G.device)
    if percept is None and a.no_mse and biometric is None:
        raise SystemExit(f"{what}: every term of the objective is switched off")
    w_morph = None if a.w_morph is None else drivers.load_latent_mat(a.w_morph)
    w_ref = None if a.w_ref is None else drivers.load_latent_mat(a.w_ref)
    morph = drivers.image_transform(a.morph, size=a.size, device=G.device)
    reference = drivers.image_transform(a.reference, size=a.size, device=G.device)
    res = drivers.demorph(G, morph, reference, w_morph=w_morph, w_ref=w_ref, alpha=a.alpha, args=args, percept=percept, biometric=biometric,
                          gamma=a.gamma, use_mse=not a.no_mse, row_weight=row_weight, seed=a.seed, out_prefix=a.out, ratio=a.ratio,
                          latent_space="w+" if a.w_plus else None)
    print(f"best step {res['best_step']}  loss {res['best_loss']:.6f} (start {res['losses'][0]:.6f})  morph row {res['row_losses'][0][res['best_step']]:.6f}  "
          f"reference row {res['row_losses'][1][res['best_step']]:.6f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
