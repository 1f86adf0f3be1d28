"""Gradient mode of the projection loop: `GradientProjectionEngine`, the literal loop (projection.ProjectionEngine, its base class: loop
state, targets, graph capture, run loop) with the loss back-propagated into the latent.  Importable from `projection` too."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, misc
from .projection import ProjectionArgs, ProjectionEngine, _wing_into, get_lr, seeded_randn
from .trail import ImprovementSlot


class GradientProjectionEngine(ProjectionEngine):
    """Gradient mode: the same loop with the loss back-propagated into the latent.

        latent_n = latent_in + eps_i * sigma_i;  img = G(latent_n)
        total = percept_weight * LPIPS + lamda * Wing + beta * (MSE | DSSIM | MS-SSIM) [+ gamma * embedding MSE]     (Wing's landmarks come from a
                                                                                                           detector: no gradient)
        latent_in <- Adam(lr_i = get_lr(i / steps)).step(d total / d latent_in);  keep (latent_n, i) if total < min_loss

    i.e. the drivers' loop (...sqz_MSE.py:143-189) with the `.cpu().detach().numpy()` at :158 removed.  One candidate per target
    and step (the steps now depend on each other); forward, losses, backward (grad.GeneratorGrad, LPIPS / embedder backward),
    Adam and the best-of bookkeeping are one device-resident launch sequence, replayed as a hipGraph.  The oracle is torch
    autograd + torch.optim.Adam through the CPU restatement (oracle/loss_ref.py: projection_gradient_ref).

    `target` may hold B > 1 images: B independent projections (own latent, Adam state, noise stream, landmarks, best-so-far)
    advance in lockstep through ONE generator forward/backward per step -- the batch that lifts the 4x4..64x64 layers off
    their batch-1 latency floor (BASELINE configs 3 and 5 are batches of independent targets).  lm_target is then [B,68,2],
    lm_steps [B,steps,68,2], lm_valid [B,steps], eps [steps,B,k,D]; `result()` returns per-target lists.

    target_b (morph refinement): every projection matches TWO identities, `target` weighted 1 - morph_alpha and target_b weighted morph_alpha
    (merge_morph's convention; a float or one value per pair):
        total = percept_weight [(1-a) LPIPS(x,Ta) + a LPIPS(x,Tb)] + beta [(1-a) P(x,Ta) + a P(x,Tb)] + lamda Wing
                + gamma [(1-a) d_a + a d_b] + id_balance |d_a - d_b|,     d_t = d(embed(x), embed(T_t)), id_metric "mse" or "cosine"
    lm_target_b blends the Wing term's target landmarks the same way; `id_trace` [B,steps,2] holds (d_a, d_b) per step.  See _init_pair."""
    _lockstep = True

    def __init__(self, G, target, latent_mean, latent_std, args: ProjectionArgs = None, percept=None, use_mse=True, lm_target=None,
                 lm_steps=None, lm_valid=None, eps=None, noise_mode="random", seed=0, use_graph=True, landmark_fn=None, biometric=None,
                 gamma=1.0, wing_kind="wing", landmark_model=None, betas=(0.9, 0.999), adam_eps=1e-8, weight_decay=0.0,
                 latent_space="z", mdf=None, optimize_noise=False, noise_init="randn", target_b=None, morph_alpha=0.5, id_balance=0.0,
                 id_metric="mse", lm_target_b=None, region_weight=None, face_crop=None, face_crop_target=None, face_crop_target_b=None,
                 face_crop_filter="area", noise_per_target=False, **ignored):
        """latent_space: "z" -- the drivers' parameter, the gradient runs on through the mapping network -- or "w+": the parameter is the
        per-layer intermediate latent ws [k, num_ws, D] itself (north_star: "backprops into the k-component latent W+"; layer `slot` reads
        ws[:, slot], networks.py:1252-1253), perturbed, descended by Adam and kept best-of exactly like z.  latent_mean is then a w-space
        start -- [k, D] (broadcast over the slots, e.g. latent_stats_w's mean) or [k, num_ws, D] -- and latent_std a w-space scale.  The
        reference has no such driver (its "W+" averages 18 copies of z, projection_example_v2_percept.py:133-162); the oracle is torch autograd
        + Adam on ws through the CPU restatement (tests/test_hip_gradient.py).

        optimize_noise: the generator's per-layer noise inputs become parameters next to the latent, as in the StyleGAN2-style projectors the
        drivers derive from (they still carry noise_regularize / noise_normalize_ and the --noise_regularize flag, :32-60, :243): the maps are
        engine-owned tensors (`noise_init`: "randn", seeded, or "const", a copy of every layer's noise_const) the generator runs with
        (`noise_mode` is then irrelevant, "keyed" included), the total gains args.noise_regularize * sum over the maps of the regulariser, and every step the maps take
        an Adam step with the latent's learning rate and betas followed by noise_normalize_.  `noises` holds the current maps, `best_noises`
        those of the best step's image ({layer name: [B, res, res]}, row j: target j), both filled inside the launch sequence.  Every target
        owns a SET of maps (one target: a set of one): the maps, their gradient, the Adam moments and the best step's maps are [B, total]
        buffers (`noise_flat`, ...; a row is one target's maps back to back), `noises` / `best_noises` / `dnoises` hold views into them, the
        optimizer count is [B]; with noise_init="randn" target j draws its maps under seed + 0x6E6F6973 + j, with "const" every target
        starts from the layers' noise_const.  Regulariser, Adam and normalisation are one call each over all targets and maps (the
        mgf_noise_sets_* entries: a launch count that depends on neither), each target gated by its own step counter and `valid` row; with
        B > 1 the generator reads a dense per-layer copy of the maps ([B, res, res] per layer, one pack launch per step), with B = 1 the
        maps themselves.

        noise_per_target (with optimize_noise): B > 1 lockstep targets optimise noise maps only when this says so (each then fits its OWN
        maps; maps shared by the batch are not built).  With one target the keyword changes nothing.

        region_weight: as ProjectionEngine's; with B lockstep targets one map for all of them or [B,1,H,W], one per target.  A target pair's
        constants (alpha (1 - alpha) LPIPS_W(Ta, Tb) and the same of the pixel term) use the weighted values.  The noise regulariser ignores it."""
        from .grad import GeneratorGrad
        pair = self._pair_arguments(target, target_b, morph_alpha, id_balance, id_metric, biometric, mdf, optimize_noise, lm_target, lm_target_b)
        if pair is not None:
            # the pixel target of the MSE term and the Wing term's landmarks are the blends: what the single-target code below is handed
            target, lm_target = pair["blend"], pair["lm_blend"]
        if noise_init not in ("randn", "const"):
            raise ValueError(f"noise_init must be 'randn' or 'const' (got {noise_init!r})")
        if noise_per_target and not optimize_noise:
            raise ValueError("GradientProjectionEngine: noise_per_target=True gives every lockstep target its own noise maps to optimise: pass "
                             "optimize_noise=True with it")
        if optimize_noise and int(target.shape[0]) > 1 and not noise_per_target:
            raise _lib.MgfError("GradientProjectionEngine: optimize_noise runs with one target per engine (lockstep targets share one generator "
                                "forward, whose noise maps are shared by the batch; per-target maps are not built); project the targets one after the other"
                                " -- or pass noise_per_target=True: a set of maps per target")
        if mdf is not None and not getattr(mdf, "differentiable", False):
            raise _lib.MgfError("GradientProjectionEngine: this MDF loss was built without its backward pass -- build it with "
                                "mdf.MDFLoss(..., differentiable=True) for gradient mode (ProjectionEngine(mdf=...), the literal loop, takes either)")
        if mdf is not None and int(target.shape[0]) > 1:
            raise _lib.MgfError("GradientProjectionEngine: the MDF objective runs with one target per engine (lockstep targets would need "
                                "per-target discriminator activations); project the targets one after the other")
        a = args or ProjectionArgs()
        if a.latent_copies != 1:
            raise _lib.MgfError("GradientProjectionEngine: latent_copies is the literal-mode v2 driver's averaged latent (projection_example_v2_percept.py); "
                                "gradient mode optimises one latent")
        if a.pixel_term not in ("mse", "dssim", "msssim") or a.pool_above:
            raise _lib.MgfError("GradientProjectionEngine: pixel_term='psnr', pixel_term='lbp' and pool_above are literal-mode objectives with no backward pass "
                                "here: PSNR as the script minimises it descends towards a LARGER error, the LBP distance is a histogram of integer codes "
                                "(its gradient is zero almost everywhere), and pool_above is the v1 driver's block mean in front of EVERY image-space loss, which has "
                                "no adjoint here (the LPIPS term alone has one: percept=PerceptualLoss(pool_above=N)); gradient mode descends Wing / LPIPS / MSE / DSSIM / MS-SSIM / biometric / MDF")
        assert latent_space in ("z", "w+"), latent_space
        self.latent_space = latent_space
        ls = (G.cfg.k, G.cfg.num_ws, G.cfg.w_dim) if latent_space == "w+" else (G.cfg.k, G.cfg.z_dim)
        B = int(target.shape[0])
        assert B == 1 or (landmark_fn is None and landmark_model is None), "landmark detectors are wired for one target per engine"
        self.pair, self.id_trace, self.optimize_noise = pair, None, bool(optimize_noise)
        self.noises = self.best_noises = self.noise_slot = self.noise_slots = None
        # one candidate per target and step, nothing pipelined, no improvement trail; B > 1 targets get a row each of the loop state (_init_state)
        super().__init__(G, target, latent_mean, latent_std, args, percept=percept, use_mse=use_mse, lm_target=lm_target,
                         lm_steps=lm_steps, lm_valid=lm_valid, eps=eps, noise_mode=noise_mode, seed=seed, use_graph=use_graph, batch=1,
                         landmark_fn=landmark_fn, biometric=biometric, gamma=gamma, wing_kind=wing_kind,
                         landmark_model=landmark_model, pipeline=False, keep_images=0, latent_shape=ls, mdf=mdf, region_weight=region_weight,
                         face_crop=face_crop, face_crop_target=face_crop_target, face_crop_target_b=face_crop_target_b,
                         face_crop_filter=face_crop_filter)
        self.targets = B
        a, dev = self.args, self.device
        if biometric is not None:
            biometric.embedder.keep_activations = True          # FaceEmbedder's contract (the FaceNet embedder re-uses its buffers block after block otherwise)
        self.gg = GeneratorGrad(G)
        self.betas, self.adam_eps, self.weight_decay = betas, float(adam_eps), float(weight_decay)
        self.lr_table = torch.as_tensor(np.array([get_lr(i / a.step, a.lr, a.lr_rampdown, a.lr_rampup) for i in range(a.step)],
                                                 dtype=np.float32), device=dev)
        # Adam moves the start latent: state here (the literal loop never writes it), and like the moments not rewound -- a rewound engine
        # goes on from where the descent stands
        self._reg(self.latent_in)
        self.exp_avg = self._reg(torch.zeros_like(self.latent_in))
        self.exp_avg_sq = self._reg(torch.zeros_like(self.latent_in))
        self.adam_t = self._reg(torch.zeros(B, dtype=torch.int32, device=dev))
        self.dimg = torch.zeros_like(self.target)
        if self.optimize_noise:
            self._init_noise(noise_init, seed)
        if pair is not None:
            self._init_pair(float(id_balance), id_metric)

    @staticmethod
    def _pair_arguments(target, target_b, morph_alpha, id_balance, id_metric, biometric, mdf, optimize_noise, lm_target, lm_target_b):
        """Checks of the two-identity objective, and its blended single-target inputs.  None without target_b."""
        if target_b is None:
            if lm_target_b is not None or float(id_balance) != 0.0:
                raise ValueError("GradientProjectionEngine: lm_target_b and id_balance belong to a target pair: pass target_b")
            return None
        if mdf is not None:
            raise _lib.MgfError("GradientProjectionEngine: target_b (morph refinement) does not combine with mdf=: the MDF loss is not a sum of "
                                "quadratic terms against stored target activations, so it would need a second evaluation per step, which is not built")
        if optimize_noise:
            raise _lib.MgfError("GradientProjectionEngine: target_b (morph refinement) does not combine with optimize_noise=True (noise maps fitted "
                                "to two images at once are not built)")
        if float(id_balance) != 0.0 and biometric is None:
            raise ValueError("GradientProjectionEngine: id_balance weighs |d_a - d_b| of the biometric term: pass biometric= with it")
        if float(id_balance) < 0.0:
            raise ValueError(f"GradientProjectionEngine: id_balance must be >= 0 (got {id_balance})")
        if id_metric not in ("mse", "cosine"):
            raise ValueError(f"GradientProjectionEngine: id_metric must be 'mse' or 'cosine' (got {id_metric!r})")
        _lib.require_gpu(target, target_b)
        if tuple(target_b.shape) != tuple(target.shape):
            raise ValueError(f"GradientProjectionEngine: target and target_b do not pair up: {tuple(target.shape)} vs {tuple(target_b.shape)}")
        B = int(target.shape[0])
        al = misc.as_numpy(morph_alpha, np.float64).reshape(-1)
        if al.size not in (1, B):
            raise ValueError(f"GradientProjectionEngine: morph_alpha must be one value or one per pair ({B}), got {al.size}")
        if not np.all((al >= 0.0) & (al <= 1.0)):
            raise ValueError(f"GradientProjectionEngine: morph_alpha must lie in [0, 1] (got {al.tolist()}): the objective's reduction to one "
                             "blended target holds for convex weights only")
        al = np.array(np.broadcast_to(al, (B,)))
        ta = target.detach().float().clone(memory_format=torch.contiguous_format)
        tb = target_b.detach().float().clone(memory_format=torch.contiguous_format)
        blend = torch.empty_like(ta)
        for j in range(B):                  # alpha exactly 0 or 1: that target's own bits (the end points equal the single-target engine)
            a = float(al[j])
            blend[j] = ta[j] if a == 0.0 else (tb[j] if a == 1.0 else ta[j] * (1.0 - a) + tb[j] * a)
        lm_blend = lm_target
        if lm_target_b is not None:
            if lm_target is None:
                raise ValueError("GradientProjectionEngine: lm_target_b needs lm_target (the first identity's landmarks)")
            la, lb = np.asarray(lm_target, dtype=np.float64), np.asarray(lm_target_b, dtype=np.float64)
            if la.shape != lb.shape:
                raise ValueError(f"GradientProjectionEngine: lm_target and lm_target_b do not pair up: {la.shape} vs {lb.shape}")
            w = al.reshape((B,) + (1,) * (la.ndim - 1)) if (B > 1 or la.ndim == 3) else float(al[0])
            lm_blend = (1.0 - w) * la + w * lb
        return dict(ta=ta, tb=tb, alpha=al, blend=blend, lm_blend=lm_blend)

    def _init_pair(self, id_balance, id_metric):
        """Two identities per projection (morph refinement).  Every quadratic term against (Ta weighted 1 - alpha, Tb weighted alpha) equals
        the same term against one blended target plus a constant, so LPIPS, MSE and their backward run once per step on blends -- the cached
        unit taps (PerceptualLoss.set_target_pair) and the pixel blend `self.target` -- and the constants are added on the device; DSSIM and
        MS-SSIM are evaluated against both targets (PixelTerm.set_pair); the identity term (balance |d_a - d_b|, cosine metric) is
        mgf_embed_pair_loss_f32."""
        P, a, dev, B = self.pair, self.args, self.device, self.targets
        al = P["alpha"]
        self.pair_alpha = torch.as_tensor(al, dtype=torch.float32, device=dev)
        if self.percept is not None:
            self.percept.set_target_pair(P["ta"], P["tb"], al)
            self.pair_p_off = self.percept.pair_offset * float(a.percept_weight)          # percept_weight * alpha (1 - alpha) LPIPS(Ta, Tb)
        self.pixel.set_pair(P["ta"], P["tb"], al)
        if self.biometric is not None:
            self.biometric.set_target_pair(P["ta"], P["tb"], al, id_balance=id_balance, metric=id_metric)
            self.id_trace = self._reg(torch.full([B, self.steps, 2], float("nan"), dtype=torch.float64, device=dev), float("nan"))
            self.biometric.pair_trace = (self.id_trace, self.step_ctr)

    def retarget(self, *args, **kw):
        if self.pair is not None:
            raise _lib.MgfError("GradientProjectionEngine: an engine built on a target pair is not re-targeted; build a fresh one")
        if self.targets > 1:
            raise _lib.MgfError("GradientProjectionEngine: an engine of lockstep targets is not re-targeted; build a fresh one")
        return super().retarget(*args, **kw)

    def _init_noise(self, noise_init, seed):
        """The noise maps as parameters, a SET of maps per target (one target: a set of one): [B, total] buffers for the maps, their gradient,
        the two Adam moments and the best step's maps (a row is one target's maps back to back), [B, res, res] views per layer for the
        generator and the backward pass, and the map table (sides and offsets inside a row) the mgf_noise_sets_* entries take."""
        G, dev, L, B = self.G, self.device, _lib.lib(), self.targets
        layers = [lp for lp in G.plan.layers if lp.noise_strength is not None]
        total = sum(lp.res * lp.res for lp in layers)
        z = lambda: torch.zeros(B, total, dtype=torch.float32, device=dev)
        self.noise_flat, self.noise_grad, self.noise_m, self.noise_v = self._reg(z()), z(), self._reg(z()), self._reg(z())
        self.best_noise_flat = self._reg(z(), 0)
        if noise_init == "randn":                   # (streams of their own, not the head of the latent's eps stream)
            for j in range(B):
                self.noise_flat[j].copy_(seeded_randn((total,), dev, int(seed) + 0x6E6F6973 + j))
        self.noises, self.best_noises, self.dnoises, self.noise_layers = {}, {}, {}, []
        # what the generator reads: B dense maps per layer.  One target: the maps themselves
        self.noise_dense = torch.zeros(B * total, dtype=torch.float32, device=dev) if B > 1 else None
        self.gen_noises = {} if B > 1 else self.noises
        off, offsets = 0, []
        for lp in layers:
            r = lp.res
            if noise_init == "const":
                self.noise_flat[:, off:off + r * r].copy_(lp.noise_const.reshape(1, -1).expand(B, -1))
            view = lambda t: t[:, off:off + r * r].view(B, r, r)
            self.noises[lp.name], self.best_noises[lp.name], self.dnoises[lp.name] = view(self.noise_flat), view(self.best_noise_flat), view(self.noise_grad)
            if B > 1:
                self.gen_noises[lp.name] = self.noise_dense[B * off:B * (off + r * r)].view(B, r, r)
            self.noise_layers.append((lp.name, r))
            offsets.append(off)
            off += r * r
        self.noise_total = total
        self.noise_sides, self.noise_offsets, self.noise_maps = _lib.map_table([r for _, r in self.noise_layers], offsets)
        self.noise_adam_t = self._reg(torch.zeros(B, dtype=torch.int32, device=dev))
        self.noise_ctr = torch.zeros(B, dtype=torch.int32, device=dev)      # the step counters as they stood before select_best advanced them
        # target j's improvement flag of select_best: take[0] = 0 where this step improved, else -1 (_noise_update reads it after the launch
        # that wrote it); `noise_slot` is target 0's
        self.noise_slots = [ImprovementSlot(1, 1, dev) for _ in range(B)]
        self.noise_slot = self.noise_slots[0]
        for slot in self.noise_slots:
            self._table += slot.state(with_take=True)
        nbytes = int(L.mgf_noise_sets_scratch_bytes(self.noise_sides, self.noise_maps, B))
        if nbytes <= 0:
            raise _lib.MgfError(f"GradientProjectionEngine: optimize_noise: the set kernels do not take this generator's maps (sides "
                                f"{[r for _, r in self.noise_layers]}: at most 32 maps, powers of two)")
        self.noise_scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        self.gg.noise_grads = True

    def _valid_rows(self):
        """(pointer, row stride) of the `valid` table as the set kernels take it: a row per target."""
        if self.valid is None:
            return 0, 0
        return self.valid.data_ptr(), (int(self.valid.shape[-1]) if self.targets > 1 else 0)

    def _noise_pack(self):
        """The generator's dense per-layer maps from the targets' sets (B > 1; in front of the forward pass, so that maps written from outside
        between steps count, as they do with one target, whose maps the generator reads in place)."""
        if self.noise_dense is not None:
            _lib.check(_lib.lib().mgf_noise_sets_pack_f32(self.noise_dense.data_ptr(), self.noise_flat.data_ptr(), self.noise_offsets, self.noise_sides,
                                                          self.noise_maps, self.targets, self.noise_total, _lib.stream_ptr()), "noise_sets_pack")

    def _noise_regularize(self, has_p):
        """One call for every target: p_loss[j] (+)= noise_regularize * sum_maps reg of target j's maps, added map after map in float32, and
        noise_grad += noise_regularize * d reg / d maps (the regulariser rides in the float32 p_loss slot like the biometric and MDF terms;
        select_best forms the total in float64)."""
        _lib.check(_lib.lib().mgf_noise_sets_regularize_grad_f32(
            self.noise_grad.data_ptr(), self.p_loss.data_ptr(), 1, self.noise_flat.data_ptr(), self.noise_offsets, self.noise_sides, self.noise_maps,
            self.targets, self.noise_total, float(self.args.noise_regularize), 1, int(has_p), self.noise_scratch.data_ptr(), _lib.stream_ptr()),
            "noise_sets_regularize_grad")

    def _noise_update(self):
        """After select_best: keep the maps of each improving target (they still are the ones its image was generated with), then move them --
        one Adam call on d total / d maps = the generator's d<img, dimg>/d maps (already in noise_grad) + noise_regularize * d reg / d maps,
        one noise_normalize_ call over every map; a target's skipped step moves none of its maps (its own counter and `valid` row gate its
        slices inside the kernels)."""
        L, st, B = _lib.lib(), _lib.stream_ptr(), self.targets
        for j in range(B):
            _lib.check(L.mgf_keep_improvements(self.best_noise_flat[j].data_ptr(), self.noise_flat[j].data_ptr(), self.noise_total,
                                               self.noise_slots[j].take.data_ptr(), 1, st), "keep_improvements(noise maps)")
        vptr, vstride = self._valid_rows()
        _lib.check(L.mgf_adam_sets_f32(self.noise_flat.data_ptr(), self.noise_m.data_ptr(), self.noise_v.data_ptr(), self.noise_adam_t.data_ptr(),
                                       self.noise_grad.data_ptr(), self.lr_table.data_ptr(), self.noise_ctr.data_ptr(), 1, vptr, vstride,
                                       self.noise_total, B, self.noise_total, self.steps, float(self.betas[0]), float(self.betas[1]), self.adam_eps,
                                       self.weight_decay, st), "adam_sets")
        _lib.check(L.mgf_noise_sets_normalize_f32(self.noise_flat.data_ptr(), self.noise_offsets, self.noise_sides, self.noise_maps, B,
                                                  self.noise_total, self.noise_ctr.data_ptr(), 1, vptr, vstride, self.steps,
                                                  self.noise_scratch.data_ptr(), st), "noise_sets_normalize")

    def _noise_kw(self, ctr):
        """noise_mode="keyed": row t of the forward is target t at ITS step -- stride 1 over the per-target counters, nothing added per row --
        so a target of a lockstep group draws what a one-target engine on it draws."""
        kw = super()._noise_kw(ctr)
        if kw["noise_mode"] == "keyed":
            kw.update(noise_step_stride=1 if self.targets > 1 else 0, noise_step_add=0, noise_aux=(1, 0))
        return kw

    # The three points at which a subclass couples the rows (demorph.DemorphEngine: rows that are linear mixes of parameters).  Here a row IS
    # a parameter: the hooks add no launch and reorder none.
    def _make_rows(self):
        """Perturb the parameters and return the generator's input rows [B, *latent shape]."""
        # B targets: one flat parameter of B * numel floats, one noise row [B * numel] per step
        _lib.check(_lib.lib().mgf_latent_perturb(self.latent_n.data_ptr(), self.latent_in.data_ptr(), self.eps.data_ptr(), self.sigma.data_ptr(),
                                                 self.step_ctr.data_ptr(), 1, self.steps, self.targets * self.numel, _lib.stream_ptr()), "latent_perturb")
        return self.latent_n

    def _apply_row_gradients(self, drows):
        """The parameters' gradient [B, *latent shape] from the rows' (the generator backward's output)."""
        return drows

    def _bookkeeping(self, dz, has_p):
        """Per-target optimizer step, Wing term and best-of bookkeeping (tiny launches)."""
        L, st, B = _lib.lib(), _lib.stream_ptr(), self.targets
        for j in range(B):
            ctr = self.step_ctr[j:]
            valid = None if self.valid is None else (self.valid[j] if B > 1 else self.valid)
            _lib.check(L.mgf_adam_step_f32(self.latent_in[j:].data_ptr(), self.exp_avg[j:].data_ptr(), self.exp_avg_sq[j:].data_ptr(),
                                           self.adam_t[j:].data_ptr(), dz[j:].data_ptr(), self.lr_table.data_ptr(), ctr.data_ptr(),
                                           _lib.ptr(valid), self.numel, self.steps, float(self.betas[0]), float(self.betas[1]),
                                           self.adam_eps, self.weight_decay, st), "adam_step")
            if self.use_wing:
                _wing_into(self.wing_kind, self.w_loss[j:], self.lm_tables[j], self.lm_target[j] if B > 1 else self.lm_target, 1, ctr)
            self._select_best(self.latent_n[j:], 1, self.noise_slots[j] if self.noise_slots else None, row=j, valid=valid, has_p=has_p)

    def _iteration(self):
        a, B = self.args, self.targets
        rows = self._make_rows()
        opt_noise = self.optimize_noise
        if opt_noise:
            self._noise_pack()
        nkw = dict(noise_mode="inject", noises=self.gen_noises) if opt_noise else self._noise_kw(self.step_ctr)
        if self.latent_space == "w+":
            img = self.gg.forward(ws=rows, **nkw)                                 # [B, k, num_ws, D]: every layer reads its own slot
        else:
            img = self.gg.forward(rows, **nkw)                                    # psi lands in `c` in the drivers: no truncation
        if B == 1:
            self._landmarks(img)                                                  # before Adam: a "no face" step must not move the latent
        tstride = img.numel() // B if B > 1 else 0
        pair = self.pair
        # dimg = beta * d pixel term / d img (zero without one); the window terms write their value with it, the MSE value follows below
        self.pixel.grad_into(self.dimg, self.mse_loss, img, self.target, B, tstride, float(a.beta), 0)
        if self.percept is not None:
            self.percept.distance_into(self.p_loss, img, keep_taps=True)
            self.percept.grad_into(self.dimg, scale=float(a.percept_weight), accumulate=True)
            if a.percept_weight != 1.0:
                self.p_loss.mul_(float(a.percept_weight))
            if pair is not None:            # the constant the blended taps leave out: `losses` holds the pair objective, not a shifted one
                self.p_loss.add_(self.pair_p_off)
        if self.biometric is not None:      # rides in the p_loss slot, like the literal loop (a target pair: one launch of the pair kernel)
            self.biometric.distance_into(self.p_loss, img, scale=self.gamma, accumulate=self.bio_accumulate)
            self.biometric.grad_into(self.dimg, scale=self.gamma, accumulate=True)
        if self.mdf is not None:            # p_loss (+)= MDF, dimg += d MDF / d img (1024_example_mdfloss.py:165 without the detach)
            self.mdf.distance_into(self.p_loss, img, accumulate=self.mdf_accumulate, dimg=self.dimg, grad_accumulate=True)
        self.pixel.value_after_grad_into(self.mse_loss, img, self.target, B, tstride)
        if opt_noise:
            dz = self.gg.backward_ws(self.dimg, dnoises=self.dnoises) if self.latent_space == "w+" else self.gg.backward(self.dimg, dnoises=self.dnoises)
        else:
            dz = self.gg.backward_ws(self.dimg) if self.latent_space == "w+" else self.gg.backward(self.dimg)
        dz = self._apply_row_gradients(dz)
        has_p = self.has_p or opt_noise
        if opt_noise:
            self._noise_regularize(self.has_p)
            self.noise_ctr.copy_(self.step_ctr)
        self._bookkeeping(dz, has_p)
        if opt_noise:
            self._noise_update()
        return img

    def result(self):
        """One target: like ProjectionEngine.result().  B targets: (best_latents [B,k,D] cpu, best_steps [B], best_losses [B],
        losses [B,steps]) as numpy / tensors; a target that never improved on min_loss_init raises like the reference."""
        if self.targets == 1:
            return super().result()
        torch.cuda.synchronize(self.device)
        bs = self.best_step.cpu().numpy()
        if (bs < 0).any():
            raise IndexError(f"projection: targets {np.nonzero(bs < 0)[0].tolist()} never improved on the initial min_loss")
        return self.best_latent.cpu().clone(), bs, self.min_loss.cpu().numpy(), self.losses.cpu().numpy()
