"""The latent-projection loop of the reference drivers (1024_example_wing_loss_perceptual_sqz_MSE.py:131-208 and its
MSE / percept / Wing siblings), device-resident on MI355X.

Semantics ("literal" mode = what the reference computes).  Every driver detaches the generator output
to numpy before any loss, so `latent_in` never receives a gradient and Adam is inert; the loop is a best-of-N noisy search
around `latent_mean`:

    for i in range(steps):
        t = i / steps
        sigma = latent_std * noise * max(0, 1 - t / noise_ramp) ** 2                  (:156)
        latent_n = latent_in + randn_like(latent_in) * sigma                          (:157, :71-73)
        img = G(latent_n, 0.7)[0]      # 0.7 lands in `c`; no truncation; noise_mode="random"   (:158)
        total = LPIPS(img, target) + lamda * Wing(landmarks(img), landmarks(target)) + beta * MSE(img, target)   (:173-179)
        if total < min_loss: min_loss, best = total, latent_n                         (:186-189)

One iteration is a fixed sequence of HIP kernel launches with all loop state (step counter, best-so-far, loss history)
on the device, captured once into a hipGraph and replayed: no PCIe copy and no host synchronisation per step (the
reference makes three crossings of 12.6 MB per step).  Landmark extraction is dlib on the host in the reference
(:159-170) -- a third-party detector that is not reproducible offline -- so landmarks enter as an injected [steps,68,2]
float64 table (and a `valid` table for the "no face found -> continue" branch, :165-166).

`GradientProjectionEngine` (gradient_projection.py, importable from here) is the gradient-descent reading of the north star (the loss is
back-propagated into the latent and Adam moves it) -- the loop the drivers set up (optimizer, lr schedule) but never get (the detach severs it).
"""
from __future__ import annotations

import math
import os
import weakref
from dataclasses import dataclass
from functools import partial

import numpy as np
import torch

from . import _lib, misc
from .pixel_term import MSSSIM_WEIGHTS, PixelTerm, msssim_max_levels, msssim_weights  # noqa: F401  (the MS-SSIM helpers are public here)
from .trail import ImprovementTrail


@dataclass
class ProjectionArgs:
    """argparse defaults of the reference driver (...sqz_MSE.py:224-245)."""
    step: int = 5000
    lamda: float = 0.01
    beta: float = 1.0
    lr: float = 0.01
    lr_rampup: float = 0.05
    lr_rampdown: float = 0.25
    noise: float = 0.05
    noise_ramp: float = 0.75
    truncation_psi: float = 0.7
    n_mean_latent: int = 10000
    ratio: float = 1.0
    percept_weight: float = 1.0     # coefficient of the LPIPS term: 1 in the Wing/LPIPS/MSE drivers, 0.5 in 1024_example_percept_MSE.py:147
    min_loss_init: float = 100.0
    # "mse": beta * MSE(img, target), the drivers' pixel term.  "psnr": the pixel term of 1024_example_PSNR.py:113-114,158 --
    # 10 log10(255^2 / mean((p0 - p1)^2)) on the [-1, 1] float images, MINIMISED like every other loss of these loops (:173-175 keeps
    # the candidate with the smallest value; the script's objective as written, not a claim that it is a sensible one).  AS WRITTEN also
    # covers the element order (`psnr_layout="script"`, the default): :150-153 permute the generated image and tensor2np it back into
    # C-H-W order, tensor2np the target into H-W-C order, and :158 compares the two FLATTENED arrays -- element i of the candidate's
    # CHW stream against element i of the target's HWC stream, i.e. different pixels and channels.  `psnr_layout="aligned"` is the PSNR the
    # function defines on corresponding pixels (a deliberate deviation from the script; ranks candidates by their MSE)
    # "dssim": `dssim` of 1024_example_SSIM.py:115-117 (= lpips/__init__.py:54-55), (1 - SSIM) / 2 with skimage's defaults, on the uint8
    # images (the generated image as the drivers save it, misc.to_pil) -- the function as defined; the script's own call site (:158) passes
    # flattened float arrays, which compare_ssim rejects.  That is the literal loop (mgf_dssim_u8_f32).  Gradient mode descends the SAME function
    # on the unquantised pixels 127.5 x + 127.5 (mgf_dssim_grad_f32: the rint / clip has gradient zero almost everywhere); the two agree to float32
    # rounding on images that lie on the uint8 grid
    # "lbp": the matching distance of 1024_example_LBP_percept.py:34-58,162-166 -- 1 - cos(LBP(24, 3, 'uniform') code map of the saved image at
    # 224 x 224, the target file's code map) in float64 -- in place of every other term (the script scores nothing else); needs
    # ProjectionEngine(lbp_target=lbp.target_feature(file pixels))
    # "msssim": 1 - multi-scale SSIM (Wang, Simoncelli, Bovik 2003: 11-tap Gaussian windows, sigma 1.5, `msssim_levels` levels of a 2 x 2 mean pyramid,
    # the usual level weights renormalised over the levels in use -- msssim_weights), the structural term of the MIPGAN family of morph optimisers.
    # The reference tree has no such script; the definition is include/mgf.h's (mgf_msssim_f32).  BOTH loops use the continuous form on the
    # unquantised pixels 127.5 x + 127.5 (no script defines a quantised one): the literal loop scores with mgf_msssim_f32, gradient mode descends
    # mgf_msssim_grad_f32.  Every level's sides must be >= 11: 1024^2, 256^2 and 161 x 176 take five levels, 64^2 three
    pixel_term: str = "mse"
    msssim_levels: int = 5
    psnr_layout: str = "script"
    # projection_example_v2_percept.py:131-166: the optimised latent holds `latent_copies` (18 there) copies of the start latent, every copy
    # receives its own noise each step and the generator sees their mean (`torch.mean(latent_n, 1)`, reproduced in torch's summation order:
    # the kept latent -- that mean -- is bit-exact); 1 = the other drivers' single latent.  Literal mode; eps is then [steps, 1, copies, k, D]
    latent_copies: int = 1
    # projection_example_v1.py:150-155: a generated image taller than `pool_above` pixels is block-averaged by height // pool_above before
    # the image-space losses (the target is then given at the pooled size, :84-92 resize it to 256); 0 = off (the 1024 drivers)
    pool_above: int = 0
    # `--noise_regularize` of the drivers (:243): the weight of noise_regularize(noises) (:32-52).  Their loop never calls the function (it never
    # back-propagates); GradientProjectionEngine(optimize_noise=True) adds noise_regularize * sum over the maps to its total.  Unused otherwise
    noise_regularize: float = 1e5

    def __post_init__(self):
        if self.pixel_term == "msssim" and not (isinstance(self.msssim_levels, int) and 1 <= self.msssim_levels <= len(MSSSIM_WEIGHTS)):
            raise _lib.MgfError(f"projection: msssim_levels must be an integer in 1..{len(MSSSIM_WEIGHTS)} (got {self.msssim_levels!r})")

    def pool_factor(self, resolution):
        """The block side `pool_above` averages a resolution x resolution image by (1 = not pooled): the losses see resolution // factor pixels."""
        return misc.pool_factor(resolution, self.pool_above)


def get_lr(t, initial_lr, rampdown=0.25, rampup=0.05):
    """Learning-rate schedule of the drivers (:63-68).  Inert in literal mode (the optimizer never sees a gradient)."""
    lr_ramp = min(1, (1 - t) / rampdown)
    lr_ramp = 0.5 - 0.5 * math.cos(lr_ramp * math.pi)
    lr_ramp = lr_ramp * min(1, t / rampup)
    return initial_lr * lr_ramp


def noise_schedule(steps, latent_std, noise, noise_ramp):
    """sigma_i for i in range(steps) as float32, with the driver's roundings (:156): `latent_std` is a 0-d float32 TENSOR there, so
    `latent_std * args.noise` rounds to float32, the multiplication by the python-float ramp factor rounds to float32 again, and
    `.item()` hands that value to latent_noise (:157, :71-73), where `noise * strength` multiplies a float32 tensor by it."""
    base = np.float32(latent_std) * np.float32(noise)                                   # float32 x float32 -> float32, like the tensor op
    return np.array([base * np.float32(max(0, 1 - (i / steps) / noise_ramp) ** 2) for i in range(steps)], dtype=np.float32)


def latent_stats(G, n_mean_latent=10000, device="cuda", generator=None):
    """latent_mean [k,D] and latent_std scalar from N(0,I) samples (:251-255)."""
    samples = torch.randn(n_mean_latent, *G.input_shape[1:], device=device, generator=generator)
    mean = samples.mean(0)
    std = ((samples - mean).pow(2).sum() / n_mean_latent) ** 0.5
    return mean, std


def _as_latent(latent_mean, shape):
    """latent_mean as a tensor of `shape` = (k, D) or (k, num_ws, D): a [k, D] mean is broadcast over the layer slots of a W+ latent."""
    t = latent_mean.detach().clone().float()
    if len(shape) == 3 and t.numel() == shape[0] * shape[2]:
        t = t.reshape(shape[0], 1, shape[2]).expand(*shape)
    return t.reshape(*shape).contiguous()


def _wing_into(kind, out, table, target, n, ctr):
    """out[n] (float64) = WingLoss(10, 2) ("wing") or AdaptiveWingLoss(14, 0.5, 1, 2.1) ("awing") of the landmark rows ctr .. ctr + n - 1 of
    `table` against `target`; rows past the table's end read its last row."""
    L, st = _lib.lib(), _lib.stream_ptr()
    if kind == "wing":
        _lib.check(L.mgf_wing_loss_f64(out.data_ptr(), table.data_ptr(), target.data_ptr(), n, target.numel(), 10.0, 2.0, ctr.data_ptr(),
                                       table.shape[0] - 1, st), "wing_loss")
    else:
        _lib.check(L.mgf_adaptive_wing_loss_f64(out.data_ptr(), table.data_ptr(), target.data_ptr(), n, target.numel(), 14.0, 0.5, 1.0, 2.1,
                                                ctr.data_ptr(), table.shape[0] - 1, st), "adaptive_wing_loss")


def mapping_only(G, z):
    """w [n, k, D] = the mapping network on z [n, k, D] for ANY n, without touching the generator's synthesis workspaces: the kernel
    writes into a buffer of its own (G.mapping / G._mapping_into size the whole synthesis workspace for the batch -- 1.6 GB per sample at
    1024^2 -- which a statistics pass over 10 000 samples must never do)."""
    _lib.require_gpu(z)
    cfg = G.cfg
    assert tuple(z.shape[1:]) == (cfg.k, cfg.z_dim), tuple(z.shape)
    z = z.contiguous().float()
    w = torch.empty(z.shape[0], cfg.k, cfg.w_dim, dtype=torch.float32, device=z.device)
    _lib.check(_lib.lib().mgf_mapping_forward(w.data_ptr(), z.data_ptr(), G.plan.mapping_blob.data_ptr(), z.shape[0], cfg.k, cfg.w_dim,
                                              cfg.mapping_layers // 2, int(cfg.normalize_global), _lib.stream_ptr()), "mapping_forward")
    return w


def latent_stats_w(G, n_mean_latent=10000, device="cuda", generator=None):
    """Statistics of the INTERMEDIATE latent for a W+ search (what StyleGAN2-style projectors use: w_avg and w_std of mapped samples):
    mean [k, D] and the scalar std of G.mapping(z)[:, :, 0] over z ~ N(0, I), with the drivers' formula (:251-255) applied to w."""
    z = torch.randn(n_mean_latent, *G.input_shape[1:], device=device, generator=generator)
    w = mapping_only(G, z)
    mean = w.mean(0)
    std = ((w - mean).pow(2).sum() / n_mean_latent) ** 0.5
    return mean, std


def seeded_generator(device, seed):
    """A generator of its own on `device`, seeded with `seed`; None (torch's global stream) without a seed."""
    return None if seed is None else torch.Generator(device=device).manual_seed(seed)


def seeded_randn(shape, device, seed):
    """N(0, 1) float32 of `shape` on `device`, the head of the stream `seed` keys."""
    return torch.randn(*shape, device=device, generator=seeded_generator(device, seed))


def seeded_latent_stats(G, args, latent_space="z", seed=None):
    """(latent_mean, latent_std) of the latent space a projection searches ("z": latent_stats, "w+": latent_stats_w) from
    args.n_mean_latent samples of the stream `seed` keys (None: torch's global stream)."""
    stats = latent_stats_w if latent_space == "w+" else latent_stats
    return stats(G, args.n_mean_latent, G.device, generator=seeded_generator(G.device, seed))


class ProjectionEngine:
    """One target image <-> one latent search, replayable as a hipGraph."""
    _lockstep = False           # several targets per engine: GradientProjectionEngine only
    graph_debug = False         # True (set from outside before the first run()): captures keep their hipGraph_t, so that its nodes can be counted (bench.py)

    def __init__(self, G, target, latent_mean, latent_std, args: ProjectionArgs = None, percept=None, use_mse=True,
                 lm_target=None, lm_steps=None, lm_valid=None, eps=None, noise_mode="random", seed=0, use_graph=True, batch=1,
                 landmark_fn=None, biometric=None, gamma=1.0, wing_kind="wing", landmark_model=None, pipeline=False, keep_images=0,
                 latent_shape=None, landmark_input="float", lbp_target=None, mdf=None, region_weight=None, face_crop=None,
                 face_crop_target=None, face_crop_target_b=None, face_crop_filter="area"):
        """batch = number of consecutive loop steps evaluated per generator forward.  In literal mode the steps do not depend
        on each other (latent_in never changes), so evaluating `batch` candidates at once and examining them in step order
        gives exactly the sequential loop's result while the small 4x4..64x64 layers, the mapping network and the LPIPS tail
        get `batch` times more parallel work per launch.

        wing_kind: "wing" (WingLoss(10, 2), the default drivers) or "awing" (AdaptiveWingLoss(14, 0.5, 1, 2.1) on the same landmark
        tensors, 1024_example_wing_loss_adaptive.py:176 with lamda = 1e-5).

        pipeline: software-pipeline consecutive batches over two streams -- while the losses and the selection of batch i run
        on a side stream, the generator already synthesises batch i+1 (its own latent / image buffers and step counter).  The
        literal loop's steps are independent, and selection still happens in step order, so results are unchanged; one extra
        generator batch is in flight at any time, and the run's last launch sequence scores its batch with nothing beside it (the
        first generator batch and the last loss phase are the two un-overlapped ends: B generator forwards for B scored batches).

        keep_images: K > 0 keeps the SCORED image of every improvement on the device (the drivers write `{step:06d}_{loss:04f}.png`
        of exactly that image -- random per-layer noise included -- at every improvement, :186-195): a trail of up to K images with
        their steps and losses, filled inside the launch sequence (no host round trip); after K improvements the last slot is
        overwritten, so the best-so-far image is always there.  `improvements()` returns the trail, `save_improvements()` writes it
        under the reference's file names.

        biometric: optional `iresnet.BiometricLoss`; adds gamma * MSE(embed(img), embed(target)) to the objective (the
        FaceNet term of 1024_example_FaceNet_percept.py:147-158 on the vendored IResNet embedder).

        mdf: optional `mdf.MDFLoss`; adds its per-candidate loss to the p_loss slot after LPIPS and the biometric term -- the whole
        objective of the MDF drivers (1024_example_mdfloss.py:165, p_loss = criterion(imgs, img_gen), with use_mse=False and
        min_loss_init 1000; on the pooled image when pool_above is set, projection_example_v1_mdfloss.py:153-157).

        landmark_model: optional DEVICE callable `m(img [B,3,H,W]) -> (landmarks [B,68,2] float64, valid [B] int32)` -- the GPU
        landmark-regressor interface of SURVEY.md 8f row 3.  It runs inside the launch sequence (graph-capturable if the model
        is), so the loop keeps its no-host-round-trip property; results are scattered into the landmark table on the device.

        landmark_fn: optional host callback `f(img_hwc float32 numpy [H,W,3]) -> [68,2] array or None` standing where the
        drivers call dlib on every generated image (:159-170; `drivers.reference_gray_u8` reproduces their cv2 normalise +
        gray conversion).  With it the landmark table is filled step by step (None = "no face", the step is skipped) at
        the price of one device->host image copy and a host call per candidate, and graph replay is off.

        landmark_input: what `landmark_fn` is handed.  "float": the float32 [H,W,3] image (12.6 MB per candidate at 1024^2 crosses to the
        host, the caller converts it itself).  "gray_u8": the uint8 [H,W] gray image the drivers build for dlib (:159-163, cv2.normalize +
        BGR2GRAY on RGB data), made ON THE DEVICE (mgf_reference_gray_u8, bit-identical to drivers.reference_gray_u8) and copied into
        pinned host memory -- 1 MB per candidate -- and the launch sequence stays two captured hipGraphs with the host detour between
        them: {perturb, generator, gray image, device->host copy} | callbacks, one host->device copy of the landmark rows | {losses,
        selection}.

        region_weight: a map W [H,W] (or [1,1,H,W]) >= 0 with a positive sum, at the size the image-space losses see (the pooled size with
        pool_above): the LPIPS term becomes sum_l sum_p omega_l[p] m_l[p] (PerceptualLoss.set_region_weight) and the pixel term
        sum_c sum_p W[p] (x - t)^2 / (C sum W) (mgf_mse_weighted_f32).  A constant W is today's objective.  Wing, biometric and MDF terms
        ignore it; the DSSIM / MS-SSIM / PSNR / LBP pixel terms and latent_copies > 1 refuse it.

        face_crop: the biometric term embeds through the aligned face crop (BiometricLoss.set_crop; an ArcFace embedder) -- the [2,3] matrix of
        the candidates, crop pixel index -> pixel index of the image the losses see (the pooled one under pool_above: drivers.scale_crop);
        noise_mode: the generator's per-layer noise.  "random" (the drivers'): fresh draws in launch order, so a result depends on the batch
        size, eager or replayed, pipelined or not.  "keyed": the maps of step i are a function of (seed, i) alone (Generator._draw_noise_keyed;
        the key is `seed`, held in the device tensor `noise_key`, which retarget(seed=...) rewrites in place) -- every launch form of one batch
        size gives the same bits, a rewound or re-targeted engine repeats its run, and drivers.render_latent(noise_mode="keyed",
        noise_key=seed, noise_step=best step) re-renders the image that was scored.

        face_crop_target / face_crop_target_b: the matrices of the target image(s), face_crop by default; face_crop_filter "area" or
        "bilinear".  The engine only hands them to `biometric.set_crop` ahead of its set_target calls; without face_crop it never touches the
        crop, and one set on the BiometricLoss by hand stays."""
        self.G, self.args = G, args or ProjectionArgs()
        self.batch = int(batch)
        assert self.batch >= 1
        a = self.args
        dev = G.device
        self.device = dev
        _lib.require_gpu(target, latent_mean)
        self.steps = a.step
        self.target = target.detach().float().clone(memory_format=torch.contiguous_format)     # the engine's OWN copy: retarget() rewrites it in place
        nt = int(self.target.shape[0])
        assert nt == 1 or self._lockstep, "one target per engine (the drivers process images serially)"
        self.percept = percept
        self.use_lbp = a.pixel_term == "lbp"
        self.use_mse = use_mse and not self.use_lbp
        self.use_wing = lm_target is not None
        if self.use_lbp and (lbp_target is None or self.use_wing or percept is not None or biometric is not None or mdf is not None):
            raise _lib.MgfError("projection: pixel_term='lbp' is the whole objective of 1024_example_LBP_percept.py -- pass lbp_target "
                                "(lbp.target_feature of the target file) and no landmark / LPIPS / biometric term")
        self.noise_mode = noise_mode
        self.noise_key = None                       # noise_mode="keyed": the key on the device (_init_state)
        k, D = G.cfg.k, G.cfg.z_dim
        # (k, D): the drivers' z latent.  GradientProjectionEngine(latent_space="w+") passes (k, num_ws, D)
        self.latent_shape = ls = tuple(latent_shape) if latent_shape is not None else (k, D)
        self.numel = int(np.prod(ls))
        self.copies = int(a.latent_copies)
        if not 1 <= self.copies <= 255:
            raise ValueError(f"latent_copies must be 1 .. 255 (got {a.latent_copies})")
        if self.copies > 1 and self.numel % 32:
            # (torch reduces a width's last numel % 32 columns on another path with another summation order: the bit-exact mean is only
            # claimed for widths it reduces four vector registers at a time -- k D = 17 x 32 = 544 is one)
            raise ValueError(f"latent_copies > 1 needs a latent of a multiple of 32 elements (got {self.numel})")
        assert wing_kind in ("wing", "awing")
        self.wing_kind = wing_kind
        self.landmark_fn = landmark_fn
        self.landmark_model = landmark_model
        if landmark_model is not None:
            assert lm_target is not None and landmark_fn is None, "landmark_model needs lm_target and excludes landmark_fn"
            # + batch spare rows: the candidates of a ragged last batch that lie past the final step land there, not on real rows
            lm_steps = np.zeros((a.step + self.batch,) + tuple(np.shape(lm_target)), np.float64)
            lm_valid = np.zeros(a.step + self.batch, np.int32)
        assert landmark_input in ("float", "gray_u8"), landmark_input
        self.landmark_input = landmark_input
        self.callback_graphs = landmark_fn is not None and landmark_input == "gray_u8"
        if landmark_fn is not None:
            assert lm_target is not None, "landmark_fn needs the target image's landmarks (lm_target)"
            spare = self.batch if self.callback_graphs else 0          # (a ragged last batch's surplus candidates land on spare rows)
            lm_steps = np.zeros((a.step + spare,) + tuple(np.shape(lm_target)), np.float64)
            lm_valid = np.zeros(a.step + spare, np.int32)
            if not self.callback_graphs:
                use_graph = False
        self._table = []                            # the loop state: (tensor, reset value) in registration order, see _reg
        self._init_state(nt, latent_mean, latent_std, eps, seed, lm_target, lm_steps, lm_valid)
        B = nt * self.batch                         # images per generator call
        self._arange = torch.arange(B, dtype=torch.int64, device=dev)
        self._init_pool(B)
        self.pixel = PixelTerm(a, self.use_mse, self.target.shape, B, dev, region_weight is not None, G.cfg.img_resolution)
        self.biometric, self.gamma, self.mdf = biometric, float(gamma), mdf
        self.face_crop_filter = face_crop_filter if face_crop is not None else None
        if face_crop is not None and biometric is None:
            raise ValueError("face_crop is the crop of the biometric term: pass biometric= with it")
        if face_crop is None and (face_crop_target is not None or face_crop_target_b is not None):
            raise ValueError("face_crop_target / face_crop_target_b need face_crop (the candidates' matrix)")
        if region_weight is None and percept is not None and hasattr(percept, "set_region_weight"):
            percept.set_region_weight(None)
        self._set_targets(None, lbp_target, region_weight, face_crop, face_crop_target, face_crop_target_b)
        # the p_loss slot takes LPIPS, the biometric term and MDF in that order: a term accumulates where one in front of it has written
        self.bio_accumulate = percept is not None
        self.mdf_accumulate = percept is not None or biometric is not None
        self.has_p = self.mdf_accumulate or mdf is not None                     # the slot is live
        self.keep_images = int(keep_images)
        self.trail = None                           # the improvement trail (keep_images > 0): select_best fills its slot, _loss_phase its images
        if self.keep_images > 0:
            self.trail = ImprovementTrail(self.keep_images, B, (G.cfg.img_channels, G.cfg.img_resolution), dev)
            self._table += self.trail.state()
        self.use_graph = use_graph
        self.graph = None
        if self.callback_graphs:
            c, r = G.cfg.img_channels, G.cfg.img_resolution
            assert c == 3, "the gray conversion is defined on 3-channel images"
            lshape = tuple(self.lm_target.shape)
            self.gray_dev = torch.empty(B, r, r, dtype=torch.uint8, device=dev)
            self.gray_host = torch.empty(B, r, r, dtype=torch.uint8).pin_memory()
            self.gray_scratch = torch.empty(B * int(_lib.lib().mgf_reference_gray_scratch_floats()), dtype=torch.float32, device=dev)
            self.lm_stage_host = torch.zeros(B, *lshape, dtype=torch.float64).pin_memory()
            self.ok_stage_host = torch.zeros(B, dtype=torch.int32).pin_memory()
            self.lm_stage = torch.zeros(B, *lshape, dtype=torch.float64, device=dev)
            self.ok_stage = torch.zeros(B, dtype=torch.int32, device=dev)
            self.cb_graphs = None
            self._host_step = 0                     # host mirror of step_ctr (the callbacks need the step numbers without a device read)
        self.pipeline = bool(pipeline) and landmark_fn is None
        if self.pipeline:
            if (G.n, G.lean) != (B, True):
                G._alloc(B, True)
            self.latent_ns = [self.latent_n, torch.empty_like(self.latent_n)]
            self.imgs = [G.img, torch.empty_like(G.img)]
            self.gen_ctr = self._reg(torch.zeros(1, dtype=torch.int32, device=dev), 0)   # step counter of the generator side
            self.loss_stream = torch.cuda.Stream(device=dev)
            self.graphs = [None, None]
            self.prime_graph = None
            self.tail_graphs = [None, None]                                       # losses only: the run's LAST launch sequence has no next batch to synthesise
            self._parity = 0
            self._primed = False
            self._seq_launched = 0                                                # host count of launch sequences since the last rewind

    def _init_state(self, nt, latent_mean, latent_std, eps, seed, lm_target, lm_steps, lm_valid):
        """What is shaped by the number of targets: start latent, noise stream and schedule, landmark tables, loop state, the three loss slots.
        nt = 1 is the drivers' loop, `batch` candidates per call; nt > 1 are GradientProjectionEngine's lockstep projections (batch 1), a row per
        target of everything: lm_target [nt,68,2], lm_steps [nt,steps,68,2], lm_valid [nt,steps], eps [steps,nt,*latent], losses [nt,steps]."""
        a, dev, ls = self.args, self.device, self.latent_shape
        start = latent_mean.detach().float()
        if nt > 1 and start.numel() == nt * self.numel:                     # one start latent per target
            self.latent_in = start.reshape(nt, *ls).contiguous().clone()
        else:
            self.latent_in = _as_latent(latent_mean, ls).reshape(1, *ls).expand(nt, *ls).contiguous()
        self.sigma = torch.as_tensor(noise_schedule(a.step, float(latent_std), a.noise, a.noise_ramp), device=dev)
        copies = (self.copies,) if self.copies > 1 else ()
        if eps is None:
            eps = seeded_randn((a.step, nt, *copies, *ls), dev, seed)
        self.eps = eps.to(dev).contiguous().float()
        assert self.eps.shape[0] >= a.step and (self.eps[0].numel() == self.numel * self.copies if nt == 1
                                                else tuple(self.eps.shape[1:]) == (nt, *ls)), \
            f"eps must be [steps, {nt}{', copies' if copies else ''}, *latent shape] (got {tuple(self.eps.shape)})"
        self.lm_tables = None
        if self.use_wing:
            self.lm_target = torch.as_tensor(lm_target, dtype=torch.float64, device=dev).contiguous()
            self.lm_steps = torch.as_tensor(lm_steps, dtype=torch.float64, device=dev).contiguous()
            if nt == 1:
                assert self.lm_steps.shape[0] >= a.step and self.lm_steps.shape[1:] == self.lm_target.shape
                self.lm_tables = [self.lm_steps]
            else:
                assert self.lm_target.shape[0] == nt and self.lm_steps.shape[0] == nt and self.lm_steps.shape[1] >= a.step
                self.lm_tables = [self.lm_steps[j] for j in range(nt)]
        self.valid = None if lm_valid is None else torch.as_tensor(lm_valid, dtype=torch.int32, device=dev).contiguous()
        if nt > 1 and self.valid is not None:
            self.valid = self.valid.reshape(nt, -1)
        if self.noise_mode == "keyed":              # what the keyed launches read next to the step counter; not rewound: a rewound run repeats
            self.noise_key = self._reg(torch.zeros(1, dtype=torch.int64, device=dev))
            self._set_noise_key(seed)
        # device-resident loop state, one row per target (select_best advances a target's own counter)
        self.step_ctr = self._reg(torch.zeros(nt, dtype=torch.int32, device=dev), 0)
        self.min_loss = self._reg(torch.full([nt], float(a.min_loss_init), dtype=torch.float64, device=dev), float(a.min_loss_init))
        self.best_latent = self._reg(torch.zeros(nt, *ls, dtype=torch.float32, device=dev), 0)
        self.best_step = self._reg(torch.full([nt], -1, dtype=torch.int32, device=dev), -1)
        self.losses = self._reg(torch.full([a.step] if nt == 1 else [nt, a.step], float("nan"), dtype=torch.float64, device=dev), float("nan"))
        n = nt * self.batch
        self.latent_n = torch.empty(n, *ls, dtype=torch.float32, device=dev)
        self.p_loss = torch.zeros(n, dtype=torch.float32, device=dev)
        self.mse_loss = torch.zeros(n, dtype=torch.float32, device=dev)
        self.w_loss = torch.zeros(n, dtype=torch.float64, device=dev)

    def _set_noise_key(self, seed):
        """The 64 key bits of `seed` into the device tensor the captured keyed launches read (in place)."""
        v = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.noise_key.fill_(v - ((v >> 63) << 64))

    def _noise_kw(self, ctr):
        """The generator's noise keywords of one forward whose sample j is step ctr + j: in keyed mode the counter and the clamp that
        mgf_latent_perturb reads, so candidate j of a batch draws the maps of ITS step whatever batch it is scored in."""
        if self.noise_mode != "keyed":
            return dict(noise_mode=self.noise_mode)
        return dict(noise_mode="keyed", noise_key=self.noise_key, noise_step=ctr, noise_step_add=1, noise_step_max=self.steps - 1)

    def _reg(self, tensor, reset=None):
        """Register a loop-state tensor where it is allocated, and return it.  Every registered tensor is saved and restored around a graph
        capture (_state); `reset` is the value it was allocated with, which rewind() gives it again; None: rewind() leaves it where the run left
        it (the start latent, the Adam moments, the noise maps and theirs)."""
        self._table.append((tensor, reset))
        return tensor

    def _set_targets(self, target, lbp_target, region_weight, face_crop, face_crop_target, face_crop_target_b=None):
        """Hand the target (and what comes with one: region weight, LBP code map, crop matrices) to every term, in place in the buffers the
        launch sequence reads -- captured graphs reference them.  The constructor (target None: self.target is the new copy) and retarget();
        a weight / crop of None stays as it is."""
        if region_weight is not None:
            w = self.pixel.set_region_weight(region_weight)
            if self.percept is not None:
                self.percept.set_region_weight(w[:, None])
        if target is not None:
            self.target.copy_(target)
        self.pixel.refresh_target(self.target, lbp_target)
        if self.percept is not None:
            self.percept.set_target(self.target)                  # same shapes on a retarget: rewrites the cached taps in place
        if face_crop is not None:
            self.biometric.forget_target()        # (another engine's or the last target's: set_target follows, one embedder pass, not two)
            self.biometric.set_crop(face_crop, face_crop_target, face_crop_target_b, filter=self.face_crop_filter)
        if self.biometric is not None:
            self.biometric.set_target(self.target)
        if self.mdf is not None:
            self.mdf.set_target(self.target)

    def _init_pool(self, B):
        """projection_example_v1.py:150-155: images above `pool_above` pixels are block-averaged by height // pool_above in front of the
        image-space losses; the target comes at the pooled size."""
        a, G = self.args, self.G
        r = G.cfg.img_resolution
        self.pool_factor = a.pool_factor(r)
        want = r // self.pool_factor
        if tuple(self.target.shape[-2:]) != (want, want):
            raise _lib.MgfError(f"projection: the target is {tuple(self.target.shape[-2:])}, the image-space losses see {want}x{want} "
                                f"(generator {r}x{r}, pool_above={a.pool_above})")
        if self.pool_factor > 1:
            f = self.pool_factor
            # the block mean as the library's own upfirdn2d: an f x f box filter of weight 1 / f^2, down-sampling by f, no padding
            self.pool_box = torch.full([f, f], 1.0 / (f * f), dtype=torch.float32, device=self.device)
            self.pooled = torch.empty(B, G.cfg.img_channels, want, want, dtype=torch.float32, device=self.device)

    def _pooled(self, img):
        if self.pool_factor == 1:
            return img
        from . import conv as cv
        return cv.upfirdn_into(self.pooled[:img.shape[0]], img, self.pool_box, up=1, down=self.pool_factor, pad=(0, 0, 0, 0), gain=1.0)

    # ------------------------------------------------------------------ one iteration
    def _iteration(self):
        """`batch` consecutive steps of the loop: perturb -> generator -> losses -> in-order best-so-far selection."""
        img = self._gen_phase(self.latent_n, self.step_ctr)
        self._loss_phase(img, self.latent_n)
        return img

    def _gen_phase(self, latent_n, ctr):
        L, st, a, B = _lib.lib(), _lib.stream_ptr(), self.args, self.batch
        if self.copies > 1:       # the v2 driver's averaged copies (projection_example_v2_percept.py:147-159)
            _lib.check(L.mgf_latent_perturb_mean(latent_n.data_ptr(), self.latent_in.data_ptr(), self.eps.data_ptr(), self.sigma.data_ptr(),
                                                 ctr.data_ptr(), B, self.steps, self.numel, self.copies, st), "latent_perturb_mean")
        else:
            _lib.check(L.mgf_latent_perturb(latent_n.data_ptr(), self.latent_in.data_ptr(), self.eps.data_ptr(),
                                            self.sigma.data_ptr(), ctr.data_ptr(), B, self.steps, self.numel, st), "latent_perturb")
        # psi lands in `c`.  lean: the literal loop has no backward pass -- layer outputs share arenas block after block
        return self.G.forward_workspace(latent_n, a.truncation_psi, lean=True, **self._noise_kw(ctr))[0]

    def _loss_phase(self, img, latent_n):
        L, st, a, B = _lib.lib(), _lib.stream_ptr(), self.args, self.batch
        full_img, img = img, self._pooled(img)              # (the improvement trail keeps the image as generated)
        if self.percept is not None:
            self.percept.distance_into(self.p_loss, img)
            if a.percept_weight != 1.0:
                self.p_loss.mul_(float(a.percept_weight))
        if self.biometric is not None:      # rides in the p_loss slot: p_loss = LPIPS + gamma * embedding MSE
            self.biometric.distance_into(self.p_loss, img, scale=self.gamma, accumulate=self.bio_accumulate)
        if self.mdf is not None:            # p_loss (+)= MDF (1024_example_mdfloss.py:165)
            self.mdf.distance_into(self.p_loss, img, accumulate=self.mdf_accumulate)
        self.pixel.value_into(self.mse_loss, img, self.target, B, 0)           # the B candidates share the one target
        self._landmarks(full_img)
        if self.use_lbp:        # rides in the float64 slot, coefficient 1
            self.pixel.lbp_into(self.w_loss, full_img)
        if self.use_wing:
            _wing_into(self.wing_kind, self.w_loss, self.lm_steps, self.lm_target, B, self.step_ctr)
        self._select_best(latent_n, B, self.trail, valid=self.valid)
        if self.trail is not None:
            _lib.check(L.mgf_keep_improvements(self.trail.imgs.data_ptr(), full_img.data_ptr(), self.trail.imgs.shape[1],
                                               self.trail.take.data_ptr(), B, st), "keep_improvements")

    def _select_best(self, latent_n, n, slot, row=0, valid=None, has_p=None, numel=None, loss_slots=None):
        """The in-order best-so-far selection over the `n` candidates `latent_n` of target `row`: that target's rows of the loop state and of
        the three loss slots (a slot that no term writes goes in as null), its `valid` table, and `slot`, the ImprovementSlot that learns
        which candidates improved (None: nobody asks).  The one place that spells mgf_select_best's argument list.  numel: the floats of one
        candidate where that is not one latent (the de-morphing engine's parameter pair); loss_slots: its (p, w, mse) slots in place of row
        `row` of the engine's."""
        a, j = self.args, row
        has_p = self.has_p if has_p is None else has_p
        take, count, slots, steps, losses = (None, None, 0, None, None) if slot is None else (slot.take, slot.count, slot.slots, slot.steps, slot.losses)
        p_loss, w_loss, mse_loss = (self.p_loss[j:], self.w_loss[j:], self.mse_loss[j:]) if loss_slots is None else loss_slots
        _lib.check(_lib.lib().mgf_select_best(
            self.min_loss[j:].data_ptr(), self.best_latent[j:].data_ptr(), self.best_step[j:].data_ptr(),
            self.losses.reshape(self.min_loss.numel(), -1)[j].data_ptr(), latent_n.data_ptr(), self.numel if numel is None else int(numel),
            _lib.ptr(p_loss if has_p else None), _lib.ptr(w_loss if (self.use_wing or self.use_lbp) else None),
            _lib.ptr(mse_loss if self.use_mse else None), 1.0 if self.use_lbp else float(a.lamda), float(a.beta),
            self.step_ctr[j:].data_ptr(), _lib.ptr(valid), n, self.steps, _lib.ptr(take), _lib.ptr(count), slots, _lib.ptr(steps), _lib.ptr(losses),
            _lib.stream_ptr()), "select_best")

    def _landmarks(self, img):
        """Fill this batch's rows of the landmark / valid tables when a detector is attached (host callback or device model)."""
        B = self.batch
        if self.landmark_fn is not None and self.callback_graphs:
            # the callbacks ran on the host between the two launch sequences (_cb_sequence); their rows wait in the device staging buffers
            self._scatter_rows(self.lm_stage, self.ok_stage)
        elif self.landmark_fn is not None:
            s0 = int(self.step_ctr.item())                                     # host sync (the reference syncs three times per step)
            host = img.permute(0, 2, 3, 1).contiguous().cpu().numpy()         # [B,H,W,3] float32, what the drivers build at :159-161
            self._detect(host, s0, self.lm_steps[s0:], self.valid[s0:])
        if self.landmark_model is not None:
            lm, ok = self.landmark_model(img)
            self._scatter_rows(lm.to(torch.float64).reshape(B, *self.lm_target.shape), ok.to(torch.int32).reshape(B))

    def _scatter_rows(self, lm, ok):
        """This batch's landmark rows and valid flags, device tensors, into the rows of its steps of the tables (a ragged last batch's surplus
        lands on the spare rows)."""
        idx = self.step_ctr.long() + self._arange
        self.lm_steps.index_copy_(0, idx, lm)
        self.valid.index_copy_(0, idx, ok)

    def _detect(self, images, s0, lm_rows, ok_rows):
        """The host detector on every candidate of the batch that starts at step s0, in step order (`images[j]`: what landmark_input names):
        row j of lm_rows / ok_rows takes candidate j's landmarks and a 1; None = "no face", the rows stay and the step is skipped (:165-166)."""
        for j in range(min(self.batch, self.steps - s0)):
            lm = self.landmark_fn(images[j])
            if lm is None:
                continue
            lm_rows[j].copy_(torch.as_tensor(np.asarray(lm, dtype=np.float64).reshape(self.lm_target.shape)))
            ok_rows[j] = 1

    # ------------------------------------------------------------------ pipelined mode
    def _pipe_gen(self, p):
        """Generator side of batch parity p (own latent / image buffer, own step counter)."""
        self.G.img = self.imgs[p]
        img = self._gen_phase(self.latent_ns[p], self.gen_ctr)
        self.gen_ctr.add_(self.batch).clamp_(max=self.steps)
        return img

    def _pipe_step(self, p):
        """Steady state: losses + selection of the batch in buffers p on the loss stream, the generator of the next batch in buffers
        p ^ 1 on the current stream; joined at the end."""
        main = torch.cuda.current_stream(self.device)
        self.loss_stream.wait_stream(main)
        with torch.cuda.stream(self.loss_stream):
            self._loss_phase(self.imgs[p], self.latent_ns[p])
        self._pipe_gen(p ^ 1)
        main.wait_stream(self.loss_stream)

    def _pipe_tail(self, p):
        """The run's last launch sequence: losses + selection of the batch in buffers p, nothing left to synthesise beside them."""
        self._loss_phase(self.imgs[p], self.latent_ns[p])

    def _pipe_sequence(self):
        """The pipelined mode's "launch one sequence" (run()): captures on first use, primes the pipeline, and picks steady state or tail."""
        if self.use_graph and self.graphs[0] is None:                     # (the warm-up overwrites both image buffers: capture before priming)
            step, tail = [partial(self._pipe_step, p) for p in (0, 1)], [partial(self._pipe_tail, p) for p in (0, 1)]
            # a tail shares its steady-state graph's pool; the first batch of a run (nothing to score beside it yet) is a graph of its own in
            # the pool of graphs[0]: a re-targeted engine starts every run with it
            g = self._capture_graphs(step, [(step[0], None), (tail[0], 0), (step[1], None), (tail[1], 2), (partial(self._pipe_gen, 0), 0)])
            self.graphs, self.tail_graphs, self.prime_graph = [g[0], g[2]], [g[1], g[3]], g[4]
        if not self._primed:
            if self.use_graph and self._parity == 0:
                self.prime_graph.replay()                                 # the first batch has no losses to overlap with
            else:
                self._pipe_gen(self._parity)
            self._primed = True
        last = -(-self.steps // self.batch) - 1                          # index of the sequence that scores the run's last candidates

        def launch():
            final = self._seq_launched >= last                            # (and anything a caller launches past the end: nothing left to score)
            if self.use_graph:
                (self.tail_graphs if final else self.graphs)[self._parity].replay()
            else:
                (self._pipe_tail if final else self._pipe_step)(self._parity)
            self._parity ^= 1
            self._seq_launched += 1
        return launch

    # ------------------------------------------------------------------ callback mode on the gray uint8 image
    def _cb_phase_a(self):
        """perturb -> generator -> the drivers' gray uint8 image of every candidate -> pinned host memory (all asynchronous)."""
        img = self._gen_phase(self.latent_n, self.step_ctr)
        n, _, h, w = img.shape
        _lib.check(_lib.lib().mgf_reference_gray_u8(self.gray_dev.data_ptr(), img.data_ptr(), n, h, w, self.gray_scratch.data_ptr(),
                                                    _lib.stream_ptr()), "reference_gray_u8")
        self.gray_host.copy_(self.gray_dev, non_blocking=True)
        return img

    def _cb_phase_b(self):
        self._loss_phase(self.G.img, self.latent_n)

    def _cb_sequence(self):
        """The callback mode's "launch one sequence" (run()): phase A, one stream synchronisation, the host detector on every candidate's gray
        image, ONE host->device copy of the batch's landmark rows, phase B."""
        a, b = self._cb_phase_a, self._cb_phase_b
        if self.use_graph and self.cb_graphs is None:
            self.cb_graphs = tuple(self._capture_graphs([a, b], [(a, None), (b, 0)]))
            if self.use_wing:                       # the warm-up scattered staging rows no detector has filled
                self.lm_steps.zero_()
                self.valid.zero_()
        if self.cb_graphs is not None:
            a, b = self.cb_graphs[0].replay, self.cb_graphs[1].replay
        st = torch.cuda.current_stream(self.device)

        def launch():
            a()
            st.synchronize()
            s0 = self._host_step
            self.ok_stage_host.zero_()
            self._detect(self.gray_host.numpy(), s0, self.lm_stage_host, self.ok_stage_host)
            self.lm_stage.copy_(self.lm_stage_host, non_blocking=True)
            self.ok_stage.copy_(self.ok_stage_host, non_blocking=True)
            b()
            self._host_step = min(s0 + self.batch, self.steps)
        return launch

    def _state(self):
        """Device tensors that make up the loop state (saved and restored around the capture warm-up): every registered one, see _reg."""
        return tuple(t for t, _ in self._table)

    def improvements(self):
        """The improvement trail of a keep_images=K engine: list of (step, loss, image [C,H,W]) in the order the improvements
        happened -- the (step, min_loss, img_gen_raw) triples the drivers turn into PNG files (:186-195).  Images still resident in the
        device trail are device tensors, those already spilled to the host (ImprovementTrail.spill) CPU tensors.  With keep_images >= batch
        the list is complete; otherwise a launch sequence with more than K improvements kept its first K-1 and its latest (a warning
        says how many images were lost)."""
        assert self.trail is not None, "construct the engine with keep_images=K"
        return self.trail.listing()

    def save_improvements(self, output_dir, ratio=1.0):
        """Write the trail as the drivers do: `{output_dir}/{step:06d}_{loss:04f}.png` of crop(to_pil(img), ratio) (:190-195)."""
        from .drivers import save_image
        paths = []
        for step, loss, img in self.improvements():
            paths.append(save_image(self.G, img.unsqueeze(0).to(self.device), os.path.join(output_dir, "{:06d}_{:04f}.png".format(step, loss)), ratio))
        return paths

    def _capture_graphs(self, warmup, bodies):
        """THE capture protocol of every launch mode.  warmup: bodies run once each, eagerly, in order, on a side stream (allocations, lazy
        init; they advance the loop for real, and noise_mode="random" draws its per-layer noise in launch order: their number and order are part
        of a mode's result there -- unchanged -- while noise_mode="keyed" draws by (key, step) and does not depend on them).  bodies: [(body, index into this list of the graph whose memory pool it shares, or None)], captured in order.  The loop state
        -- every registered tensor -- is saved in front and put back afterwards, and the generator's workspace is pinned.  Returns the graphs."""
        state = [t.clone() for t in self._state()]
        main, s = torch.cuda.current_stream(self.device), torch.cuda.Stream(device=self.device)
        s.wait_stream(main)
        with torch.cuda.stream(s):
            for body in warmup:
                body()
        main.wait_stream(s)
        torch.cuda.synchronize(self.device)
        keep = bool(self.graph_debug)       # keep the hipGraph_t behind the executable graph, so that its nodes can be counted afterwards
        graphs = []
        for body, share in bodies:
            g = torch.cuda.CUDAGraph(keep_graph=True) if keep else torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=None if share is None else graphs[share].pool()):
                body()
            if keep:
                g.instantiate()
            graphs.append(g)
        for dst, src in zip(self._state(), state):
            dst.copy_(src)
        # the captured graphs reference the generator's workspace of this batch size: keep it alive as long as this engine lives
        weakref.finalize(self, self.G.unpin, self.G.pin())
        return graphs

    def _plain_sequence(self):
        """The plain mode's "launch one sequence" (run()): the whole iteration, as one graph where graphs are on."""
        if self.use_graph and self.graph is None:
            (self.graph,) = self._capture_graphs([self._iteration], [(self._iteration, None)])
        return self.graph.replay if self.graph is not None else self._iteration

    def run(self, steps=None):
        """Advance the loop by `steps` iterations (default: all remaining), `batch` of them per launch sequence (lockstep targets advance together)."""
        done = int(self.step_ctr[0].item()) if steps is None else None
        n = (self.steps - done) if steps is None else steps
        n = (n + self.batch - 1) // self.batch
        launch = (self._pipe_sequence if self.pipeline else self._cb_sequence if self.callback_graphs else self._plain_sequence)()
        for _ in range(n):
            if self.trail is not None:
                self.trail.before_sequence()
            launch()
        return self

    def retarget(self, target, lm_target=None, lm_steps=None, lm_valid=None, eps=None, seed=None, latent_mean=None, latent_std=None,
                 lbp_target=None, region_weight=None, face_crop=None, face_crop_target=None):
        """Point this engine at ANOTHER target image and rewind the loop, keeping everything that was expensive to set up: the captured
        hipGraph(s), the generator workspace, the LPIPS / embedder workspaces, the loss scratch.  Only data changes, in place, in the
        buffers the graph already references: the target image and its cached LPIPS taps / embedding, the landmark tables, the noise
        stream (`eps` given, or redrawn from `seed`; `seed` also re-keys noise_mode="keyed"), optionally the start latent and the noise schedule, and the loop state (step
        counter, best-so-far, loss history, improvement trail).  A run after retarget() equals the run of a freshly constructed engine
        on the same inputs bit for bit (tests/test_hip_drivers.py).  This is what the reference's serial per-image loop amortises by
        keeping G / percept / latent statistics outside `projection()` (projection_example_v2_percept_morph.py:311-355); BASELINE
        configs 3 and 5 are batches of targets.  region_weight: the new target's region weight, written into the weight buffers in place (an
        engine built with a weight; without the argument the weight stays).  face_crop / face_crop_target: the new target's crop matrices (an
        engine built with face_crop; the matrix buffer the captured launches read is rewritten in place; without the argument the crop stays)."""
        a, dev = self.args, self.device
        _lib.require_gpu(target)
        assert tuple(target.shape) == tuple(self.target.shape), (tuple(target.shape), tuple(self.target.shape))
        torch.cuda.synchronize(dev)
        if face_crop is not None and self.face_crop_filter is None:
            raise _lib.MgfError("retarget: this engine was built without a face crop; build a fresh one with face_crop=")
        self._set_targets(target, lbp_target, region_weight, face_crop, face_crop_target)
        if self.use_wing:
            assert lm_target is not None, "this engine has a Wing term: pass the new target's landmarks"
            self.lm_target.copy_(torch.as_tensor(lm_target, dtype=torch.float64).reshape(self.lm_target.shape))
            if self.landmark_fn is not None or self.landmark_model is not None:
                self.lm_steps.zero_()
                self.valid.zero_()
            else:
                assert lm_steps is not None, "pass the per-step landmark table of the new target"
                t = torch.as_tensor(lm_steps, dtype=torch.float64)
                assert t.shape[0] >= a.step and tuple(t.shape[1:]) == tuple(self.lm_target.shape)
                self.lm_steps[:a.step].copy_(t[:a.step])
                if self.valid is not None:
                    self.valid.copy_(torch.ones(self.valid.shape, dtype=torch.int32) if lm_valid is None
                                     else torch.as_tensor(lm_valid, dtype=torch.int32).reshape(self.valid.shape))
                else:
                    assert lm_valid is None, "the engine was built without a `valid` table; construct it with lm_valid to use one"
        if eps is not None:
            assert eps.shape[0] >= a.step
            self.eps[:a.step].copy_(eps[:a.step].reshape(a.step, *self.eps.shape[1:]))
        elif seed is not None:
            self.eps.copy_(seeded_randn(self.eps.shape, dev, seed))                      # same draw as the constructor's
        if seed is not None and self.noise_key is not None:
            self._set_noise_key(seed)               # noise_mode="keyed": the captured launches read the key from this tensor
        if latent_mean is not None:
            self.latent_in.copy_(latent_mean.detach().reshape(self.latent_in.shape))
        if latent_std is not None:
            self.sigma.copy_(torch.as_tensor(noise_schedule(a.step, float(latent_std), a.noise, a.noise_ramp)))
        self.rewind()
        return self

    def rewind(self):
        """Loop state back to step 0 (graph, workspaces and inputs untouched): every registered tensor that has a reset value (_reg) takes
        it again; the host-side counters follow.  GradientProjectionEngine: like the latent and its Adam moments, the noise maps and theirs
        stay where the run left them; the best step's maps and the improvement flag are cleared with the best-so-far they belong to."""
        for t, value in self._table:
            if value is not None:
                t.zero_() if value == 0 else t.fill_(value)
        if self.trail is not None:
            self.trail.forget()
        if self.callback_graphs:
            self._host_step = 0
        if self.pipeline:
            self._parity, self._primed, self._seq_launched = 0, False, 0
        return self

    def result(self):
        """(best_latent [1,k,D] cpu, best_step int, best_loss float, losses [steps] float64 numpy).  Raises like the
        reference (`latent_path[-1]` on an empty list, :208) when no step ever improved on min_loss_init."""
        torch.cuda.synchronize(self.device)
        bs = int(self.best_step.item())
        if bs < 0:
            raise IndexError("projection: no iteration improved on the initial min_loss (reference: latent_path[-1] on an empty list)")
        return self.best_latent.cpu().clone(), bs, float(self.min_loss.item()), self.losses.cpu().numpy()


def save_best_png(G, latent, path, ratio=1.0, noise_mode="const", noises=None, noise_key=None, noise_step=None):
    """Write the image of `latent` as the drivers do (misc.to_pil + crop_max_rectangle, misc.py:94-130; :194-195).  noises: the per-layer
    maps to render with (GradientProjectionEngine(optimize_noise=True).best_noises: the saved PNG is then the scored image).
    noise_mode="keyed" with noise_key / noise_step (the engine's seed and the best step): the maps the best step was scored with."""
    from . import misc
    latent = latent.to(G.device)
    if noises is not None:
        noise_mode = "inject"
    keyed = dict(noise_key=noise_key, noise_step=noise_step, noise_step_add=0) if noise_mode == "keyed" else {}
    if latent.ndim == 4:                       # a W+ result [1, k, num_ws, D] (GradientProjectionEngine(latent_space="w+"))
        img = G.forward_workspace(ws=latent, noise_mode=noise_mode, noises=noises, **keyed)[0]
    else:
        img = G.forward_workspace(latent, None, noise_mode=noise_mode, noises=noises, **keyed)[0]
    im = misc.crop_max_rectangle(misc.to_pil(img), ratio)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    im.save(path)
    return path


def synthetic_landmarks(steps, res, seed):
    """Injected stand-in for the dlib detector: fixed [68,2] grid in the central half + seeded jitter."""
    rng = np.random.Generator(np.random.PCG64(seed))
    target = rng.integers(res // 4, 3 * res // 4, size=(68, 2)).astype(np.float64)
    per_step = target[None] + rng.integers(-max(res // 64, 1), max(res // 64, 1) + 1, size=(steps, 68, 2)).astype(np.float64)
    return target, per_step


def __getattr__(name):
    """`GradientProjectionEngine` lives in gradient_projection.py, which imports this module: importable from here as before, on first use."""
    if name == "GradientProjectionEngine":
        from .gradient_projection import GradientProjectionEngine
        return GradientProjectionEngine
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
