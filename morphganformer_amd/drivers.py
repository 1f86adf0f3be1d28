"""The callers on either side of the projection loop, re-stated as functions:

  image_transform   target image -> [1,3,S,S] in [-1,1]      (1024_example_wing_loss_perceptual_sqz_MSE.py:89-108)
  save_latent_mat / load_latent_mat    the `.mat` latent exchange format, key 'w'   (1024_merge_morph_2.py:73-92)
  generate_images   z ~ N(0,1) -> G(z, psi) -> PNG           (1024_generate.py:19-41)
  merge_morph       (1-a) w1 + a w2 -> G(., psi) -> JPG+.mat (1024_merge_morph_2.py:83-92; the reference hard-codes a = 0.5,
                    BASELINE config 4 sweeps 11 values)
  refine_morph      the blend descended against BOTH contributing subjects (gradient mode with a target pair; no reference script)
  demorph_latent / demorph    the other contributor of a morph from one trusted image: the closed form on two projections, and the coupled
                    descent (demorph.DemorphEngine; no reference script)
  project_image     latent statistics + one ProjectionEngine run + best-of PNG / .mat   (:135-208, :246-268)
  lpips_map / save_lpips_map    the spatial LPIPS map of an image against a target (PNetLin(spatial=True), lpips/networks_basic.py:75-76) and its
                    .npy / gray .png files
  second_stage      a projection initialised from an earlier result (edit_MSE.py pattern, BASELINE config 5)
  warp_morphs       the 0.5 / 0.5 morph warped onto the averaged landmarks (1024_warp_morphs.py:128-210; the warp itself is `warp.py`, re-exported here)

Every image is produced by the HIP generator (`engine.Generator`); there is no CPU path here.  Landmark detection (dlib) is a
closed third-party CPU dependency: landmarks are passed in by the caller (projection.synthetic_landmarks stands in offline).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib, misc
from .evolution import EvolutionProjectionEngine, recombination_weights
from .projection import (GradientProjectionEngine, ProjectionArgs, ProjectionEngine, save_best_png, seeded_generator, seeded_latent_stats,
                         seeded_randn)
from .warp import (WARP_EXTRA_POINTS, _cv_affine_inverse, _cv_bounding_rect, _cv_fill_convex_poly, _cv_line8, _pack_warp_records,      # noqa: F401
                   frame_points, gray_u8_device, warp_morph, warp_morph_u8, warp_plan)


# ----------------------------------------------------------------------------------------------------------------- image I/O
def image_transform(src, size=1024, device="cuda"):
    """Resize(size) (shorter side, bilinear, PIL semantics) -> CenterCrop(size) -> ToTensor -> Normalize(0.5, 0.5).
    `src`: path or PIL image.  Returns float32 [1,3,size,size] on `device`."""
    from PIL import Image
    im = Image.open(src) if not isinstance(src, Image.Image) else src
    im = im.convert("RGB")
    w, h = im.size
    if (w <= h and w != size) or (h < w and h != size):
        if w <= h:
            nw, nh = size, int(size * h / w)
        else:
            nw, nh = int(size * w / h), size
        im = im.resize((nw, nh), Image.BILINEAR)
        w, h = im.size
    if w < size or h < size:            # CenterCrop pads small images with zeros
        pl, pt = max((size - w) // 2, 0), max((size - h) // 2, 0)
        canvas = Image.new("RGB", (max(w, size), max(h, size)))
        canvas.paste(im, (pl, pt))
        im, (w, h) = canvas, canvas.size
    top, left = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
    im = im.crop((left, top, left + size, top + size))
    x = torch.from_numpy(np.asarray(im, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255)
    return ((x - 0.5) / 0.5).unsqueeze(0).to(device)


def reference_gray_u8(img_hwc):
    """The gray uint8 image the drivers hand to dlib (:161-163): cv2.normalize(img, None, 0, 255, NORM_MINMAX, CV_8U) over
    the whole float image, then cv2.cvtColor(..., COLOR_BGR2GRAY) applied to RGB-ordered data (so channel 0 gets the blue
    weight) -- restated in numpy with OpenCV's 8-bit fixed-point coefficients (B 1868, G 9617, R 4899, >> 14)."""
    x = np.asarray(img_hwc, dtype=np.float32)
    lo, hi = float(x.min()), float(x.max())
    scale = 255.0 / (hi - lo) if hi > lo else 0.0
    u8 = np.clip(np.rint((x.astype(np.float64) - lo) * scale), 0, 255).astype(np.uint8)
    c = u8.astype(np.uint32)
    return ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def to_uint8_image(G, img):
    """[1,C,H,W] float32 device image in [-1,1] -> uint8 HWC numpy (misc.to_pil's rint+clip, misc.py:114-130) on the device."""
    return misc.to_uint8(img)


def save_image(G, img, path, ratio=1.0):
    """`crop(misc.to_pil(img[0]), ratio).save(path)` of the drivers (...sqz_MSE.py:190-195)."""
    im = misc.crop_max_rectangle(misc.to_pil(img), ratio)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    im.save(path)
    return path


def noise_mat_key(layer_name):
    """The .mat key of a layer's optimised noise map: 'synthesis.b64.conv0' -> 'noise_b64_conv0' (MATLAB variable names hold no dots)."""
    return "noise_" + layer_name.replace("synthesis.", "").replace(".", "_")


def save_latent_mat(path, w, noises=None):
    """`{'w': float32 [1,k,D]}` in MATLAB v5 format, like sio.savemat in the drivers (:201-206).  noises: {layer name: map} of a
    projection that optimised the noise maps -- stored as [res, res] float32 arrays under noise_mat_key(name) beside 'w'."""
    import scipy.io as sio
    w = misc.as_numpy(w, np.float32)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    out = {"w": w}
    for name, t in (noises or {}).items():
        m = misc.as_numpy(t, np.float32)
        out[noise_mat_key(name)] = m.reshape(m.shape[-2], m.shape[-1])
    sio.savemat(path, out)
    return path


def load_latent_mat(path):
    import scipy.io as sio
    w = np.asarray(sio.loadmat(path)["w"], dtype=np.float32)
    if w.ndim not in (3, 4):
        raise ValueError(f"{path}: 'w' has shape {w.shape}, expected [1,k,D] (or a W+ latent [1,k,num_ws,D])")
    return w


# ----------------------------------------------------------------------------------------------------------------- drivers
def generate_images(G, images_num=32, truncation_psi=0.7, output_dir=None, ratio=1.0, seed=None, noise_mode="random"):
    """1024_generate.py:31-41.  Returns the list of z tensors used (and writes sample_%06d.png when `output_dir` is given)."""
    gen = seeded_generator(G.device, seed)
    zs = []
    for i in range(images_num):
        z = torch.randn([1, G.cfg.k, G.cfg.z_dim], device=G.device, generator=gen)
        img = G(z, truncation_psi=truncation_psi, noise_mode=noise_mode)[0]
        if output_dir is not None:
            save_image(G, img, os.path.join(output_dir, f"sample_{i:06d}.png"), ratio)
        zs.append(z.cpu())
    return zs


def render_latent(G, w, truncation_psi=0.7, noise_mode="random", noise_key=None, noise_step=None):
    """The image of a projected latent as the morph drivers render it: `G(w, truncation_psi)` for a z latent [n,k,D] (the 0.7 lands in `c`,
    SURVEY 0.2) and `G(ws=w)` for a W+ latent [n,k,num_ws,D] (gradient mode, latent_space="w+": every layer reads its own slot;
    truncation acts in the mapping network only, networks.py:935-941, so there is none to apply).  -> [n,3,R,R], the caller's own tensor.
    noise_mode="keyed" with noise_key / noise_step (a projection result's `noise_key` and `step`): the per-layer maps that step of a
    noise_mode="keyed" projection was scored with, for every latent of `w` -- the image the loop ranked, rendered again."""
    w = (w if isinstance(w, torch.Tensor) else torch.from_numpy(np.asarray(w, dtype=np.float32))).to(G.device)
    keyed = dict(noise_key=noise_key, noise_step=noise_step, noise_step_add=0) if noise_mode == "keyed" else {}
    if w.ndim == 4:
        return G(ws=w, noise_mode=noise_mode, **keyed)[0]
    return G(w, truncation_psi, noise_mode=noise_mode, **keyed)[0]


def merge_morph(G, w1, w2, alphas=(0.5,), truncation_psi=0.7, noise_mode="random", out_prefix=None, ratio=1.0, batched=False):
    """Linear latent morphs `dw = (1-a) w1 + a w2` rendered with G(dw, psi) (1024_merge_morph_2.py:83-92).
    w1/w2: numpy or tensors [1,k,D] (what the `.mat` files hold), or two W+ results [1,k,num_ws,D] -- blended slot by slot and rendered
    through `G(ws=...)` (render_latent).  Returns (latents [A,1,k,D] numpy, images [A,3,H,W] device).
    The blend is done in numpy float32 exactly like the reference (`0.5 * w1 + 0.5 * w2` on loadmat arrays).
    batched=True renders the whole sweep with ONE generator forward of len(alphas) images (BASELINE config 4's 11-alpha sweep as one
    batch-11 forward) instead of one forward per alpha like the script; the images agree to float32 rounding (other kernel shapes)."""
    _, blend = _latent_pair(w1, w2, "merge_morph")
    lat, imgs = [], []
    sweep = render_latent(G, np.concatenate([blend(a) for a in alphas]), truncation_psi, noise_mode) if batched and len(alphas) > 1 else None
    for j, a in enumerate(alphas):
        dw = blend(a)
        img = sweep[j:j + 1] if sweep is not None else render_latent(G, dw, truncation_psi, noise_mode)
        if out_prefix is not None:
            tag = f"{out_prefix}_a{a:.2f}"
            save_image(G, img, tag + ".jpg", ratio)
            save_latent_mat(tag + ".mat", dw)
        lat.append(dw)
        imgs.append(img[0].clone())
    return np.stack(lat), torch.stack(imgs)


def _blend_latents(a1, a2, a):
    """merge_morph's latent blend in its float32 numpy arithmetic (`0.5 * w1 + 0.5 * w2` on loadmat arrays, 1024_merge_morph_2.py:83)."""
    return (0.5 * a1 + 0.5 * a2) if a == 0.5 else (np.float32(1.0 - a) * a1 + np.float32(a) * a2)


def _latent_pair(w1, w2, who):
    """The two latents of a morph (numpy or tensors) as float32 arrays of one shape -> (the first, alpha -> their blend)."""
    a1, a2 = misc.as_numpy(w1, np.float32), misc.as_numpy(w2, np.float32)
    if a1.shape != a2.shape:
        raise ValueError(f"{who}: the two latents differ in shape: {a1.shape} vs {a2.shape}")
    return a1, lambda a: _blend_latents(a1, a2, a)


def refine_morph(G, w1, w2, target_a, target_b, alphas=(0.5,), lockstep=True, args: ProjectionArgs = None, percept=None, biometric=None,
                 gamma=1.0, id_balance=0.0, id_metric="mse", latent_std=None, eps=None, seed=None, use_graph=True, noise_mode="random",
                 use_mse=True, lm_target=None, lm_target_b=None, lm_steps=None, weight_decay=0.0, mode="gradient", out_prefix=None, ratio=None,
                 region_weight=None, face_crop=None, face_crop_b=None, face_crop_filter="area"):
    """Morph refinement: for every alpha start at merge_morph's blend (1 - a) w1 + a w2 (the same float32 arithmetic) and descend it so that
    the image matches BOTH contributing subjects -- target_a weighted 1 - a, target_b weighted a: perceptually, in pixels and in identity
    space, the two identity distances kept in balance by id_balance |d_a - d_b| (GradientProjectionEngine(target_b=...) has the objective).
    w1 / w2: [1,k,D] z latents or [1,k,num_ws,D] W+ latents (what the `.mat` files hold; the latent space follows their shape);
    target_a / target_b: [1,3,S,S].  lockstep=True refines all alphas in ONE engine (B lockstep pairs, one generator forward / backward per
    step); False runs one engine per alpha on the same noise stream.  latent_std: the perturbation scale around the start (default: the
    latent statistics' scale, as for a projection).  lm_target / lm_target_b [68,2] and lm_steps [steps,68,2] add the Wing term against the
    blended landmarks.  Returns one dict per alpha: alpha, w_start (numpy), w (best latent, [1,k,D] or W+), losses, best_step, best_loss,
    id_distances ((d_a, d_b) at the best step; None without a biometric term).  out_prefix: `<prefix>_a{alpha:.2f}_refined.mat / .png`, the
    image rendered like a projection result (no truncation).  region_weight: one map [S,S] >= 0 that weights the LPIPS and pixel terms of
    every alpha (GradientProjectionEngine(region_weight=...); `face_region_weight` builds one from landmarks).  face_crop / face_crop_b: the
    identity term embeds through the aligned face crop (BiometricLoss.set_crop) -- the [2,3] matrices under which target_a / target_b are
    embedded (face_crop_b: face_crop by default), or "landmarks": arcface_crop of lm_target / lm_target_b.  The candidate of alpha is cropped by
    arcface_crop of the blended landmarks (1 - a) lm_target + a lm_target_b, or, with matrices given, by their blend (a blend of
    similarities is one).  face_crop_filter: "area" or "bilinear"."""
    if mode != "gradient":
        raise ValueError(f"refine_morph descends the objective: mode must be 'gradient' (got {mode!r}; the literal loop never moves the latent)")
    a1, blend = _latent_pair(w1, w2, "refine_morph")
    if a1.ndim not in (3, 4) or a1.shape[0] != 1:
        raise ValueError(f"refine_morph: latents must be [1,k,D] or [1,k,num_ws,D] (got {a1.shape})")
    alphas = [float(a) for a in alphas]
    if not alphas or not all(0.0 <= a <= 1.0 for a in alphas):
        raise ValueError(f"refine_morph: alphas must lie in [0, 1] (got {alphas})")
    if tuple(target_a.shape) != tuple(target_b.shape) or target_a.shape[0] != 1:
        raise ValueError(f"refine_morph: target_a and target_b must both be [1,3,S,S] (got {tuple(target_a.shape)} and {tuple(target_b.shape)})")
    args = args or ProjectionArgs()
    space = "w+" if a1.ndim == 4 else "z"
    starts = [blend(a) for a in alphas]
    B = len(alphas)
    dev = G.device
    if latent_std is None:
        _, latent_std = seeded_latent_stats(G, args, space, seed)
    ls = tuple(a1.shape[1:])
    if eps is None:                      # one stream for the whole sweep: lockstep or not, alpha j sees the same noise
        eps = seeded_randn((args.step, B, *ls), dev, 0 if seed is None else seed)
    eps = eps.to(dev).float().reshape(-1, B, *ls)
    crop_kw = lambda js: {}
    if face_crop is not None or face_crop_b is not None:
        if face_crop is None or biometric is None:
            raise ValueError("refine_morph: face_crop_b needs face_crop, and both need a biometric term")
        ma = _resolve_crop(face_crop, lm_target, "face_crop")
        mb = ma if face_crop_b is None else _resolve_crop(face_crop_b, lm_target_b, "face_crop_b")
        if ma.shape != (2, 3) or mb.shape != (2, 3):
            raise ValueError(f"refine_morph: face_crop / face_crop_b are one [2,3] matrix each (got {ma.shape}, {mb.shape})")
        if isinstance(face_crop, str) and isinstance(face_crop_b, str):      # the landmarks the engine blends for the Wing term
            la, lb = np.asarray(lm_target, dtype=np.float64), np.asarray(lm_target_b, dtype=np.float64)
            pred = lambda a: arcface_crop((1.0 - a) * la + a * lb)
        else:
            pred = lambda a: (1.0 - a) * ma + a * mb
        crop_kw = lambda js: dict(face_crop=np.stack([pred(alphas[j]) for j in js]), face_crop_target=ma, face_crop_target_b=mb,
                                  face_crop_filter=face_crop_filter)

    def run(js):
        n = len(js)
        rep = lambda t: t.expand(n, *t.shape[1:]).contiguous()
        lm_kw = {}
        if lm_target is not None:
            tile = lambda x: np.asarray(x, dtype=np.float64) if n == 1 else np.stack([np.asarray(x, dtype=np.float64)] * n)
            lm_kw = dict(lm_target=tile(lm_target), lm_steps=tile(lm_steps), lm_target_b=None if lm_target_b is None else tile(lm_target_b))
        eng = GradientProjectionEngine(G, rep(target_a), torch.from_numpy(np.concatenate([starts[j] for j in js])).to(dev), float(latent_std), args,
                                       weight_decay=weight_decay, percept=percept, eps=eps[:, js].contiguous(), noise_mode=noise_mode,
                                       use_graph=use_graph, use_mse=use_mse, latent_space=space, biometric=biometric, gamma=gamma,
                                       target_b=rep(target_b), morph_alpha=[alphas[j] for j in js], id_balance=id_balance, id_metric=id_metric,
                                       region_weight=region_weight, **lm_kw, **crop_kw(js))
        w, step, loss, losses = eng.run().result()
        trace = None if eng.id_trace is None else eng.id_trace.cpu().numpy()
        if n == 1:
            w, step, loss, losses = w, [step], [loss], losses[None]
        return [dict(alpha=alphas[j], w_start=starts[j], w=w[i:i + 1].clone(), losses=np.asarray(losses[i]), best_step=int(step[i]),
                     best_loss=float(loss[i]), id_distances=None if trace is None else (float(trace[i, int(step[i]), 0]), float(trace[i, int(step[i]), 1])))
                for i, j in enumerate(js)]

    out = run(list(range(B))) if lockstep else [r for j in range(B) for r in run([j])]
    if out_prefix is not None:
        for r in out:
            tag = f"{out_prefix}_a{r['alpha']:.2f}_refined"
            save_latent_mat(tag + ".mat", r["w"])
            r["image"] = save_best_png(G, r["w"], tag + ".png", args.ratio if ratio is None else ratio)
    return out


def demorph_latent(w_morph, w_ref, alpha=0.5):
    """The closed-form de-morph of two projections: merge_morph's `w_M = (1 - a) w_A + a w_B` solved for the other contributor,
    `w_B = (w_M - (1 - a) w_A) / a`, in float32 numpy like the blend it inverts.  w_morph / w_ref: z latents [1,k,D] or W+ latents
    [1,k,num_ws,D] of one shape.  The errors of both projections come back amplified by 1 / a: alpha must lie in (0, 1]."""
    alpha = float(alpha)
    if not 0.0 < alpha <= 1.0:
        raise ValueError(f"demorph_latent: alpha must lie in (0, 1] (got {alpha}): at alpha = 0 the morph holds nothing of the other contributor")
    _latent_pair(w_morph, w_ref, "demorph_latent")
    wm, wa = misc.as_numpy(w_morph, np.float32), misc.as_numpy(w_ref, np.float32)
    return (wm - np.float32(1.0 - alpha) * wa) / np.float32(alpha)


def demorph(G, morph_img, reference_img, w_morph=None, w_ref=None, alpha=0.5, args: ProjectionArgs = None, percept=None, biometric=None,
            gamma=1.0, use_mse=True, row_weight=(1.0, 1.0), latent_std=None, latent_space=None, eps=None, seed=None, use_graph=True,
            noise_mode="random", lm_target=None, lm_steps=None, lm_valid=None, region_weight=None, face_crop=None, face_crop_target=None,
            face_crop_filter="area", weight_decay=0.0, out_prefix=None, ratio=None):
    """Reference-based de-morphing: restore the second contributor of the suspected morph `morph_img` [1,3,S,S] from `reference_img`, one
    trusted image of the first, by the coupled descent of demorph.DemorphEngine (G((1 - alpha) p_A + alpha p_B) against the morph, G(p_A)
    against the reference; the restored face is G(p_B)).  w_morph / w_ref: the latents of earlier projections of the two images (what the
    `.mat` files hold, z or W+; both or neither) -- the descent then starts at p_A = w_ref, p_B = demorph_latent(w_morph, w_ref, alpha); without
    them both parameters start at the latent mean (`latent_space`: "z", the default, or "w+").  Returns the engine's result (w_a, w_b, best_step,
    best_loss, losses, row_losses) plus w_start_b.  out_prefix: `<prefix>_restored.mat / .png` (w_b, rendered like a projection result) and
    `<prefix>_reference.mat` (w_a)."""
    from .demorph import DemorphEngine
    args = args or ProjectionArgs()
    if (w_morph is None) != (w_ref is None):
        raise ValueError("demorph: w_morph and w_ref come together (the closed-form start needs both projections)")
    if w_morph is not None:
        start_b = demorph_latent(w_morph, w_ref, alpha)
        start_a = misc.as_numpy(w_ref, np.float32)
        if start_a.ndim not in (3, 4) or start_a.shape[0] != 1:
            raise ValueError(f"demorph: latents must be [1,k,D] or [1,k,num_ws,D] (got {start_a.shape})")
        space = "w+" if start_a.ndim == 4 else "z"
        if latent_space not in (None, space):
            raise ValueError(f"demorph: latent_space={latent_space!r} but the latents are {space} latents {start_a.shape}")
    else:
        space = latent_space or "z"
    mean, std = (None, latent_std) if (latent_std is not None and w_morph is not None) else seeded_latent_stats(G, args, space, seed)
    if latent_std is None:
        latent_std = std
    if w_morph is None:
        start_a = start_b = misc.as_numpy(mean, np.float32)[None]
    to_dev = lambda w: torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(G.device)
    eng = DemorphEngine(G, morph_img, reference_img, to_dev(start_a), to_dev(start_b), float(latent_std), args, alpha=alpha, row_weight=row_weight,
                        percept=percept, biometric=biometric, gamma=gamma, use_mse=use_mse, lm_target=lm_target, lm_steps=lm_steps, lm_valid=lm_valid,
                        eps=eps, latent_space=space, region_weight=region_weight, face_crop=face_crop, face_crop_target=face_crop_target,
                        face_crop_filter=face_crop_filter, use_graph=use_graph, weight_decay=weight_decay, noise_mode=noise_mode,
                        seed=0 if seed is None else seed)
    res = eng.run().result()
    res["w_start_b"] = np.asarray(start_b, dtype=np.float32)
    if out_prefix is not None:
        save_latent_mat(out_prefix + "_restored.mat", res["w_b"])
        save_latent_mat(out_prefix + "_reference.mat", res["w_a"])
        res["image"] = save_best_png(G, res["w_b"], out_prefix + "_restored.png", args.ratio if ratio is None else ratio)
    return res


def merge_morph_tree(G, src_path, dst_path, truncation_psi=0.7, ratio=1.0, noise_mode="random"):
    """The directory walk of 1024_merge_morph_2.py:53-92: `src_path/<id>/<name>/` holds the projected latents (`.mat`, beside their `.png`s) of
    one bona fide image; every id folder has two such name folders (entries with a dot are skipped, :61-63; the first two are used, :64-65), and
    every latent of the first is morphed with every latent of the second -- `0.5 * w1 + 0.5 * w2`, rendered with `G(W, truncation_psi)` -- into
    `dst_path/<id>/<stem1>+<stem2>.jpg / .mat` (:77-92); pairs whose image already exists are skipped (:80).  Returns the list of written stems."""
    done = []
    for ident in sorted(os.listdir(src_path)):
        id_dir = os.path.join(src_path, ident)
        if not os.path.isdir(id_dir):
            continue
        names = [nm for nm in sorted(os.listdir(id_dir)) if len(nm.split(".")) == 1]
        if len(names) < 2:
            raise ValueError(f"{id_dir}: needs the latent folders of two bona fide images, found {names}")
        dst_id = os.path.join(dst_path, ident)
        os.makedirs(dst_id, exist_ok=True)
        mats = [[f for f in sorted(os.listdir(os.path.join(id_dir, nm))) if f.endswith(".mat")] for nm in names[:2]]
        for im1 in mats[0]:
            w1 = load_latent_mat(os.path.join(id_dir, names[0], im1))
            for im2 in mats[1]:
                stem = im1[:-4] + "+" + im2[:-4]
                if os.path.exists(os.path.join(dst_id, stem + ".jpg")):
                    continue
                w2 = load_latent_mat(os.path.join(id_dir, names[1], im2))
                lat, imgs = merge_morph(G, w1, w2, (0.5,), truncation_psi, noise_mode=noise_mode)
                save_image(G, imgs[0:1], os.path.join(dst_id, stem + ".jpg"), ratio)
                save_latent_mat(os.path.join(dst_id, stem + ".mat"), lat[0])
                done.append(os.path.join(ident, stem))
    return done


def merge_files(src_path, dst_path):
    """1024_merge_files.py:20-45, the step in front of the morph walk above ("combine all bonafides from different results"): a results tree
    `src_path/<version>/<variant>/<id>/<name>/<file>` is folded over its variants into `dst_path/<version>/<id>/<name>/<file>` -- the per-image
    folders of every variant of a version land side by side under one id; entries of an id folder that carry a dot are skipped (:36), files
    are copied with `shutil.copy` (a later variant's file of the same name overwrites an earlier one, as in the script, which walks
    `os.listdir` order; here sorted, so the result does not depend on the file system).  Host-side file bookkeeping: no tensor is touched.
    Returns the list of destination files."""
    import shutil
    out = []
    for version in sorted(os.listdir(src_path)):
        v_dir = os.path.join(src_path, version)
        if not os.path.isdir(v_dir):
            continue
        os.makedirs(os.path.join(dst_path, version), exist_ok=True)          # (:23-25: made even when the version holds no variant)
        for variant in sorted(os.listdir(v_dir)):
            for ident in sorted(os.listdir(os.path.join(v_dir, variant))):
                id_dir = os.path.join(v_dir, variant, ident)
                for name in sorted(os.listdir(id_dir)):
                    if len(name.split(".")) > 1:
                        continue
                    dst_fold = os.path.join(dst_path, version, ident, name)
                    os.makedirs(dst_fold, exist_ok=True)
                    for img in sorted(os.listdir(os.path.join(id_dir, name))):
                        out.append(shutil.copy(os.path.join(id_dir, name, img), os.path.join(dst_fold, img)))
    return out


# the five points ArcFace networks are trained on, in a 112 x 112 crop (insightface's arcface_dst): eye centres, nose tip, mouth corners
ARCFACE_TEMPLATE = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]], dtype=np.float64)


def arcface_crop(landmarks, size=112):
    """The crop matrix M [2,3] float64 of `BiometricLoss.set_crop` from face landmarks: crop pixel index (u, v) -> image pixel index, the
    least-squares similarity (Umeyama 1991, a reflection excluded) that carries the ArcFace template, scaled by size / 112, onto the face's five
    points.  landmarks: [5,2] (x, y) -- left eye, right eye, nose tip, left and right mouth corner as the image shows them -- or the [68,2]
    set of the Wing term, of which the eye centres mean(36:42) and mean(42:48), the nose tip 30 and the mouth corners 48 and 54 are taken.
    Host only."""
    pts = misc.as_numpy(landmarks, np.float64)
    if pts.shape == (68, 2):
        pts = np.stack([pts[36:42].mean(0), pts[42:48].mean(0), pts[30], pts[48], pts[54]])
    if pts.shape != (5, 2) or not np.all(np.isfinite(pts)):
        raise ValueError(f"arcface_crop: landmarks must be finite [68,2] or [5,2] points (got {pts.shape})")
    src = ARCFACE_TEMPLATE * (float(size) / 112.0)
    mu_s, mu_d = src.mean(0), pts.mean(0)
    sc, dc = src - mu_s, pts - mu_d
    U, D, Vt = np.linalg.svd(dc.T @ sc / 5.0)
    e = np.array([1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])      # the proper rotation closest to the fit, never a mirror image
    R = U @ np.diag(e) @ Vt
    scale = float((D * e).sum() / ((sc ** 2).sum() / 5.0))
    return np.concatenate([scale * R, (mu_d - scale * R @ mu_s)[:, None]], axis=1)


def scale_crop(M, f):
    """M re-expressed for the image block-averaged by f (ProjectionArgs.pool_above): pixel index x of the image is index x' = (x + 1/2) / f - 1/2
    of the pooled one (pixel centres; a block's mean sits at the block's centre).  M [2,3] or [n,2,3] -> float64 of the same shape."""
    M = np.array(misc.as_numpy(M), dtype=np.float64)         # (a copy: the caller's matrix stays as it is)
    M[..., :, :2] /= float(f)
    M[..., :, 2] = (M[..., :, 2] + 0.5) / float(f) - 0.5
    return M


def _resolve_crop(face_crop, landmarks, what):
    """A face_crop argument as float64 matrices: given as such, or "landmarks" -> arcface_crop of one [68,2] / [5,2] set or of each of B sets."""
    if isinstance(face_crop, str):
        if face_crop != "landmarks":
            raise ValueError(f"{what} must be a [2,3] matrix or 'landmarks' (got {face_crop!r})")
        if landmarks is None:
            raise ValueError(f"{what}='landmarks' needs the landmarks it is derived from")
        lm = misc.as_numpy(landmarks, np.float64)
        return arcface_crop(lm) if lm.ndim == 2 else np.stack([arcface_crop(l) for l in lm])
    return misc.as_numpy(face_crop, np.float64)


def face_region_weight(landmarks, size, inside=1.0, outside=0.0, feather=0.0):
    """A region weight from face landmarks: `inside` on the convex hull of the [68,2] (x, y) points, `outside` elsewhere -- the landmark hull is
    the region the reference's warp script treats as the face (1024_warp_morphs.py:160-210 triangulates exactly these points).  Host only: the
    hull is scipy.spatial.ConvexHull, filled as a polygon (Pillow ImageDraw, boundary included); feather > 0 blurs the edge with a Gaussian of
    that sigma in pixels (scipy.ndimage.gaussian_filter).  -> float32 [size, size] for the engines' region_weight."""
    from PIL import Image, ImageDraw
    from scipy.spatial import ConvexHull
    pts = np.asarray(landmarks, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] < 3 or not np.isfinite(pts).all():
        raise ValueError(f"face_region_weight: landmarks must be finite [P,2] points, P >= 3 (got {pts.shape})")
    if inside < 0 or outside < 0 or feather < 0 or max(inside, outside) <= 0:
        raise ValueError("face_region_weight: inside, outside >= 0 (not both zero) and feather >= 0")
    hull = pts[ConvexHull(pts).vertices]                         # counter-clockwise
    mask = Image.new("L", (int(size), int(size)), 0)
    ImageDraw.Draw(mask).polygon([(float(x), float(y)) for x, y in hull], fill=1, outline=1)
    w = np.where(np.asarray(mask) > 0, float(inside), float(outside))
    if feather > 0:
        from scipy.ndimage import gaussian_filter
        w = gaussian_filter(w, sigma=float(feather), mode="nearest")
    return np.ascontiguousarray(w, dtype=np.float32)


def load_region_weight(path):
    """A region weight file -> float32 [H,W]: a .npy float map as it is, any image file as its gray values scaled to [0, 1]."""
    if str(path).endswith(".npy"):
        w = np.load(path)
    else:
        from PIL import Image
        w = np.asarray(Image.open(path).convert("L"), dtype=np.float32) / 255.0
    if w.ndim != 2:
        raise ValueError(f"{path}: a region weight is one [H,W] map (got {w.shape})")
    return np.ascontiguousarray(w, dtype=np.float32)


def lpips_map(percept, img, target):
    """Where `img` departs from `target`: the [N,1,H,W] map of a lpips.PerceptualLoss(spatial=True) (PNetLin.forward with spatial=True,
    lpips/networks_basic.py:75-76,85-87).  img: [N,3,H,H] in [-1,1]; target: [1,3,H,H] (shared) or [N,3,H,H]."""
    if percept is None or not getattr(percept, "spatial", False):
        raise ValueError("lpips_map needs a lpips.PerceptualLoss built with spatial=True")
    return percept(img, target)


def save_lpips_map(map, path, vmax=None):
    """`path + '.npy'`: the map as float32 [H,W]; `path + '.png'`: gray uint8 round(255 * min(map / vmax, 1)), vmax = the map's maximum
    unless given (an all-zero map gives an all-zero PNG).  map: [1,1,H,W] / [H,W], tensor or array.  Returns the two paths."""
    from PIL import Image
    m = misc.as_numpy(map, np.float32)
    m = m.reshape(m.shape[-2], m.shape[-1])
    top = float(m.max()) if vmax is None else float(vmax)
    scaled = np.minimum(m.astype(np.float64) / top, 1.0) if top > 0 else np.zeros(m.shape)
    u8 = np.clip(np.rint(255.0 * scaled), 0, 255).astype(np.uint8)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.save(path + ".npy", m)
    Image.fromarray(u8).save(path + ".png")
    return path + ".npy", path + ".png"


def _best_lpips_map(G, percept, w, target, noises):
    """The map of the best latent's image -- rendered as projection.save_best_png renders it -- against the target."""
    w = w.to(G.device)
    mode = "inject" if noises is not None else "const"
    if w.ndim == 4:
        img = G.forward_workspace(ws=w, noise_mode=mode, noises=noises)[0]
    else:
        img = G.forward_workspace(w, None, noise_mode=mode, noises=noises)[0]
    return lpips_map(percept, img.float(), target)[0, 0]


DEFAULT_BATCH = 32       # loop steps per generator forward in literal mode: the configuration bench.py times (1.6 GB of activations per step at 1024^2;
                         # measured 20 .. 64: 32 is the fastest, 25 -- the round-2 figure -- 1.5 - 3 % behind)


def project_image(G, target, lm_target, lm_steps, args: ProjectionArgs = None, percept=None, latent_mean=None, latent_std=None,
                  eps=None, out_prefix=None, batch=DEFAULT_BATCH, use_graph=True, noise_mode="random", use_mse=True, seed=None,
                  landmark_fn=None, mode="literal", weight_decay=0.0, path_to_gen=None, keep_images=64, engine=None,
                  return_engine=False, latent_space="z", landmark_input="float", biometric=None, gamma=1.0, lbp_target=None, pipeline=None,
                  mdf=None, optimize_noise=False, noise_init="randn", lpips_map=False, region_weight=None, face_crop=None,
                  face_crop_filter="area", elite=None, es_weights="log", mean_lr=1.0):
    """One full `projection(...)` call (:135-208).  `target`: [1,3,S,S] from image_transform; `lm_target` [68,2] and either
    `lm_steps` [steps,68,2] (injected landmark detections) or `landmark_fn` (host detector called on every generated image,
    see ProjectionEngine; landmark_input="gray_u8" hands it the drivers' gray uint8 image, built on the device).  mode="literal" is the loop as the reference executes it (best-of-N noisy sampling, `batch` steps per
    forward -- 32 by default, the benchmarked configuration; the result does not depend on it); mode="gradient" back-propagates the
    loss into the latent and lets Adam move it (GradientProjectionEngine; one candidate per step; weight_decay=1e-4 is the
    1024_example_MSE.py:117 optimizer; latent_space="w+" optimises the per-layer intermediate latent [k, num_ws, D] instead of z -- the
    statistics are then taken in w space, projection.latent_stats_w -- and `w` comes back as [1, k, num_ws, D]); mode="evolution" is the literal loop with a mean
    that moves (evolution.EvolutionProjectionEngine: every batch of candidates is a generation, after which the mean becomes the weighted average
    of its best `elite` candidates -- `es_weights` "log" or "equal", step `mean_lr` -- so terms without a gradient steer the latent too; z only,
    never pipelined; outputs and engine= re-targeting are literal mode's, and the result gains `mean` [1,k,D] and `elite_used`).  Returns dict(w, step,
    loss, losses).

    biometric / gamma: an iresnet.BiometricLoss (embedder "facenet" or "iresnetNN") adds gamma * MSE(embed(img), embed(target)) to the objective
    (BASELINE config 3; 1024_example_FaceNet_percept.py:147-158).  lbp_target: with args.pixel_term="lbp" the target FILE's LBP code map
    (lbp.target_feature; 1024_example_LBP_percept.py:140).  mdf: an mdf.MDFLoss adds the MDF discriminator-feature loss in the p_loss slot --
    the whole objective of 1024_example_mdfloss.py / projection_example_v1_mdfloss*.py with use_mse=False, args.min_loss_init=1000 (and
    args.pool_above=256 for the v1 scripts); literal mode only.

    Outputs, like the drivers: with `path_to_gen` the SCORED image of every improvement -- the candidate as it was generated and
    ranked, its random per-layer noise included -- is written as `{path_to_gen}/{step:06d}_{loss:04f}.png` (:190-195; literal mode:
    the images stay on the device during the run, `keep_images` slots that are spilled to the host between launch sequences, and are
    written afterwards; gradient mode: the best latent's rendering under that name).  `out_prefix` adds the latent as
    `{out_prefix}.mat` (key 'w', :201-206 of the morph drivers) and, when no `path_to_gen` trail is written, the best latent's
    rendering as `{out_prefix}.png`.

    pipeline: literal mode without a host landmark callback -- the losses and the selection of one batch of candidates run on a side stream while the
    generator already synthesises the next batch (ProjectionEngine(pipeline=True): same result, bit for bit; one more image batch of memory).  None
    (default) = where it was measured to pay: LPIPS(squeeze) without an embedder (+1.9 % on a 1000-step projection at 1024^2 and 32 candidates per
    forward; LPIPS(vgg) and the FaceNet term, whose own matrix work then competes with the generator's, lose 1 - 1.5 %, and with no perceptual term
    there is nothing to overlap, -0.5 %: those stay on one stream).

    optimize_noise / noise_init: gradient mode also descends the generator's per-layer noise maps (GradientProjectionEngine(optimize_noise=True):
    Adam + noise_normalize_, args.noise_regularize * the regulariser in the total).  The result gains `noises`, the maps of the best step's image;
    the PNG is rendered with them -- the scored image -- and the .mat holds them beside 'w' (noise_mat_key).

    lpips_map: with a spatial perceptual term (lpips.PerceptualLoss(spatial=True); the engines score with it exactly as with a non-spatial one)
    the result gains `lpips_map` [H,W]: where the best latent's image -- G(best latent, noise_mode="const"), or with optimize_noise the best
    step's maps, as the saved PNG is rendered -- departs from the target; with `path_to_gen` it is also written there as
    best_lpips_map.npy / .png (save_lpips_map).

    region_weight: a map [H,W] >= 0 at the size the image-space losses see that weights the LPIPS and pixel terms by region (both engines'
    region_weight; `face_region_weight` builds one from landmarks).  A re-targeted engine takes the new target's weight in place.

    face_crop: the biometric term (an ArcFace embedder) embeds candidates and target through the aligned, antialiased face crop
    (BiometricLoss.set_crop) instead of a resize of the whole frame: a [2,3] matrix, crop pixel index -> pixel index of the GENERATED image
    (`arcface_crop`), or "landmarks" = arcface_crop(lm_target).  Under args.pool_above it is re-expressed for the pooled image the losses see
    (`scale_crop`).  face_crop_filter: "area" (default) or "bilinear".  A re-targeted engine takes the new target's matrix in place.

    engine: a ProjectionEngine from an earlier call with the same generator, objective, step count and batch (return_engine=True
    hands it out) -- it is re-targeted in place (`ProjectionEngine.retarget`), which keeps its captured hipGraph and workspaces; this is
    how `project_many` walks a list of targets.

    noise_mode="keyed": the per-layer noise of step i is a function of (seed, i) alone (ProjectionEngine), so the run replays bit for bit and
    does not depend on how its steps were launched.  The result gains `noise_key` (the seed's 64 bits), the final PNG is rendered with the best
    step's maps instead of constant noise -- the scored image -- and render_latent(G, res["w"], noise_mode="keyed", noise_key=res["noise_key"],
    noise_step=res["step"]) renders it again."""
    args = args or ProjectionArgs()
    if mode not in ("literal", "gradient", "evolution"):
        raise ValueError(f"mode must be 'literal', 'gradient' or 'evolution' (got {mode!r})")
    sampling = mode in ("literal", "evolution")              # the loops that score `batch` candidates per forward and keep literal mode's outputs
    if engine is not None and not sampling:
        raise ValueError("engine= (re-targeting) is for literal and evolution mode")
    if mode == "evolution" and pipeline:
        raise _lib.MgfError("project_image: mode='evolution' is never pipelined (the next generation's candidates are drawn around a mean that "
                            "depends on this generation's losses)")
    if latent_space not in ("z", "w+") or (latent_space == "w+" and mode != "gradient"):
        raise ValueError("latent_space must be 'z', or 'w+' together with mode='gradient'")
    if optimize_noise and mode != "gradient":
        raise ValueError("optimize_noise needs mode='gradient' (the literal loop never back-propagates)")
    if lpips_map and (percept is None or not getattr(percept, "spatial", False)):
        raise ValueError("lpips_map=True needs a perceptual term that returns maps: percept=lpips.PerceptualLoss(spatial=True)")
    if lpips_map and tuple(target.shape[2:]) != (G.img_resolution, G.img_resolution):
        raise ValueError(f"lpips_map=True: the target is {tuple(target.shape[2:])}, the generated image {G.img_resolution}x{G.img_resolution} "
                         "(args.pool_above): the map is defined at the image's own size")
    crop = None
    if face_crop is not None:
        if biometric is None:
            raise ValueError("face_crop is the crop of the biometric term: pass biometric= with it")
        crop = _resolve_crop(face_crop, lm_target, "face_crop")
        f = args.pool_factor(G.img_resolution)
        if f > 1:
            crop = scale_crop(crop, f)
    if latent_mean is None or latent_std is None:
        latent_mean, latent_std = seeded_latent_stats(G, args, latent_space, seed)
    if pipeline is None:
        pipeline = mode == "literal" and landmark_fn is None and biometric is None and getattr(percept, "net", None) == "squeeze"
    keep = max(int(keep_images), int(batch)) if path_to_gen is not None and sampling else 0
    if engine is not None and (mode == "evolution") != isinstance(engine, EvolutionProjectionEngine):
        raise ValueError(f"engine= was built for another mode than {mode!r}")
    if engine is not None and mode == "evolution" and not (
            engine.elite == (max(1, batch // 4) if elite is None else int(elite)) and engine.mean_lr == float(mean_lr) and
            np.array_equal(engine.es_weight_table, recombination_weights(engine.elite, es_weights))):
        raise ValueError("engine= was built with another elite / es_weights / mean_lr")
    if engine is not None:
        if (engine.G is not G or engine.batch != batch or engine.steps != args.step or engine.keep_images != keep or
                engine.pipeline != (bool(pipeline) and landmark_fn is None)):
            raise ValueError("engine= was built for another generator / batch / step count / trail size / pipeline mode")
        # the objective is baked into the captured launch sequence: a re-targeted engine must score exactly what a fresh one would
        diff = [name for name, ok in (("landmarks (Wing term)", engine.use_wing == (lm_target is not None)),
                                      ("percept", engine.percept is percept), ("use_mse", engine.use_mse == bool(use_mse)),
                                      ("noise_mode", engine.noise_mode == noise_mode), ("args", engine.args == args),
                                      ("landmark_fn", engine.landmark_fn is landmark_fn), ("biometric", engine.biometric is biometric),
                                      ("gamma", biometric is None or engine.gamma == float(gamma)), ("mdf", engine.mdf is mdf),
                                      ("region_weight", engine.pixel.region_weighted == (region_weight is not None)),
                                      ("face_crop", engine.face_crop_filter == (face_crop_filter if crop is not None else None))) if not ok]
        if diff:
            raise ValueError("engine= was built for another objective: " + ", ".join(diff) + " differ(s); build a fresh engine")
        eng = engine.retarget(target, lm_target=lm_target, lm_steps=lm_steps, eps=eps, seed=seed if (eps is None or noise_mode == "keyed") else None,
                              latent_mean=latent_mean, latent_std=float(latent_std), lbp_target=lbp_target, region_weight=region_weight,
                              face_crop=crop)
    elif mode == "gradient":
        eng = GradientProjectionEngine(G, target, latent_mean, float(latent_std), args, weight_decay=weight_decay, percept=percept,
                                       lm_target=lm_target, lm_steps=lm_steps, eps=eps, noise_mode=noise_mode, use_graph=use_graph,
                                       use_mse=use_mse, landmark_fn=landmark_fn, seed=0 if seed is None else seed, latent_space=latent_space,
                                       biometric=biometric, gamma=gamma, mdf=mdf, optimize_noise=optimize_noise, noise_init=noise_init,
                                       region_weight=region_weight, face_crop=crop, face_crop_filter=face_crop_filter)
    else:
        es = dict(elite=elite, es_weights=es_weights, mean_lr=mean_lr) if mode == "evolution" else {}
        eng = (EvolutionProjectionEngine if es else ProjectionEngine)(
            G, target, latent_mean, float(latent_std), args, percept=percept, lm_target=lm_target,
            lm_steps=lm_steps, eps=eps, noise_mode=noise_mode, use_graph=use_graph, batch=batch, use_mse=use_mse,
            landmark_fn=landmark_fn, keep_images=keep, seed=0 if seed is None else seed, landmark_input=landmark_input,
            biometric=biometric, gamma=gamma, lbp_target=lbp_target, pipeline=pipeline, mdf=mdf, region_weight=region_weight,
            face_crop=crop, face_crop_filter=face_crop_filter, **es)
    w, step, loss, losses = eng.run().result()
    out = {"w": w, "step": step, "loss": loss, "losses": losses}
    if mode == "evolution":
        out["mean"], out["elite_used"] = eng.mean.cpu(), eng.elite_used()
    # noise_mode="keyed": the key the run drew under; with the best step it names the maps of the scored image, which every rendering below uses
    png_kw = {}
    if noise_mode == "keyed" and not optimize_noise:
        out["noise_key"] = int(eng.noise_key.item()) & 0xFFFFFFFFFFFFFFFF
        png_kw = dict(noise_mode="keyed", noise_key=out["noise_key"], noise_step=int(step))
    best_noises = None
    if optimize_noise:
        best_noises = {name: t.clone() for name, t in eng.best_noises.items()}
        out["noises"] = best_noises
    if out_prefix is not None:
        save_latent_mat(f"{out_prefix}.mat", w, noises=best_noises)
        if path_to_gen is None:                      # no improvement trail asked for: still leave an image of the result beside the latent
            out["image"] = save_best_png(G, w, f"{out_prefix}.png", args.ratio, noises=best_noises, **png_kw)
    if path_to_gen is not None:
        if sampling:
            out["images"] = eng.save_improvements(path_to_gen, args.ratio)
        else:
            out["images"] = [save_best_png(G, w, os.path.join(path_to_gen, "{:06d}_{:04f}.png".format(step, loss)), args.ratio, noises=best_noises, **png_kw)]
    if lpips_map:
        out["lpips_map"] = _best_lpips_map(G, percept, w, target, best_noises)
        if path_to_gen is not None:
            out["lpips_map_files"] = save_lpips_map(out["lpips_map"], os.path.join(path_to_gen, "best_lpips_map"))
    if return_engine:
        out["engine"] = eng
    return out


def project_many(G, targets, landmarks=None, dynamic=False, lockstep=1, region_weights=None, face_crops=None, out_prefixes=None, **kw):
    """Pair-level sharding of BASELINE configs 3/5: rank r projects `targets[r::world]` (or, with dynamic=True, whatever the
    shared `distributed.WorkQueue` hands it), then ONE all_gather returns every item's {latent, loss, step} to every rank.
    targets: list of [1,3,S,S] device tensors (or image paths); landmarks: optional list of (lm_target, lm_steps) per item.
    lockstep > 1 (gradient mode, static sharding): a rank advances that many of its items through one generator
    forward/backward per step (GradientProjectionEngine with B targets) instead of one after the other.
    In literal mode the rank builds ONE engine (latent statistics, LPIPS workspaces, hipGraph capture) for its first item and
    re-targets it for the others, as the reference keeps G / percept / latent statistics outside its per-image loop
    (projection_example_v2_percept_morph.py:311-355).
    region_weights: one region weight [H,W] for every item, or a list with one per item (project_image's region_weight).
    face_crops: one face crop per item (project_image's face_crop: a [2,3] matrix or "landmarks"), set before the item is projected -- a
    re-targeted engine takes it in place, a lockstep group gets its items' matrices as one [B,2,3] stack.
    optimize_noise=True with lockstep > 1: every target of a group optimises noise maps of its own (GradientProjectionEngine(
    noise_per_target=True)).  The maps do not fit the fixed-width gather: with out_prefixes (one path prefix per item) the rank that projected
    item i writes out_prefixes[i] + ".mat" (the latent and the best step's maps, save_latent_mat) and a PNG rendered with those maps, like
    project_image's out_prefix; without out_prefixes the maps are dropped and only the gathered latents remain.
    Returns dict(latents [N,k,D], losses [N], steps [N], items [N]) ordered by item id, plus `mine`: the items this rank worked on."""
    if isinstance(region_weights, (list, tuple)) and len(region_weights) != len(targets):
        raise ValueError(f"project_many: {len(region_weights)} region weights for {len(targets)} targets")
    rw = lambda i: region_weights[i] if isinstance(region_weights, (list, tuple)) else region_weights
    if face_crops is not None and len(face_crops) != len(targets):
        raise ValueError(f"project_many: {len(face_crops)} face crops for {len(targets)} targets")
    fc = lambda i: {} if face_crops is None else {"face_crop": face_crops[i]}
    if out_prefixes is not None:
        if len(out_prefixes) != len(targets):
            raise ValueError(f"project_many: {len(out_prefixes)} output prefixes for {len(targets)} targets")
        if not (lockstep > 1 and kw.get("optimize_noise")):
            raise ValueError("project_many: out_prefixes go with lockstep > 1 and optimize_noise=True (the per-target noise maps, which the "
                             "gather does not carry); the latents of every other run are in the result")
    import torch.distributed as dist
    from .distributed import gather_many, pack_result, run_sharded, shard_items, unpack_results
    on = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
    # an item is a device tensor, an image path, or a callable that produces the tensor when the item is taken (a rank only ever touches its own)
    tsize = G.img_resolution // (kw.get("args") or ProjectionArgs()).pool_factor(G.img_resolution)       # (projection_example_v1.py: the losses' size)
    load = lambda t: t if isinstance(t, torch.Tensor) else (t() if callable(t) else image_transform(t, size=tsize, device=G.device))
    w_plus = kw.get("latent_space", "z") == "w+"
    lshape = (G.cfg.k, G.cfg.num_ws, G.cfg.w_dim) if w_plus else (G.cfg.k, G.cfg.z_dim)      # a W+ result is [k, num_ws, D] per item
    width = int(np.prod(lshape)) + 3
    if w_plus and kw.get("mode") != "gradient":
        raise ValueError("latent_space='w+' needs mode='gradient'")
    if lockstep > 1:
        if dynamic or kw.get("mode") != "gradient":
            raise ValueError("lockstep groups need mode='gradient' and static sharding")
        recs = []
        mine = shard_items(len(targets), rank, world)
        for g0 in range(0, len(mine), lockstep):
            ids = mine[g0:g0 + lockstep]
            res = _project_group(G, [load(targets[i]) for i in ids], [landmarks[i] for i in ids] if landmarks is not None else None,
                                 region_weight=None if region_weights is None else [rw(i) for i in ids],
                                 **({} if face_crops is None else {"face_crop": [face_crops[i] for i in ids]}), **kw)
            recs += [pack_result(res["w"][j:j + 1].to(G.device), float(res["loss"][j]), int(res["step"][j]), item=i) for j, i in enumerate(ids)]
            if out_prefixes is not None:
                ratio = (kw.get("args") or ProjectionArgs()).ratio
                for j, i in enumerate(ids):
                    maps = {name: t[None] for name, t in res["noises"][j].items()}
                    save_latent_mat(f"{out_prefixes[i]}.mat", res["w"][j:j + 1], noises=maps)
                    save_best_png(G, res["w"][j:j + 1], f"{out_prefixes[i]}.png", ratio, noises=maps)
        rows = torch.stack(recs) if recs else torch.empty([0, width], dtype=torch.float64, device=G.device)
        out = unpack_results(gather_many(rows, -(-len(targets) // world)), lshape)
        out["mine"] = list(mine)
        return out
    reuse = kw.get("mode", "literal") in ("literal", "evolution") and kw.get("landmark_fn") is None and kw.get("eps") is None
    if reuse and (kw.get("latent_mean") is None or kw.get("latent_std") is None):
        kw["latent_mean"], kw["latent_std"] = seeded_latent_stats(G, kw.get("args") or ProjectionArgs(), "z", kw.get("seed"))   # once per rank, not per item
    state = {"eng": None}

    def work(i):
        lm_t, lm_s = landmarks[i] if landmarks is not None else (None, None)
        eng = state["eng"]
        if eng is not None and eng.use_wing != (lm_t is not None):
            eng = None                     # an item with / without landmarks after one without / with: another objective, a fresh engine
        r = project_image(G, load(targets[i]), lm_t, lm_s, engine=eng, return_engine=reuse, region_weight=rw(i), **fc(i), **kw)
        state["eng"] = r.get("engine")
        return pack_result(r["w"].to(G.device), r["loss"], r["step"], item=i)

    rows, mine = run_sharded(len(targets), work, width, G.device, dynamic=dynamic)
    out = unpack_results(rows, lshape)
    out["mine"] = mine                                       # the items THIS rank projected, in the order it took them
    return out


def read_pair_csv(path, threshold=0.5):
    """The pair list of projection_example_v2_percept_morph.py:337-343: rows `img1, img2, similarity`; the header row (`img1`) and rows below the
    similarity threshold are skipped.  -> [(img1, img2), ...]"""
    import csv
    pairs = []
    with open(path, "r", newline="") as fh:
        for row in csv.reader(fh):
            if not row or row[0] == "img1":
                continue
            if float(row[2]) < threshold:
                continue
            pairs.append((row[0], row[1]))
    return pairs


def morph_pairs(G, pairs, src_dir, dst_raw, dst_morph, landmarks=None, truncation_psi=0.7, ratio=1.0, noise_mode="random", **project_kw):
    """BASELINE config 3's outer loop (projection_example_v2_percept_morph.py:330-365): for every pair of bona fide images, project both into the
    latent space, render them (`<a>_<b>_A.png`, `_B.png` under dst_raw) and their 0.5 / 0.5 latent morph (`<a>_<b>.png` under dst_morph); pairs
    whose morph exists are skipped (:352).  The 2 x len(pairs) projections are independent: `project_many` shards them over the ranks of the
    process group (static or, with dynamic=True, through the work queue) and gathers every latent to every rank; the renderings are then
    dealt `pairs[rank::world]`.  pairs: [(img1, img2)] file names under src_dir (read_pair_csv); landmarks: optional {file name: (lm_target,
    lm_steps)}; project_kw: project_image's arguments (args, percept, biometric, gamma, batch, seed, mode, dynamic, ...) and project_many's
    (lockstep; with lockstep > 1 also optimize_noise / noise_init: per-target noise maps, and out_prefixes, one per projected file in
    pair order, to keep them -- the renderings here use `noise_mode`).
    Returns dict(pairs (the ones worked on), latents [2P,k,D] (W+: [2P,k,num_ws,D]), losses, steps, written (this rank's morph paths))."""
    import torch.distributed as dist
    from .distributed import shard_items
    stem = lambda f: f.split(".")[0]                          # (`img1.split('.')[0]`, :347)
    on = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
    # ONE rank looks at dst_morph and tells the others: the static shards and the size of the result gather are derived from this list, so
    # every rank must hold the same one (node-local scratch or a lagging network file system would otherwise let them disagree -- and an
    # empty list on some ranks only would let those skip the collective the others wait in)
    todo = [(a, b) for a, b in pairs if not os.path.exists(os.path.join(dst_morph, f"{stem(a)}_{stem(b)}.png"))] if rank == 0 else None
    if on and world > 1:
        box = [todo]
        dist.broadcast_object_list(box, src=0)
        todo = [tuple(pr) for pr in box[0]]
    if not todo:
        return {"pairs": [], "latents": None, "losses": None, "steps": None, "written": []}
    files = [f for pr in todo for f in pr]
    lms = None if landmarks is None else [landmarks[f] for f in files]
    res = project_many(G, [os.path.join(src_dir, f) for f in files], landmarks=lms, **project_kw)
    written = []
    for pi in shard_items(len(todo), rank, world):
        a, b = todo[pi]
        name = f"{stem(a)}_{stem(b)}"
        w1, w2 = res["latents"][2 * pi:2 * pi + 1], res["latents"][2 * pi + 1:2 * pi + 2]
        for w, tag in ((w1, "_A"), (w2, "_B")):                 # (a W+ result [1,k,num_ws,D] renders through G(ws=...): render_latent)
            save_image(G, render_latent(G, w, truncation_psi, noise_mode), os.path.join(dst_raw, name + tag + ".png"), ratio)
        _, imgs = merge_morph(G, w1, w2, (0.5,), truncation_psi, noise_mode=noise_mode)
        save_image(G, imgs[0:1], os.path.join(dst_morph, name + ".png"), ratio)
        written.append(os.path.join(dst_morph, name + ".png"))
    return {"pairs": todo, "latents": res["latents"], "losses": res["losses"], "steps": res["steps"], "written": written}


def _project_group(G, targets, landmarks, args: ProjectionArgs = None, percept=None, latent_mean=None, latent_std=None, eps=None,
                   use_graph=True, noise_mode="random", use_mse=True, seed=None, weight_decay=0.0, mode="gradient", latent_space="z",
                   biometric=None, gamma=1.0, batch=None, pipeline=None, mdf=None, region_weight=None, face_crop=None,
                   face_crop_filter="area", optimize_noise=False, noise_init="randn", **unused):
    """B targets through one lockstep GradientProjectionEngine; returns dict(w [B,k,D] (W+: [B,k,num_ws,D]), step [B], loss [B],
    losses [B,steps]).  optimize_noise: every target optimises its own noise maps (noise_per_target=True; the regulariser's weight is
    args.noise_regularize), and the result gains `noises`: one {layer: [res, res]} dict per target, the maps of its best step's image."""
    args = args or ProjectionArgs()
    if noise_init not in ("randn", "const"):
        raise ValueError(f"noise_init must be 'randn' or 'const' (got {noise_init!r})")
    if mdf is not None:
        raise _lib.MgfError("project_many(lockstep > 1): the MDF objective runs one target per engine in gradient mode; use lockstep=1")
    if unused or pipeline:                          # (`batch` is literal mode's steps per forward: gradient mode evaluates one candidate per step; `pipeline` is literal mode's too)
        unused = dict(unused, **({"pipeline": pipeline} if pipeline else {}))
        raise TypeError(f"project_many(lockstep=...): unsupported arguments {sorted(unused)}")
    if latent_mean is None or latent_std is None:
        latent_mean, latent_std = seeded_latent_stats(G, args, latent_space, seed)
    tg = torch.cat([t.reshape(1, *t.shape[-3:]) for t in targets]).contiguous()
    if region_weight is not None:                   # one map per target of the group
        region_weight = torch.stack([torch.as_tensor(misc.as_numpy(w, np.float64)).reshape(
            tg.shape[-2], tg.shape[-1]) for w in region_weight])[:, None]
    lm_t = lm_s = None
    if landmarks is not None:
        lm_t, lm_s = np.stack([np.asarray(l[0]) for l in landmarks]), np.stack([np.asarray(l[1]) for l in landmarks])
    if len(targets) == 1 and lm_t is not None:
        lm_t, lm_s = lm_t[0], lm_s[0]
    crop = None
    if face_crop is not None:                       # one crop per target of the group
        crop = np.stack([_resolve_crop(c, None if landmarks is None else landmarks[j][0], "face_crops[i]").reshape(2, 3)
                         for j, c in enumerate(face_crop)])
    eng = GradientProjectionEngine(G, tg, latent_mean, float(latent_std), args, weight_decay=weight_decay, percept=percept,
                                   lm_target=lm_t, lm_steps=lm_s, eps=eps, noise_mode=noise_mode, use_graph=use_graph, use_mse=use_mse,
                                   seed=0 if seed is None else seed, latent_space=latent_space, biometric=biometric, gamma=gamma,
                                   region_weight=region_weight, face_crop=crop, face_crop_filter=face_crop_filter,
                                   **(dict(optimize_noise=True, noise_per_target=True, noise_init=noise_init) if optimize_noise else {}))
    w, step, loss, losses = eng.run().result()
    out = {"w": w, "step": step, "loss": loss, "losses": losses}
    if len(targets) == 1:
        out = {"w": w, "step": np.array([step]), "loss": np.array([loss]), "losses": losses[None]}
    if noise_mode == "keyed" and not optimize_noise:
        out["noise_key"] = int(eng.noise_key.item()) & 0xFFFFFFFFFFFFFFFF
    if optimize_noise:
        out["noises"] = [{name: t[j].clone() for name, t in eng.best_noises.items()} for j in range(len(targets))]
    return out


def warp_morphs(G, w1, w2, landmark1, landmark2, landmark_G=None, landmark_fn=None, out_dir=None, truncation_psi=0.7, noise_mode="random"):
    """The whole of 1024_warp_morphs.py's main (:128-210): the 0.5 / 0.5 latent morph rendered with `G(W, truncation_psi)` (:153-156),
    the averaged landmarks of the two bona fide images + the 12 frame points triangulated (scipy Delaunay, :160-164), the morph's own
    landmarks (:166-168: `get_landmarks_G` -- here `landmark_G` [68,2], or `landmark_fn(gray uint8 [H,W])` called on the drivers' gray image
    of the morph), then every triangle of the morph warped onto the averaged mesh (:186-200) and written as bytes (:203-206).
    landmark1 / landmark2: [68,2] detections on the two source images (dlib is the caller's; `get_landmarks_img`, :46-56).
    Writes morph_G.png and Morph_final.png under `out_dir` when given.  Returns dict(latent [1,k,D], morph uint8 [H,W,3] (what the script
    reads back from morph_G.png), warped uint8 [H,W,3] (Morph_final.png), points_G, points_avg)."""
    lat, imgs = merge_morph(G, w1, w2, (0.5,), truncation_psi, noise_mode=noise_mode)
    img = imgs[0:1]
    size = int(img.shape[-1])
    morph_u8 = to_uint8_image(G, img)                       # the bytes misc.to_pil writes and cv2.imread reads back (channel order does not matter: per-channel work)
    if landmark_G is None:
        if landmark_fn is None:
            raise ValueError("warp_morphs: pass the morph's landmarks (landmark_G) or a detector (landmark_fn)")
        landmark_G = landmark_fn(gray_u8_device(img)[0])
        if landmark_G is None:                              # (the script would fail on `None.detach()` two lines later)
            raise _lib.MgfError("warp_morphs: the detector found no face in the morph")
    l1, l2, lg = (misc.as_numpy(v, np.float64).reshape(-1, 2) for v in (landmark1, landmark2, landmark_G))
    if not (l1.shape == l2.shape == lg.shape):
        raise ValueError(f"warp_morphs: landmark sets differ in shape: {l1.shape}, {l2.shape}, {lg.shape}")
    extra = np.asarray(frame_points(size), dtype=np.float64)
    points_avg = np.concatenate([(l1 + l2) / 2, extra])    # torch.div(landmark1.add(landmark2), 2) on DoubleTensors
    points_G = np.concatenate([lg, extra])
    warped = warp_morph_u8(morph_u8, points_G, points_avg)
    if out_dir is not None:
        from PIL import Image
        os.makedirs(out_dir, exist_ok=True)
        Image.fromarray(morph_u8, "RGB").save(os.path.join(out_dir, "morph_G.png"))
        Image.fromarray(warped, "RGB").save(os.path.join(out_dir, "Morph_final.png"))
    return {"latent": lat[0], "morph": morph_u8, "warped": warped, "points_G": points_G, "points_avg": points_avg}


def cv_resize_linear_u8(img_u8_hwc, width, height):
    """cv2.resize(I, (width, height)) of a uint8 image with the default INTER_LINEAR, restated from OpenCV's published sources (imgproc
    resize.cpp: half-pixel centres, coefficients rounded to 11-bit fixed point, HResizeLinear in int32, VResizeLinear<uchar>'s
    `(((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2`).  Host-side input formatting of one small image, like
    image_transform; cv2 is absent offline, so bit-parity with it is UNPINNED."""
    a = np.asarray(img_u8_hwc)
    assert a.dtype == np.uint8 and a.ndim == 3
    ih, iw = a.shape[:2]

    from .lbp import resize_table as table

    x0, x1, a0, a1 = table(width, iw)
    y0, y1, b0, b1 = table(height, ih)
    src = a.astype(np.int64)
    hrow = src[:, x0] * a0[None, :, None] + src[:, x1] * a1[None, :, None]             # [ih, width, c], scale 2048
    s0, s1 = hrow[y0], hrow[y1]
    out = (((b0[:, None, None] * (s0 >> 4)) >> 16) + ((b1[:, None, None] * (s1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def facenet_feature(image_u8_hwc, embedder):
    """extract_FaceNet.py:30-40: `cv2.resize(I, (224, 224))`, clamp to [0, 255], (x - 127.5) / 128, InceptionResnetV1 -> the flattened
    512-d embedding.  embedder: facenet.InceptionResnetV1Embedder (the HIP network; its weights are the caller's)."""
    small = cv_resize_linear_u8(image_u8_hwc, 224, 224)
    x = torch.from_numpy(small.astype(np.float32)).clamp_(0, 255).sub_(127.5).div_(128.0).permute(2, 0, 1)[None].contiguous()
    emb = embedder(x.to(embedder.device if hasattr(embedder, "device") else "cuda"))
    return emb.detach().cpu().numpy().reshape(-1)


def second_stage(G, target, w_init, latent_std, lm_target, lm_steps, **kw):
    """A second projection whose noisy candidates are drawn around an earlier result instead of the latent mean
    (edit_MSE.py: `latent_in = w1` pattern; BASELINE config 5)."""
    w0 = torch.as_tensor(misc.as_numpy(w_init, np.float32))
    return project_image(G, target, lm_target, lm_steps, latent_mean=w0.reshape(w0.shape[-2:]).to(G.device),
                         latent_std=latent_std, **kw)
