"""Command-line front ends with the reference scripts' arguments and defaults:

    python -m morphganformer_amd.cli generate --model net.pkl --output-dir images --images-num 32 --truncation-psi 0.7
                                              (1024_generate.py:44-54)
    python -m morphganformer_amd.cli project  --model net.pkl --image face.png --landmarks lm.npz --path_to_gen out/
                                              (1024_example_wing_loss_perceptual_sqz_MSE.py:222-268; argparse names kept)
    python -m morphganformer_amd.cli morph    --model net.pkl --w1 a.mat --w2 b.mat --alphas 0,0.1,...,1 --out out/a+b
                                              (1024_merge_morph_2.py:25-92)
    python -m morphganformer_amd.cli morph    ... --refine --image-a a.png --image-b b.png --biometric iresnet50 --id-balance 0.5
                                              (each blend descended against both subjects: <out>_a0.50_refined.mat / .png)
    python -m morphganformer_amd.cli lpips-map --image-a a.png --image-b b.png --out maps/a_vs_b --lpips-backbone squeeze.pth
                                              (where the two images differ: PNetLin(spatial=True), lpips/networks_basic.py:75-76; no model)

`--gpus` pins the visible device like the scripts' CUDA_VISIBLE_DEVICES line.  The reference detects landmarks with dlib on the
target and on every generated image; dlib is a closed third-party dependency, so `project` takes them from `--landmarks`
(an .npz with `target` [68,2] and `steps` [>=step,68,2], e.g. written by a detector run elsewhere) or, without it, runs the
MSE(+LPIPS) objective only (the 1024_example_MSE.py / ..._percept.py variants).

Options that subcommands share are declared once, in the `_*_arguments` groups `build_parser` composes; `_read_state_dict`, `_embedder_state`,
`_lpips_term`, `_biometric_term` and `_projection_args` build the pieces of an objective from a namespace, under the label (`project`,
`morph --refine`) their messages carry; every subcommand has one handler, which `main` looks up in `COMMANDS` with what to open for it.
"""
import argparse
import os
import sys


def _render_arguments(p, psi="--truncation_psi"):
    """What a rendering that is written as an image takes: --ratio and the truncation psi (`generate` spells it with a hyphen, like 1024_generate.py)."""
    p.add_argument("--ratio", type=float, default=1.0, help="height / width of the largest centred rectangle an image is cropped to when written")
    p.add_argument(psi, type=float, default=0.7)


def _objective_arguments(p, align_help=None):
    """Target size, step count, loss weights, seed and the LPIPS and biometric terms (1024_example_wing_loss_perceptual_sqz_MSE.py:222-245): the
    projection loop and `morph --refine`.  align_help: the subcommand's meaning of --biometric-align, where it has the option."""
    p.add_argument("--size", type=int, default=1024)
    p.add_argument("--n_mean_latent", type=int, default=10000)
    p.add_argument("--step", type=int, default=5000)
    p.add_argument("--lamda", type=float, default=0.01)
    p.add_argument("--beta", type=float, default=1)
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--noise", type=float, default=0.05)
    p.add_argument("--percept_weight", type=float, default=1.0, help="coefficient of the LPIPS term (0.5 with --beta 0.5 = 1024_example_percept_MSE.py)")
    p.add_argument("--msssim-levels", type=int, default=5,
                   help="--pixel-term msssim: levels of the 2 x 2 mean pyramid, 1..5 (every level's sides must be >= 11: 64 x 64 allows 3)")
    p.add_argument("--no-mse", action="store_true", help="drop the MSE term (beta * MSE)")
    p.add_argument("--no-lpips", action="store_true", help="MSE(+Wing) only, the 1024_example_MSE.py objective")
    p.add_argument("--seed", type=int, default=None)
    _lpips_arguments(p)
    p.add_argument("--biometric", type=str, default="none", choices=["none", "facenet", "iresnet18", "iresnet34", "iresnet50", "iresnet100", "mobilefacenet"],
                   help="add gamma * MSE(embed(img), embed(target)): facenet = InceptionResnetV1 on the un-resized image, the term "
                        "1024_example_FaceNet_percept.py:147-158 scores with (alone: --no-lpips --no-mse); iresnetNN = the vendored ArcFace network; "
                        "mobilefacenet = the vendored MobileFaceNet (same 112x112 -> 512-d contract, ~0.45 GFLOP per image)")
    p.add_argument("--gamma", type=float, default=1.0, help="coefficient of the biometric term")
    p.add_argument("--biometric-weights", type=str, default=None, metavar="STATE_DICT",
                   help="the embedder's state dict (.pth / .npz; facenet_pytorch's vggface2 weights, an insightface iresnet / mobilefacenet checkpoint) -- what the "
                        "reference fetches by name; required with --biometric unless --biometric-random")
    p.add_argument("--biometric-random", action="store_true", help="seeded random embedder weights (smoke runs only)")
    if align_help:
        p.add_argument("--biometric-align", action="store_true", help=align_help)
        p.add_argument("--biometric-crop-filter", choices=["area", "bilinear"], default="area",
                       help="--biometric-align: area = the mean over each crop pixel's footprint (default), bilinear = one sample per crop pixel")


def _lpips_arguments(p):
    """The LPIPS backbone and its weights: the objective and `lpips-map`."""
    p.add_argument("--net", type=str, default="squeeze", choices=["squeeze", "vgg", "alex"], help="LPIPS backbone")
    p.add_argument("--lpips-backbone", type=str, default=None, metavar="STATE_DICT",
                   help="torchvision feature weights of --net (.pth state dict or .npz with `features.N...` keys) -- what the reference "
                        "fetches with pretrained=True; required unless --no-lpips or --lpips-random-backbone")
    p.add_argument("--lpips-random-backbone", action="store_true",
                   help="score with SEEDED RANDOM backbone features (smoke runs only: the LPIPS term is then not a perceptual distance)")


def _lpips_pool_argument(p):
    """--lpips-pool-above: the LPIPS term's own block mean.  The module entries (`python -m morphganformer_amd.demorph`, `... .evolution`) add it;
    the subcommands of this parser keep the option tables tests/test_cli_parser_host.py pins, so they do not have it yet."""
    p.add_argument("--lpips-pool-above", type=int, default=0, metavar="N",
                   help="block-average images taller than N by height // N in front of the LPIPS backbone only (256: the v1 drivers' LPIPS size); "
                        "the pixel, biometric and MDF terms keep the full-size image, and gradient mode gets the adjoint")


def _loop_arguments(p, align_help=None):
    """The projection loop's arguments, shared by `project` and `morph-pairs` (1024_example_wing_loss_perceptual_sqz_MSE.py:222-245)."""
    p.add_argument("--model", type=str, default="models/ffhq-snapshot-1024_v2.pkl")
    _render_arguments(p)
    _objective_arguments(p, align_help)
    p.add_argument("--lr_rampup", type=float, default=0.05)
    p.add_argument("--lr_rampdown", type=float, default=0.25)
    p.add_argument("--noise_ramp", type=float, default=0.75)
    p.add_argument("--noise_regularize", type=float, default=1e5,
                   help="weight of the noise regulariser (…sqz_MSE.py:32-52,243); read with --optimize-noise, accepted and unused otherwise, like the reference")
    p.add_argument("--optimize-noise", action="store_true",
                   help="with --mode gradient (project): also descend the generator's per-layer noise maps (Adam + noise_normalize_, "
                        "--noise_regularize times the regulariser in the total); the .mat gains the best step's maps beside 'w'")
    p.add_argument("--noise-init", choices=["randn", "const"], default="randn",
                   help="--optimize-noise: start the maps from seeded N(0, 1) draws or from every layer's noise_const")
    p.add_argument("--w_plus", action="store_true",
                   help="with --mode gradient: optimise the per-layer latent W+ [k, num_ws, D] instead of z (the reference accepts the flag "
                        "and never reads it; in literal mode it stays unused here too)")
    p.add_argument("--pixel-term", choices=["mse", "psnr", "dssim", "lbp", "msssim"], default="mse",
                   help="psnr = the pixel term of 1024_example_PSNR.py (10 log10(255^2 / MSE), minimised like the script does, and -- see --psnr-layout -- "
                        "with the script's element order; use with --no-lpips); "
                        "dssim = (1 - SSIM) / 2 (1024_example_SSIM.py's `dssim`): of the uint8 images in literal mode, of the unquantised pixels with --mode gradient "
                        "(the quantisation has no gradient; the two agree on uint8-grid images); lbp = the LBP matching distance of "
                        "1024_example_LBP_percept.py, the whole objective of that script (use with --no-lpips; literal mode); msssim = 1 - multi-scale SSIM "
                        "(11-tap Gaussian windows, --msssim-levels levels) of the unquantised pixels, in both modes")
    p.add_argument("--psnr-layout", choices=["script", "aligned"], default="script",
                   help="script = 1024_example_PSNR.py:150-158 as written: the candidate's C-H-W stream against the target's H-W-C stream (different pixels "
                        "are paired); aligned = the PSNR of corresponding pixels (a deviation from the script)")
    p.add_argument("--latent-copies", type=int, default=1,
                   help="projection_example_v2_percept.py:131-166: this many noisy copies of the latent per step, averaged (torch.mean order) before the "
                        "generator (18 there, with --min-loss-init 1.0 --net vgg --no-mse --pool-above 256); literal mode")
    p.add_argument("--min-loss-init", type=float, default=100.0, help="the loop's starting min_loss (100 in the 1024 drivers, 1.0 in the v2 drivers)")
    p.add_argument("--pool-above", type=int, default=0,
                   help="projection_example_v1.py:150-155: block-average generated images taller than this (256 there) by height // N before the "
                        "image-space losses; the target image is then transformed to that size")
    p.add_argument("--batch", type=int, default=32,
                   help="loop steps evaluated per generator forward in literal mode (same result; 32 = the benchmarked configuration, 51 GB of "
                        "activations at 1024^2)")
    p.add_argument("--pipeline", type=int, default=-1, choices=[-1, 0, 1],
                   help="literal mode: score one batch of candidates on a side stream while the generator synthesises the next (same result); -1 = where it pays "
                        "(LPIPS(squeeze) without an embedder: +1.9 %% iterations/s), 0 = never, 1 = always")
    p.add_argument("--keep-images", type=int, default=64,
                   help="device slots for the scored image of every improvement (spilled to the host between launch sequences, so every "
                        "improvement gets its PNG like the reference; raised to --batch if smaller)")
    p.add_argument("--mode", type=str, default="literal", choices=["literal", "gradient"],
                   help="literal = the loop as the reference executes it (best-of-N noisy sampling); gradient = back-propagate the loss "
                        "into the latent and let Adam move it")
    p.add_argument("--mdf", type=str, default=None, metavar="DS_PTH",
                   help="add the MDF discriminator-feature loss of a Ds_*.pth file (mdf-main/weights/Ds_{SISR,Denoising,JPEG}.pth, what --mdfapp "
                        "picks) -- alone, as 1024_example_mdfloss.py scores: --no-lpips --no-mse --min-loss-init 1000; the v1 scripts "
                        "(projection_example_v1_mdfloss*.py) add --pool-above 256 (literal mode); with --mode gradient the loss is differentiated into the "
                        "latent, 1024_example_mdfloss.py's loop without its detach (one target per engine)")
    p.add_argument("--mdf-scales", type=int, default=8, help="discriminators the MDF loss uses (num_scales, default 8)")
    p.add_argument("--mdf-descending", action="store_true", help="use the discriminators from the last one down (is_ascending=0)")
    p.add_argument("--mdf-random", action="store_true", help="seeded random discriminators instead of --mdf (smoke runs only)")


def build_parser():
    ap = argparse.ArgumentParser(prog="morphganformer_amd", description="MI355X latent-projection / GANformer drivers")
    sub = ap.add_subparsers(dest="cmd", required=True)

    g = sub.add_parser("generate", help="Generate images using a pretrained network pickle")
    g.add_argument("--model", type=str, required=True)
    _render_arguments(g, psi="--truncation-psi")
    g.add_argument("--output-dir", type=str, default="images")
    g.add_argument("--images-num", type=int, default=32)
    g.add_argument("--seed", type=int, default=None)

    p = sub.add_parser("project", help="Project one face image into the latent space")
    p.add_argument("--image", type=str, required=True)
    p.add_argument("--landmarks", type=str, default=None)
    p.add_argument("--path_to_gen", type=str, default="images/projection/")
    p.add_argument("--lpips-map", action="store_true",
                   help="also write <path_to_gen>/best_lpips_map.npy / .png: the spatial LPIPS map of the best latent's image against the target")
    p.add_argument("--region-weight", type=str, default=None, metavar="FILE",
                   help="weight the LPIPS and pixel terms by region: a .npy float [H,W] map >= 0, or a gray image scaled to [0,1], at the size the "
                        "image-space losses see")
    p.add_argument("--region-from-landmarks", type=str, default=None, metavar="INSIDE,OUTSIDE[,FEATHER]",
                   help="the region weight from the target row of --landmarks: INSIDE on the landmarks' convex hull, OUTSIDE elsewhere, the edge "
                        "blurred with a Gaussian of FEATHER pixels (drivers.face_region_weight)")
    _loop_arguments(p, align_help="embed candidates and target through the aligned, antialiased 112x112 face crop ArcFace networks are trained on "
                                  "(drivers.arcface_crop of the target row of --landmarks) instead of a resize of the whole frame; iresnetNN / mobilefacenet")

    q = sub.add_parser("morph-pairs", help="Project both images of every CSV pair and render their latent morph "
                                           "(projection_example_v2_percept_morph.py:330-365; BASELINE config 3's outer loop)")
    q.add_argument("--csv", type=str, required=True, help="rows `img1,img2,similarity`; the header row and rows below --threshold are skipped")
    q.add_argument("--threshold", type=float, default=0.5)
    q.add_argument("--src", type=str, required=True, help="directory of the bona fide images")
    q.add_argument("--dst-raw", type=str, required=True, help="<a>_<b>_A.png / _B.png: the two projections")
    q.add_argument("--dst-morph", type=str, required=True, help="<a>_<b>.png: the 0.5 / 0.5 latent morph")
    q.add_argument("--dynamic", action="store_true", help="ranks pull images from a shared work queue instead of images[rank::world]")
    _loop_arguments(q)

    m = sub.add_parser("morph", help="Render linear morphs of two projected latents")
    m.add_argument("--model", type=str, required=True)
    m.add_argument("--w1", type=str, required=True)
    m.add_argument("--w2", type=str, required=True)
    m.add_argument("--alphas", type=str, default="0.5")
    m.add_argument("--out", type=str, required=True, help="output prefix: <out>_a0.50.jpg / .mat")
    _render_arguments(m)
    # `morph --refine`: descend every blend against both contributing images (drivers.refine_morph).  Without --refine none of these is read
    m.add_argument("--refine", action="store_true",
                   help="after blending, descend each blend so that its image matches BOTH subjects (gradient mode with a target pair): "
                        "<out>_a0.50_refined.mat / .png beside the linear morph's files; needs --image-a and --image-b")
    m.add_argument("--image-a", type=str, default=None, help="--refine: the image --w1 was projected from (weighted 1 - alpha)")
    m.add_argument("--image-b", type=str, default=None, help="--refine: the image --w2 was projected from (weighted alpha)")
    m.add_argument("--id-balance", type=float, default=0.0, help="--refine: weight of |d_a - d_b|, the balance of the two identity distances (needs --biometric)")
    m.add_argument("--id-metric", choices=["mse", "cosine"], default="mse",
                   help="--refine: identity distance -- mse = mean squared embedding difference (the projection's term), cosine = 1 - cosine similarity")
    _objective_arguments(m, align_help="--refine: embed both images and every candidate through the aligned face crop (drivers.arcface_crop of the "
                                       "--landmarks rows; a candidate's crop follows the blended landmarks); iresnetNN / mobilefacenet")
    m.add_argument("--pixel-term", choices=["mse", "dssim", "msssim"], default="mse", help="--refine: the pixel term, of the unquantised pixels (see `project`)")
    m.add_argument("--latent-space", choices=["auto", "z", "w+"], default="auto",
                   help="--refine: the space of --w1 / --w2 (auto = by their shape: [1,k,D] is z, [1,k,num_ws,D] is W+)")
    m.add_argument("--no-lockstep", action="store_true", help="--refine: one engine per alpha instead of all alphas in one")
    m.add_argument("--landmarks", type=str, default=None,
                   help="--refine --biometric-align: an .npz with `target` [68,2], the landmarks of --image-a, and `target_b`, those of --image-b")
    m.add_argument("--region-weight", type=str, default=None, metavar="FILE",
                   help="--refine: weight the LPIPS and pixel terms by region (a .npy float [S,S] map >= 0, or a gray image scaled to [0,1])")
    mf = sub.add_parser("merge-files", help="Fold a results tree <src>/<version>/<variant>/<id>/<name>/ over its variants (1024_merge_files.py); no model, no GPU")
    mf.add_argument("--src", type=str, required=True)
    mf.add_argument("--dst", type=str, required=True)
    t = sub.add_parser("morph-tree", help="Morph every latent pair of every id folder (the directory walk of 1024_merge_morph_2.py)")
    t.add_argument("--model", type=str, required=True)
    t.add_argument("--src", type=str, required=True, help="<src>/<id>/<name>/*.mat: two name folders per id")
    t.add_argument("--dst", type=str, required=True, help="<dst>/<id>/<stem1>+<stem2>.jpg / .mat")
    _render_arguments(t)
    w = sub.add_parser("warp", help="Morph two projected latents and warp the morph onto the averaged landmarks (1024_warp_morphs.py)")
    w.add_argument("--model", type=str, required=True)
    w.add_argument("--w1", type=str, required=True, help=".mat latent of the first bona fide image")
    w.add_argument("--w2", type=str, required=True)
    w.add_argument("--landmarks", type=str, required=True,
                   help=".npz with `lm1`, `lm2` [68,2] (detections on the two source images) and `lm_G` [68,2] (on the morph)")
    w.add_argument("--out", type=str, required=True, help="output directory: morph_G.png, Morph_final.png")
    w.add_argument("--truncation_psi", type=float, default=0.7)
    e = sub.add_parser("extract-facenet", help="The FaceNet feature of image files (`facenet_feature`, extract_FaceNet.py:30-40): 224x224 "
                                               "cv2-style resize, (x - 127.5) / 128, InceptionResnetV1 -> 512 numbers per image")
    e.add_argument("images", nargs="+", help="image files")
    e.add_argument("--out", type=str, required=True, help=".mat (scipy.io.savemat: `names`, `features` [N, 512]) or .npy ([N, 512])")
    e.add_argument("--biometric-weights", type=str, default=None, metavar="STATE_DICT",
                   help="facenet_pytorch's InceptionResnetV1 state dict (.pth / .npz) -- what the reference fetches with pretrained='vggface2'")
    e.add_argument("--biometric-random", action="store_true", help="seeded random embedder weights (smoke runs only)")
    lm = sub.add_parser("lpips-map", help="The spatial LPIPS map of two image files (PNetLin(spatial=True)): <out>.npy (float32 [N,N]) and <out>.png "
                                          "(gray, white = --vmax or the map's maximum); no model")
    lm.add_argument("--image-a", type=str, required=True)
    lm.add_argument("--image-b", type=str, required=True)
    lm.add_argument("--out", type=str, required=True, help="output prefix")
    lm.add_argument("--size", type=int, default=1024, help="both images are resized / centre-cropped to this side, like a projection target")
    _lpips_arguments(lm)
    lm.add_argument("--vmax", type=float, default=None, help="the map value drawn white (default: the map's maximum)")
    for name, p in sub.choices.items():
        if COMMANDS[name][1]:                                # every command that opens the GPU pins its device the same way
            p.add_argument("--gpus", type=str, default="0", help="the visible device(s), like the scripts' CUDA_VISIBLE_DEVICES line")
    return ap


def _read_state_dict(path):
    """A weight file -> its state dict (arrays or tensors: embedder.np64 takes both): .npz, or torch.load(weights_only=True) with a `state_dict` level unwrapped."""
    import numpy as np
    import torch
    if str(path).endswith(".npz"):
        return dict(np.load(path))
    state = torch.load(path, map_location="cpu", weights_only=True)
    return state.get("state_dict", state)


def _lpips_term(a, what, spatial=False, device="cuda"):
    """lpips.PerceptualLoss of --net / --lpips-backbone / --lpips-random-backbone; `what` is the command in front of the message."""
    if a.lpips_backbone is None and not a.lpips_random_backbone:
        raise SystemExit(f"{what}: the LPIPS term needs the torchvision backbone weights: --lpips-backbone <state dict> "
                         "(or --no-lpips / --lpips-random-backbone)")
    pool_above = int(getattr(a, "lpips_pool_above", 0) or 0)
    if spatial and pool_above:
        raise SystemExit(f"{what}: --lpips-pool-above with an LPIPS map: the map is defined at the image's own size")
    from .lpips import PerceptualLoss, load_backbone_state
    state = load_backbone_state(a.lpips_backbone) if a.lpips_backbone else None
    if state is None:
        print("WARNING: LPIPS runs on seeded random backbone weights (--lpips-random-backbone); the term is not a perceptual distance")
    return PerceptualLoss(model="net-lin", net=a.net, spatial=spatial, use_gpu=True, device=device, backbone_state=state,
                          allow_random_backbone=state is None, pool_above=pool_above)


def _embedder_state(a, missing, warning):
    """The state dict of --biometric-weights; under --biometric-random None (seeded random weights) after `warning`; neither: SystemExit(missing)."""
    if a.biometric_weights:
        return _read_state_dict(a.biometric_weights)
    if not a.biometric_random:
        raise SystemExit(missing)
    print(warning)


def _biometric_term(a, what, n, device):
    """biometric.BiometricLoss of --biometric / --biometric-weights / --biometric-random for n images per call, or None (--biometric none)."""
    if a.biometric == "none":
        return None
    state = _embedder_state(a, f"{what}: --biometric {a.biometric} needs the embedder's weights: --biometric-weights <state dict> (or --biometric-random)",
                            f"WARNING: the biometric term runs on seeded random {a.biometric} weights (--biometric-random); it is not a face embedding")
    from .biometric import BiometricLoss
    return BiometricLoss(a.biometric, state=state, n=n, device=device)


def _projection_args(a, **loop):
    """projection.ProjectionArgs of the ten options of `_objective_arguments` (+ --ratio, --pixel-term), all `morph --refine` has, plus what the
    caller names: morph's --truncation_psi is the rendering psi of the linear morph, not a loop argument, so nothing is collected by matching names."""
    from .projection import ProjectionArgs
    return ProjectionArgs(step=a.step, lamda=a.lamda, beta=a.beta, lr=a.lr, noise=a.noise, n_mean_latent=a.n_mean_latent, ratio=a.ratio,
                          percept_weight=a.percept_weight, pixel_term=a.pixel_term, msssim_levels=a.msssim_levels, **loop)


def mdf_options(a):
    """MDFLoss keyword arguments of the parsed command line: gradient mode builds the loss with its backward pass."""
    return dict(num_scales=a.mdf_scales, is_ascending=0 if a.mdf_descending else 1, differentiable=a.mode == "gradient")


def region_arguments(a):
    """Checks of `project`'s two region options (before anything is loaded) -> None, ("file", path) or ("landmarks", inside, outside, feather)."""
    if a.cmd != "project" or (a.region_weight is None and a.region_from_landmarks is None):
        return None
    if a.region_weight is not None and a.region_from_landmarks is not None:
        raise SystemExit("project: --region-weight and --region-from-landmarks both define the region weight: pass one of them")
    if a.region_weight is not None:
        return ("file", a.region_weight)
    if not a.landmarks:
        raise SystemExit("project: --region-from-landmarks takes the hull of the target's landmarks: it needs --landmarks")
    try:
        vals = [float(v) for v in a.region_from_landmarks.split(",")]
    except ValueError:
        vals = []
    if len(vals) not in (2, 3) or min(vals) < 0 or max(vals[:2]) <= 0:
        raise SystemExit(f"project: --region-from-landmarks takes INSIDE,OUTSIDE[,FEATHER], all >= 0 and not both weights zero (got {a.region_from_landmarks!r})")
    return ("landmarks", vals[0], vals[1], vals[2] if len(vals) == 3 else 0.0)


def align_arguments(a):
    """Checks of --biometric-align (before anything is loaded) -> True when the biometric term embeds through the aligned face crop."""
    if not getattr(a, "biometric_align", False):
        return False
    what = "morph --refine" if a.cmd == "morph" else a.cmd
    if a.cmd == "morph" and not a.refine:
        raise SystemExit("morph: --biometric-align belongs to --refine")
    if a.biometric == "none":
        raise SystemExit(f"{what}: --biometric-align aligns the input of the biometric term: it needs --biometric iresnetNN or mobilefacenet")
    if a.biometric == "facenet":
        raise SystemExit(f"{what}: --biometric-align is the crop of the ArcFace embedders (iresnetNN, mobilefacenet); facenet scores the "
                         "un-cropped frame by the reference's definition")
    if not a.landmarks:
        raise SystemExit(f"{what}: --biometric-align takes the crop from the target's landmarks: it needs --landmarks")
    if not os.path.isfile(a.landmarks):
        raise SystemExit(f"{what}: --biometric-align: the landmark file {a.landmarks} does not exist")
    return True


def _merge_files(a):
    from . import drivers
    files = drivers.merge_files(a.src, a.dst)
    print(f"copied {len(files)} files")


def _lpips_map(a):
    from . import drivers
    percept = _lpips_term(a, a.cmd, spatial=True)
    img_a = drivers.image_transform(a.image_a, size=a.size, device="cuda")
    img_b = drivers.image_transform(a.image_b, size=a.size, device="cuda")
    m = drivers.lpips_map(percept, img_a, img_b)
    for path in drivers.save_lpips_map(m, a.out, vmax=a.vmax):
        print(path)
    print(f"mean {float(m.mean()):.6f}  max {float(m.max()):.6f}")


def _extract_facenet(a):
    import numpy as np
    from PIL import Image
    from . import drivers
    from .facenet import InceptionResnetV1Embedder, random_state
    state = _embedder_state(a, "extract-facenet: the embedder's weights are needed: --biometric-weights <state dict> (or --biometric-random)",
                            "WARNING: seeded random InceptionResnetV1 weights (--biometric-random); the output is not a face embedding")
    net = InceptionResnetV1Embedder(random_state(0) if state is None else state, n=1, device="cuda")
    feats = [drivers.facenet_feature(np.asarray(Image.open(f).convert("RGB")), net) for f in a.images]
    feats = np.stack(feats).astype(np.float32)
    if a.out.endswith(".npy"):
        np.save(a.out, feats)
    else:
        import scipy.io as sio
        sio.savemat(a.out, {"names": np.array(a.images, dtype=object), "features": feats})
    print(f"{len(a.images)} feature(s) -> {a.out}")


def _generate(a, G):
    from . import drivers
    print("Generate and save images...")
    drivers.generate_images(G, a.images_num, a.truncation_psi, a.output_dir, a.ratio, seed=a.seed)


def _morph_tree(a, G):
    from . import drivers
    for stem in drivers.merge_morph_tree(G, a.src, a.dst, a.truncation_psi, a.ratio):
        print(stem)


def _warp(a, G):
    import numpy as np
    from . import drivers
    lm = np.load(a.landmarks)
    drivers.warp_morphs(G, drivers.load_latent_mat(a.w1), drivers.load_latent_mat(a.w2), lm["lm1"], lm["lm2"], landmark_G=lm["lm_G"],
                        out_dir=a.out, truncation_psi=a.truncation_psi)
    print("done")


def _morph(a, G):
    from . import drivers
    alphas = [float(v) for v in a.alphas.split(",")]
    if a.refine and (a.image_a is None or a.image_b is None):
        raise SystemExit("morph --refine needs the two contributing images: --image-a and --image-b")
    drivers.merge_morph(G, drivers.load_latent_mat(a.w1), drivers.load_latent_mat(a.w2), alphas, a.truncation_psi,
                        out_prefix=a.out, ratio=a.ratio)
    if a.refine:
        _refine(a, G, alphas)


def _refine(a, G, alphas):
    """`morph --refine` (drivers.refine_morph on the command line's objective)."""
    import numpy as np
    from . import drivers
    what = "morph --refine"
    w1, w2 = drivers.load_latent_mat(a.w1), drivers.load_latent_mat(a.w2)
    space = "w+" if w1.ndim == 4 else "z"
    if a.latent_space not in ("auto", space):
        raise SystemExit(f"{what}: --latent-space {a.latent_space} but {a.w1} holds a {space} latent {w1.shape}")
    args = _projection_args(a)
    percept = None if a.no_lpips else _lpips_term(a, what, device=G.device)
    biometric = _biometric_term(a, what, n=1 if a.no_lockstep else len(alphas), device=G.device)
    if biometric is None and a.id_balance != 0.0:
        raise SystemExit(f"{what}: --id-balance weighs the two identity distances: it needs --biometric")
    if percept is None and a.no_mse and biometric is None:
        raise SystemExit(f"{what}: every term of the objective is switched off")
    crop_kw = {}
    if a.biometric_align:                # (checked by align_arguments before anything was loaded)
        lm = np.load(a.landmarks)
        if "target" not in lm or "target_b" not in lm:
            raise SystemExit(f"{what}: --biometric-align needs the rows `target` and `target_b` in {a.landmarks} (found {sorted(lm.keys())})")
        crop_kw = dict(face_crop=drivers.arcface_crop(lm["target"]), face_crop_b=drivers.arcface_crop(lm["target_b"]),
                       face_crop_filter=a.biometric_crop_filter)
    ta = drivers.image_transform(a.image_a, size=a.size, device=G.device)
    tb = drivers.image_transform(a.image_b, size=a.size, device=G.device)
    res = drivers.refine_morph(G, w1, w2, ta, tb, alphas, lockstep=not a.no_lockstep, args=args, percept=percept, biometric=biometric,
                               gamma=a.gamma, id_balance=a.id_balance, id_metric=a.id_metric, seed=a.seed, use_mse=not a.no_mse,
                               out_prefix=a.out, ratio=a.ratio, **crop_kw,
                               region_weight=None if a.region_weight is None else drivers.load_region_weight(a.region_weight))
    for r in res:
        ids = "" if r["id_distances"] is None else "  d_a {:.6f}  d_b {:.6f}".format(*r["id_distances"])
        print(f"alpha {r['alpha']:.2f}: best step {r['best_step']}  loss {r['best_loss']:.6f} (start {r['losses'][0]:.6f}){ids}")


def _loop_objective(a, G):
    """What `project` and `morph-pairs` share: the command line's objective and its checks -> the keyword arguments both hand to drivers.project_image."""
    args = _projection_args(a, lr_rampup=a.lr_rampup, lr_rampdown=a.lr_rampdown, noise_ramp=a.noise_ramp, truncation_psi=a.truncation_psi,
                            psnr_layout=a.psnr_layout, pool_above=a.pool_above, latent_copies=a.latent_copies, min_loss_init=a.min_loss_init,
                            noise_regularize=a.noise_regularize)
    lpips_map = bool(getattr(a, "lpips_map", False))
    if a.no_lpips and lpips_map:
        raise SystemExit(f"{a.cmd}: --lpips-map is the map of the LPIPS term: drop --no-lpips")
    percept = None if a.no_lpips else _lpips_term(a, a.cmd, spatial=lpips_map, device=G.device)
    biometric = _biometric_term(a, a.cmd, n=a.batch if a.mode == "literal" else 1, device=G.device)
    mdf = None
    if a.mdf or a.mdf_random:
        from .mdf import MDFLoss, random_discriminators
        if a.mdf_random:
            print("WARNING: the MDF term runs on seeded random discriminators (--mdf-random); it is not the trained loss")
        mdf = MDFLoss(random_discriminators(0) if a.mdf_random else a.mdf, device=G.device, **mdf_options(a))
    if percept is None and a.no_mse and biometric is None and mdf is None and not getattr(a, "landmarks", None) and a.pixel_term != "lbp":
        raise SystemExit(f"{a.cmd}: every term of the objective is switched off")
    if a.pixel_term == "lbp" and (a.cmd != "project" or a.mode != "literal"):
        raise SystemExit("--pixel-term lbp is the objective of the single-image literal loop (project --mode literal)")
    if a.optimize_noise and (a.cmd != "project" or a.mode != "gradient"):
        raise SystemExit("--optimize-noise is for project --mode gradient (one target; the literal loop never back-propagates)")
    return dict(args=args, percept=percept, batch=a.batch, seed=a.seed, mode=a.mode, latent_space="w+" if (a.w_plus and a.mode == "gradient") else "z",
                keep_images=a.keep_images, pipeline=None if a.pipeline < 0 else (bool(a.pipeline) and a.mode == "literal"),
                biometric=biometric, gamma=a.gamma, use_mse=not a.no_mse, mdf=mdf)


def _morph_pairs(a, G):
    """One process per GPU under `python -m torch.distributed.run --nproc-per-node N -m morphganformer_amd.cli morph-pairs ...`: the
    2 x pairs projections are sharded over the ranks, one all_gather returns the latents, the renderings are dealt pairs[rank::world]."""
    import torch
    import torch.distributed as dist
    from . import drivers
    kw = _loop_objective(a, G)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and not dist.is_initialized():
        from .distributed import init_process_group
        init_process_group("nccl", device_id=torch.device("cuda", torch.cuda.current_device()))
    if a.mode == "literal":
        kw["dynamic"] = a.dynamic
    res = drivers.morph_pairs(G, drivers.read_pair_csv(a.csv, a.threshold), a.src, a.dst_raw, a.dst_morph,
                              truncation_psi=a.truncation_psi, ratio=a.ratio, **kw)
    for path in res["written"]:
        print(path)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def _project(a, G):
    import numpy as np
    from . import drivers
    region, align = region_arguments(a), align_arguments(a)
    kw = _loop_objective(a, G)
    args = kw["args"]
    tsize = a.size // args.pool_factor(a.size)           # the size the image-space losses see
    target = drivers.image_transform(a.image, size=tsize, device=G.device)
    lm_t = lm_s = None
    if a.landmarks:
        lm = np.load(a.landmarks)
        lm_t, lm_s = lm["target"], lm["steps"]
        if lm_s.shape[0] < a.step:
            raise SystemExit(f"--landmarks holds {lm_s.shape[0]} steps, --step is {a.step}")
    region_weight = None
    if region is not None and region[0] == "file":
        region_weight = drivers.load_region_weight(region[1])
    elif region is not None:           # the landmarks are in the pixels of the --size image; the weight is at the size the losses see
        region_weight = drivers.face_region_weight(np.asarray(lm_t, dtype=np.float64) * (tsize / a.size), tsize, *region[1:])
    stem = os.path.splitext(os.path.basename(a.image))[0]
    lbp_target = None
    if a.pixel_term == "lbp":          # LBP_feature(path): the file's own pixels (1024_example_LBP_percept.py:40-45,140); min_distance starts at 1 (:151)
        from PIL import Image
        from . import lbp
        lbp_target = lbp.target_feature(np.asarray(Image.open(a.image).convert("RGB")), G.device)
        args.min_loss_init = 1.0
    res = drivers.project_image(G, target, lm_t, lm_s, out_prefix=os.path.join(a.path_to_gen, stem), path_to_gen=a.path_to_gen,
                                lbp_target=lbp_target, optimize_noise=a.optimize_noise, noise_init=a.noise_init, lpips_map=a.lpips_map,
                                region_weight=region_weight, **(dict(face_crop="landmarks", face_crop_filter=a.biometric_crop_filter) if align else {}), **kw)
    print(f"best step {res['step']}  loss {res['loss']:.6f}")


# subcommand -> (handler, what main() opens for it); a handler raises or is done.  None: file bookkeeping (1024_merge_files.py), answered before
# the environment is touched; "gpu": the device; "generator": the device and the network of --model, the handler's second argument
COMMANDS = {"merge-files": (_merge_files, None), "extract-facenet": (_extract_facenet, "gpu"), "lpips-map": (_lpips_map, "gpu"),
            "generate": (_generate, "generator"), "morph-tree": (_morph_tree, "generator"), "warp": (_warp, "generator"),
            "morph": (_morph, "generator"), "morph-pairs": (_morph_pairs, "generator"), "project": (_project, "generator")}


def main(argv=None):
    a = build_parser().parse_args(argv)
    region_arguments(a)                                       # the checks of the command line run before anything is loaded
    align_arguments(a)
    handler, opens = COMMANDS[a.cmd]
    if opens:
        launched = int(os.environ.get("WORLD_SIZE", "1")) > 1 and "LOCAL_RANK" in os.environ
        # read by the HSA runtime when it starts, i.e. at the first GPU call (loader.load_network below): set here, before torch is imported,
        # like bench.py does -- the host driver only supports dmabuf IPC, RCCL fails without it
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if not launched:
            os.environ.setdefault("CUDA_VISIBLE_DEVICES", a.gpus)
        import torch
        if launched:                                          # one process per GPU (torch.distributed.run): rank r works on device LOCAL_RANK
            torch.cuda.set_device(int(os.environ["LOCAL_RANK"]))
    if opens == "generator":
        from . import loader
        print("Loading networks...")
        handler(a, loader.load_network(a.model, device="cuda")["Gs"])
    else:
        handler(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
