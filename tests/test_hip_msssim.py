"""The multi-scale SSIM pixel term on the GPU: mgf_msssim_f32 / mgf_msssim_grad_f32 (csrc/msssim.hip) against float64 torch autograd through
tests/msssim_torch_ref.py (pinned by tests/test_msssim_ref.py), and both projection engines with pixel_term="msssim" -- the gradient loop against
autograd + Adam through the CPU restatement of the generator, test by test like tests/test_hip_dssim_gradient.py and with its gates.

Kernel tolerances are DSSIM's, for the same reason -- float64 arithmetic with float32 stores, the only roundings being the store and, when
accumulating, the add: value |got - want| <= 1e-6 |want|; gradient |got - want| <= 2 * 2^-23 (|want| + |prior|) per element + 1e-9 max |want|
for the reordered float64 sums.

The images of the kernel tests are CORRELATED (target = clamp(img + 0.3 randn)): independent random images put every small shape on the
clamped branch (some level mean <= 0, loss exactly 1, gradient 0) and the comparison would be of zeros.  Each case asserts on the reference that
its smallest level mean is > 0.5; that is a condition of the test, not a tolerance."""
import ctypes
import os

import numpy as np
import pytest
import torch

from msssim_torch_ref import level_means, msssim_torch, msssim_torch_grad, msssim_weights

pytestmark = pytest.mark.gpu

# (n, c, h, w, levels): one window position; an odd side (23 -> 12); odd sides with the coarsest side exactly 11; 64^2; odd sides at two levels and
# sides that are no multiple of the tile; the smallest five-level image (161 -> 81 -> 41 -> 21 -> 11); the workload's size
SHAPES = [(2, 3, 11, 11, 1), (1, 3, 23, 44, 2), (2, 3, 33, 21, 2), (1, 3, 64, 64, 3), (3, 1, 45, 97, 3), (2, 3, 161, 176, 5), (1, 3, 1024, 1024, 5)]


def _weights(levels, weights=None):
    w = msssim_weights(levels) if weights is None else list(weights)
    return (ctypes.c_double * len(w))(*w)


def _scratch(n, c, h, w, levels):
    from morphganformer_amd import _lib
    nbytes = int(_lib.lib().mgf_msssim_scratch_bytes(n, c, h, w, levels))
    assert nbytes > 0, (n, c, h, w, levels)
    return torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")


def _value(img, tgt, levels, scale=1.0, prior=None):
    from morphganformer_amd import _lib
    n, c, h, w = img.shape
    out = torch.full([n], float("nan"), device="cuda") if prior is None else prior.clone()
    scratch, wts = _scratch(n, c, h, w, levels), _weights(levels)
    _lib.check(_lib.lib().mgf_msssim_f32(out.data_ptr(), img.data_ptr(), tgt.data_ptr(), n, c, h, w, 0 if tgt.ndim == 3 else c * h * w,
                                         ctypes.addressof(wts), levels, 255.0, scale, 0 if prior is None else 1, scratch.data_ptr(),
                                         _lib.stream_ptr()), "msssim")
    torch.cuda.synchronize()
    return out


def _grad(img, tgt, levels, scale=1.0, prior=None, with_out=True, out_prior=None):
    from morphganformer_amd import _lib
    n, c, h, w = img.shape
    dimg = torch.full_like(img, float("nan")) if prior is None else prior.clone()
    out = None if not with_out else (torch.full([n], float("nan"), device="cuda") if out_prior is None else out_prior.clone())
    scratch, wts = _scratch(n, c, h, w, levels), _weights(levels)
    _lib.check(_lib.lib().mgf_msssim_grad_f32(dimg.data_ptr(), _lib.ptr(out), img.data_ptr(), tgt.data_ptr(), n, c, h, w,
                                              0 if tgt.ndim == 3 else c * h * w, ctypes.addressof(wts), levels, 255.0, scale,
                                              0 if prior is None else 1, 0 if out_prior is None else 1, scratch.data_ptr(), _lib.stream_ptr()),
               "msssim_grad")
    torch.cuda.synchronize()
    return dimg, out


def _check_grad(tag, got, want, prior=None):
    got, want = got.double().cpu(), want.double().cpu()
    pr = torch.zeros_like(want) if prior is None else prior.double().cpu()
    bound = 2 * 2.0 ** -23 * (want.abs() + pr.abs()) + 1e-9 * float(want.abs().max())
    err = (got - (want + pr)).abs()
    worst = float((err / bound).max())
    print(f"OBS {tag}: gradient max err/bound {worst:.3f}, max |want| {float(want.abs().max()):.3e}")
    assert torch.isfinite(got).all() and worst <= 1.0, (tag, worst)


def _check_value(tag, got, want):
    got, want = got.double().cpu().numpy(), np.asarray(want, np.float64)
    rel = np.abs(got - want) / np.abs(want)
    print(f"OBS {tag}: value {got.tolist()} want {want.tolist()} max rel {rel.max():.3e}")
    assert (np.abs(got - want) <= 1e-6 * np.abs(want)).all(), (tag, got, want)


def _correlated(shape, seed):
    g = torch.Generator().manual_seed(seed)
    img = 0.7 * torch.randn(shape, generator=g)                             # |x| > 1 in places: the generator's output is unclamped
    tgt = (img + 0.3 * torch.randn(shape, generator=g)).clamp(-1, 1)
    return img, tgt, g


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_msssim_kernels_vs_autograd(shape):
    """Value and gradient against float64 autograd: a shared target and per-sample targets, writing and accumulating onto a random prior,
    scale != 1, out = NULL, the accumulated unscaled out; the value of the gradient call is the value call's, bit for bit, and a second call
    gives the same bits.  (The 1024^2 case takes the shared target only: one reference evaluation of that size.)"""
    n, c, h, w, levels = shape
    own, tgts, g = _correlated(shape[:4], h * 1009 + w)
    big = h * w >= 1 << 20
    prior = torch.randn(shape[:4], generator=g) * (1e-6 if big else 1e-4)   # about the size of the gradient: the add's rounding counts
    near = own.clone()                                                      # a SHARED target must correlate with every sample: the further
    near[1:] = own[0] + 0.2 * torch.randn((n - 1, c, h, w), generator=g)    # samples are the first one plus noise of their own
    for shared in ((True,) if big else (True, False)):
        tgt = tgts[0].contiguous() if shared else tgts
        img = near if shared else own
        tag = f"{shape} {'shared' if shared else 'per-sample'}"
        vmin = float(level_means(img, tgt, levels).min())
        assert vmin > 0.5, (tag, vmin)                                      # off the clamped branch, by a distance
        v_ref, g_ref = msssim_torch_grad(img, tgt, levels)
        d_img, d_tgt = img.cuda(), tgt.cuda()
        val = _value(d_img, d_tgt, levels)
        _check_value(tag, val, v_ref.numpy())
        dimg, out = _grad(d_img, d_tgt, levels)
        _check_grad(tag + " write", dimg, g_ref)
        assert torch.equal(out, val), (tag, out, val)                       # the gradient call's value: the same bits
        dimg2, out2 = _grad(d_img, d_tgt, levels)
        assert torch.equal(dimg, dimg2) and torch.equal(out, out2), tag      # same inputs, same bits
        assert torch.equal(_value(d_img, d_tgt, levels), val)
        dimg_only, none = _grad(d_img, d_tgt, levels, with_out=False)       # out may be NULL
        assert none is None and torch.equal(dimg_only, dimg)
        scale = 0.37
        dacc, oacc = _grad(d_img, d_tgt, levels, scale=scale, prior=prior.cuda(), out_prior=torch.full([n], 2.0, device="cuda"))
        _check_grad(tag + " scale 0.37, accumulate", dacc, scale * g_ref, prior)
        _check_value(tag + " accumulated out (unscaled)", oacc, 2.0 + v_ref.numpy())
        _check_grad(tag + " scale -2.5", _grad(d_img, d_tgt, levels, scale=-2.5)[0], -2.5 * g_ref)
        _check_value(tag + " value scale 0.5 onto 2", _value(d_img, d_tgt, levels, scale=0.5, prior=torch.full([n], 2.0, device="cuda")),
                     2.0 + 0.5 * v_ref.numpy())


def test_msssim_gradient_of_a_smooth_image():
    """A smooth image with 1 % noise -- what a projection target looks like -- where exx - ux^2 cancels (the cancellation case of the DSSIM test)."""
    shape = (1, 3, 128, 128)
    g = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 128), torch.linspace(0, 1, 128), indexing="ij")
    base = torch.stack([0.8 * torch.sin(3 * xx + 2 * yy), 0.6 * torch.cos(4 * yy - xx), 0.9 * xx * yy - 0.2])[None]
    tgt = (base + 0.01 * torch.randn(shape, generator=g))[0].contiguous()
    img = base + 0.01 * torch.randn(shape, generator=g)
    assert float(level_means(img, tgt, 4).min()) > 0.5
    v_ref, g_ref = msssim_torch_grad(img, tgt, 4)
    dimg, out = _grad(img.cuda(), tgt.cuda(), 4)
    _check_value("smooth", out, v_ref.numpy())
    _check_grad("smooth", dimg, g_ref)


def test_msssim_of_identical_images_is_zero_with_no_gradient():
    shape = (2, 3, 70, 45)
    g = torch.Generator().manual_seed(11)
    img = torch.randn(shape, generator=g) * 0.7
    dimg, out = _grad(img.cuda(), img.cuda(), 3)
    assert torch.equal(out, torch.zeros(2, device="cuda")), out
    assert torch.equal(_value(img.cuda(), img.cuda(), 3), torch.zeros(2, device="cuda"))
    pert, _ = _grad((img + 0.05 * torch.randn(shape, generator=g)).cuda(), img.cuda(), 3)
    ratio = float(dimg.abs().max() / pert.abs().max())
    print(f"OBS identical images: max |gradient| {float(dimg.abs().max()):.3e}, on a perturbed image {float(pert.abs().max()):.3e}, ratio {ratio:.3e}")
    assert ratio < 1e-12


def test_msssim_clamped_branch_is_one_with_a_zero_gradient():
    """Some level mean <= 0: ms = 0 and the gradient is DEFINED as zero (the libraries' relu-then-power gives 0 * inf = NaN there).  img = -target
    puts every channel there; one anticorrelated channel beside two correlated ones zeroes that plane only."""
    shape = (2, 3, 64, 64)
    img, tgt, g = _correlated(shape, 17)
    d_img = img.cuda()
    assert float(level_means(img, -img, 3).max()) < 0
    dimg, out = _grad(d_img, (-img).cuda(), 3)
    assert torch.equal(out, torch.ones(2, device="cuda")), out
    assert torch.equal(dimg, torch.zeros_like(dimg))
    assert torch.equal(_value(d_img, (-img).cuda(), 3), torch.ones(2, device="cuda"))
    prior = torch.randn(shape, generator=g).cuda()
    dacc, _ = _grad(d_img, (-img).cuda(), 3, scale=0.37, prior=prior)
    assert torch.equal(dacc, prior)                                         # accumulated: the prior, unchanged
    mixed = tgt.clone()
    mixed[:, 1] = -img[:, 1]
    v = level_means(img, mixed, 3)
    assert float(v[:, 1].min()) < 0 and float(v[:, [0, 2]].min()) > 0.5
    v_ref, g_ref = msssim_torch_grad(img, mixed, 3)
    assert torch.equal(g_ref[:, 1], torch.zeros_like(g_ref[:, 1])) and float(g_ref.abs().max()) > 0
    dimg, out = _grad(d_img, mixed.cuda(), 3)
    assert torch.equal(dimg[:, 1], torch.zeros_like(dimg[:, 1]))
    _check_value("one clamped channel", out, v_ref.numpy())
    _check_grad("one clamped channel", dimg, g_ref)


def test_msssim_refuses_more_levels_than_the_image_allows():
    from morphganformer_amd import _lib
    img = torch.zeros(1, 3, 64, 64, device="cuda")
    out, wts = torch.zeros(1, device="cuda"), _weights(4)
    assert int(_lib.lib().mgf_msssim_scratch_bytes(1, 3, 64, 64, 4)) == 0 and int(_lib.lib().mgf_msssim_scratch_bytes(1, 3, 64, 64, 6)) == 0
    scratch = _scratch(1, 3, 64, 64, 3)
    rc = _lib.lib().mgf_msssim_f32(out.data_ptr(), img.data_ptr(), img.data_ptr(), 1, 3, 64, 64, 0, ctypes.addressof(wts), 4, 255.0, 1.0, 0,
                                   scratch.data_ptr(), _lib.stream_ptr())
    assert rc == -1                                                         # MGF_EINVAL
    with pytest.raises(_lib.MgfError, match=r"level 3 .*8x8"):
        _lib.check(rc, "msssim")
    rc = _lib.lib().mgf_msssim_grad_f32(img.data_ptr(), out.data_ptr(), img.data_ptr(), img.data_ptr(), 1, 3, 64, 64, 0, ctypes.addressof(wts), 6,
                                        255.0, 1.0, 0, 0, scratch.data_ptr(), _lib.stream_ptr())
    with pytest.raises(_lib.MgfError, match=r"levels must lie in 1\.\.5"):
        _lib.check(rc, "msssim_grad")


def test_msssim_weights_travel_by_value():
    """Explicit weights of the C ABI (not the Python defaults), and: the host array may change after the call was issued."""
    from morphganformer_amd import _lib
    shape = (1, 3, 45, 97)
    img, tgt, _ = _correlated(shape, 29)
    wts = [0.5, 0.2, 0.3]
    v_ref, g_ref = msssim_torch_grad(img, tgt[0], 3, weights=wts)
    d_img, d_tgt = img.cuda(), tgt[0].contiguous().cuda()
    arr = _weights(3, wts)
    dimg, out = torch.empty_like(d_img), torch.empty(1, device="cuda")
    scratch = _scratch(1, 3, 45, 97, 3)
    _lib.check(_lib.lib().mgf_msssim_grad_f32(dimg.data_ptr(), out.data_ptr(), d_img.data_ptr(), d_tgt.data_ptr(), 1, 3, 45, 97, 0, ctypes.addressof(arr),
                                              3, 255.0, 1.0, 0, 0, scratch.data_ptr(), _lib.stream_ptr()), "msssim_grad")
    arr[0], arr[1], arr[2] = 0.0, 0.0, 1.0
    torch.cuda.synchronize()
    _check_value("explicit weights", out, v_ref.numpy())
    _check_grad("explicit weights", dimg, g_ref)


# ---------------------------------------------------------------------------------------------------------------- the projection loops
LEVELS = 3                                                                  # what a 64 x 64 image allows


@pytest.fixture(scope="module")
def tiny():
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import TINY, make_state_dict
    from oracle.generator_ref import to_torch_state
    sd = make_state_dict(TINY, seed=0)
    return Generator(sd, TINY, "cuda", max_batch=3), to_torch_state(sd), TINY


def _squeeze_lins():
    from morphganformer_amd.lpips import WEIGHTS_DIR
    lin = np.load(os.path.join(WEIGHTS_DIR, "lpips_lin_squeeze.npz"))
    return [torch.from_numpy(lin[f"lin{i}"]).float().reshape(-1) for i in range(7)]


def loop_inputs(tsd, cfg, steps=10):
    """Target, start latent and noise stream of the loop tests.  The start is the target's own latent plus 0.3 N(0, 1): the tiny generator's
    images of unrelated latents are uncorrelated, which would put the run on the clamped branch (gradient zero); from this start every level
    mean of the oracle's run stays positive (asserted by the tests)."""
    from morphganformer_amd.synth_weights import synthetic_latents
    from oracle.generator_ref import generator_ref
    rng = np.random.Generator(np.random.PCG64(4))
    zt = torch.from_numpy(synthetic_latents(cfg, 1, 1001))
    target = generator_ref(tsd, zt, cfg, "const").clamp(-1, 1).detach()
    latent_mean = zt[0] + 0.3 * torch.from_numpy(rng.standard_normal((cfg.k, cfg.z_dim)).astype(np.float32))
    eps = torch.from_numpy(rng.standard_normal((steps, 1, cfg.k, cfg.z_dim)).astype(np.float32))
    return target, latent_mean, eps


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("terms", ["lpips+wing+msssim", "msssim"])
def test_gradient_projection_with_msssim_matches_autograd_adam(tiny, use_graph, terms):
    """The gradient-mode loop against torch autograd + torch.optim.Adam through the CPU oracle (the gates of
    test_hip_dssim_gradient.py::test_gradient_projection_with_dssim_matches_autograd_adam): LPIPS + lamda Wing + beta MS-SSIM with a skipped
    ("no face") step, and MS-SSIM as the ONLY term -- there the latent moves on this gradient alone."""
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, synthetic_landmarks
    from oracle.generator_ref import generator_ref
    from oracle.loss_ref import backbone_random, lpips_ref, projection_gradient_ref, wing_loss_ref
    G, tsd, cfg = tiny
    full = terms != "msssim"
    steps = 10
    target, latent_mean, eps = loop_inputs(tsd, cfg, steps)
    lm_t, lm_s = synthetic_landmarks(steps, 64, 9)
    valid = np.ones(steps, np.int32)
    if full:
        valid[3] = 0
    # beta: d msssim / d latent is about 1/7 of d MSE / d latent on these images (max |gradient| 0.55 against 3.8 at step 0, measured through the
    # CPU oracle), so beta = 6 gives the pixel term the share of the gradient that it has in the test this one is modelled on (DSSIM: 1/110 and
    # beta = 100; see the comment there on why that share matters beside the random-backbone LPIPS gradient).  The run on MS-SSIM alone takes 0.8.
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.2, pixel_term="msssim", msssim_levels=LEVELS, beta=6.0 if full else 0.8, min_loss_init=1e4)
    bb, lins = backbone_random("squeeze", 0), _squeeze_lins()
    vmins = []

    def loss_fn(i, img):
        if not valid[i]:
            return None
        vmins.append(float(level_means(img.detach(), target[0], LEVELS).min()))
        d = args.beta * msssim_torch(img, target[0], LEVELS)[0]
        if not full:
            return d
        return lpips_ref(bb, lins, img, target).sum() + args.lamda * wing_loss_ref(torch.from_numpy(lm_s[i]), torch.from_numpy(lm_t)) + d

    ref = projection_gradient_ref(lambda z: generator_ref(tsd, z, cfg, "const"), loss_fn, latent_mean, 1.0, eps, steps, lr=args.lr,
                                  rampdown=args.lr_rampdown, rampup=args.lr_rampup, min_loss_init=args.min_loss_init)
    assert min(vmins) > 0.02, vmins                                         # the whole run off the clamped branch (a condition, not a tolerance)
    kw = dict(percept=PerceptualLoss(net="squeeze", allow_random_backbone=True), lm_target=lm_t, lm_steps=lm_s, lm_valid=valid) if full else dict(percept=None)
    eng = GradientProjectionEngine(G, target.cuda(), latent_mean.cuda(), 1.0, args, eps=eps.cuda(), noise_mode="const", use_graph=use_graph, **kw)
    traj = []
    for i in range(steps):
        eng.run(1)
        traj.append(eng.latent_in.cpu().clone())
    lat, bstep, bloss, losses = eng.result()
    moved = float((ref[4][-1] - latent_mean).abs().max())
    assert moved > 5 * args.lr * 0.2, "the oracle run must actually move the latent"
    got = np.array([v for v in losses if not np.isnan(v)])
    want = np.array([v for v in ref[3] if v is not None])
    print(f"OBS loop {terms} graph={use_graph}: losses max rel {np.abs(got - want).max() / np.abs(want).max():.3e}, trajectory max diff / (lr (i + 1)) "
          f"{max(float((traj[i] - ref[4][i]).abs().max()) / (args.lr * (i + 1)) for i in range(steps)):.3e}, moved {moved:.3f}, "
          f"smallest level mean {min(vmins):.3f}")
    for i in range(steps):
        assert float((traj[i] - ref[4][i]).abs().max()) < 0.05 * args.lr * (i + 1), i
    if full:
        assert np.isnan(losses[3]) and ref[3][3] is None
    assert np.abs(got - want).max() < 1e-3 * np.abs(want).max()
    assert bstep == ref[1]
    assert float((lat - ref[0]).abs().max()) < 0.05 * args.lr * steps


def wplus_inputs(tsd, cfg, steps=8):
    """W+ start, scale, noise stream and a target rendered from a ws near the start (see loop_inputs on why near).  The per-slot noise of a W+
    search decorrelates the tiny generator's images all the same: the oracle's first steps run with one channel on the clamped branch (level
    mean about -0.03) before every mean turns positive; the test asserts that no level mean comes within 0.01 of the branch point."""
    from morphganformer_amd.synth_weights import synthetic_latents
    from oracle.generator_ref import mapping_ref, synthesis_ref
    rng = np.random.Generator(np.random.PCG64(14))
    w_mean = mapping_ref(tsd, torch.from_numpy(synthetic_latents(cfg, 1, 77)), cfg)[0].detach()
    eps = torch.from_numpy(rng.standard_normal((steps, 1, cfg.k, cfg.num_ws, cfg.w_dim)).astype(np.float32))
    w_std = float(w_mean.std())
    start = w_mean[:, None, :].expand(cfg.k, cfg.num_ws, cfg.w_dim).contiguous()
    off = torch.from_numpy(rng.standard_normal((cfg.k, 1, cfg.w_dim)).astype(np.float32))
    target = synthesis_ref(tsd, (start + 0.5 * float(w_mean.std()) * off)[None], cfg, "const").clamp(-1, 1).detach()
    return w_mean, w_std, start, eps, target


def test_wplus_gradient_projection_with_msssim_matches_autograd_adam(tiny):
    """latent_space="w+" with LPIPS + beta MS-SSIM against autograd + Adam on ws through the CPU restatement's synthesis network (the gates of
    test_hip_dssim_gradient.py::test_wplus_gradient_projection_with_dssim_matches_autograd_adam)."""
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    from oracle.generator_ref import synthesis_ref
    from oracle.loss_ref import backbone_random, lpips_ref, projection_gradient_ref
    G, tsd, cfg = tiny
    steps = 8
    w_mean, w_std, start, eps, target = wplus_inputs(tsd, cfg, steps)
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.2, pixel_term="msssim", msssim_levels=LEVELS)
    bb, lins = backbone_random("squeeze", 0), _squeeze_lins()
    vabs = []

    def loss_fn(i, img):
        vabs.append(float(level_means(img.detach(), target[0], LEVELS).abs().min()))
        return lpips_ref(bb, lins, img, target).sum() + args.beta * msssim_torch(img, target[0], LEVELS)[0]

    ref = projection_gradient_ref(lambda ws: synthesis_ref(tsd, ws, cfg, "const"), loss_fn, start, w_std, eps, steps, lr=args.lr,
                                  rampdown=args.lr_rampdown, rampup=args.lr_rampup)
    assert min(vabs) > 0.01, vabs                                           # no step sits at the branch point v = 0 (a condition, not a tolerance)
    eng = GradientProjectionEngine(G, target.cuda(), w_mean.cuda(), w_std, args, percept=PerceptualLoss(net="squeeze", allow_random_backbone=True),
                                   eps=eps.cuda(), noise_mode="const", use_graph=True, latent_space="w+")
    traj = []
    for i in range(steps):
        eng.run(1)
        traj.append(eng.latent_in.cpu().clone())
    lat, bstep, bloss, losses = eng.result()
    print(f"OBS w+ loop: losses max rel {np.abs(losses - np.array(ref[3])).max() / np.abs(np.array(ref[3])).max():.3e}")
    assert tuple(lat.shape) == (1, cfg.k, cfg.num_ws, cfg.w_dim) and bstep == ref[1]
    for i in range(steps):
        assert float((traj[i] - ref[4][i]).abs().max()) < 0.05 * args.lr * (i + 1), i
    assert np.abs(losses - np.array(ref[3])).max() < 1e-3 * np.abs(np.array(ref[3])).max()
    assert float((lat - ref[0]).abs().max() / ref[0].abs().max()) < 0.02
    assert float(traj[-1][0].std(dim=1).max()) > 0.2 * args.lr            # the slots started equal and moved apart


def test_lockstep_targets_with_msssim_equal_single_runs_teacher_forced(tiny):
    """B = 3 targets in one engine (per-target images: t_batch_stride = c h w) against three single-target engines, teacher-forced as in
    test_hip_dssim_gradient.py::test_lockstep_targets_with_dssim_equal_single_runs_teacher_forced (MS-SSIM + Wing, for the reason given there):
    the first step's losses and the latents after the second agree to 1e-5."""
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, synthetic_landmarks
    G, tsd, cfg = tiny
    steps, B = 4, 3
    torch.manual_seed(23)
    latent_mean = torch.randn(cfg.k, cfg.z_dim, device="cuda")
    eps = torch.randn(steps, B, cfg.k, cfg.z_dim, device="cuda")
    near = latent_mean[None] + 0.3 * torch.randn(B, cfg.k, cfg.z_dim, device="cuda")          # targets near the start: see loop_inputs
    targets = G(near, None, noise_mode="const")[0].clamp(-1, 1).clone()
    lms = [synthetic_landmarks(steps, 64, 9 + j) for j in range(B)]
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.5, pixel_term="msssim", msssim_levels=LEVELS)
    multi = GradientProjectionEngine(G, targets, latent_mean, 1.0, args, percept=None, lm_target=np.stack([l[0] for l in lms]),
                                     lm_steps=np.stack([l[1] for l in lms]), eps=eps, noise_mode="const", use_graph=True).run(1)
    torch.cuda.synchronize()
    state = [t.clone() for t in (multi.latent_in, multi.exp_avg, multi.exp_avg_sq)]
    loss0 = multi.losses.cpu().numpy()[:, 0].copy()
    assert float(multi.lr_table[1]) > 0
    multi.run(1)
    torch.cuda.synchronize()
    after = multi.latent_in.cpu().clone()
    assert float((after - state[0].cpu()).abs().max()) > 0.2 * float(multi.lr_table[1]), "the step must move the latents"
    for j in range(B):
        e = GradientProjectionEngine(G, targets[j:j + 1].contiguous(), latent_mean, 1.0, args, percept=None, lm_target=lms[j][0],
                                     lm_steps=lms[j][1], eps=eps[:, j:j + 1].contiguous(), noise_mode="const", use_graph=False).run(1)
        torch.cuda.synchronize()
        l0 = float(e.losses.cpu().numpy().reshape(-1)[0])
        assert abs(l0 - loss0[j]) <= 1e-5 * abs(l0), (j, l0, loss0[j])
        for dst, src in zip((e.latent_in, e.exp_avg, e.exp_avg_sq), state):
            dst.copy_(src[j:j + 1].reshape(dst.shape))
        e.run(1)
        torch.cuda.synchronize()
        single = e.latent_in.cpu().reshape(after[j].shape)
        err = float((after[j] - single).abs().max() / single.abs().max())
        print(f"OBS lockstep target {j}: loss {l0:.4f}, latent_in max rel diff {err:.3e}")
        assert err <= 1e-5, (j, err)


def test_target_pair_with_msssim_is_the_weighted_sum_and_steps_like_autograd(tiny):
    """A target pair at alpha = 0.3, MS-SSIM alone: the logged pixel value is (1 - alpha) loss(x, Ta) + alpha loss(x, Tb) of the reference on
    the engine's own image, and the steps equal autograd + Adam's on that explicit two-target objective through the CPU generator (the loop
    gates: trajectory within 0.05 lr (i + 1), losses within 1e-3)."""
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    from oracle.generator_ref import generator_ref
    from oracle.loss_ref import projection_gradient_ref
    G, tsd, cfg = tiny
    steps, al = 3, 0.3
    ta, latent_mean, eps = loop_inputs(tsd, cfg, steps)
    tb = generator_ref(tsd, latent_mean[None] + 0.2 * torch.from_numpy(                      # the second identity: another image near the start
        np.random.Generator(np.random.PCG64(8)).standard_normal((1, cfg.k, cfg.z_dim)).astype(np.float32)), cfg, "const").clamp(-1, 1).detach()
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.2, pixel_term="msssim", msssim_levels=LEVELS, min_loss_init=1e4)
    pair_loss = lambda img: (1 - al) * msssim_torch(img, ta[0], LEVELS)[0] + al * msssim_torch(img, tb[0], LEVELS)[0]
    ref = projection_gradient_ref(lambda z: generator_ref(tsd, z, cfg, "const"), lambda i, img: args.beta * pair_loss(img), latent_mean, 1.0, eps,
                                  steps, lr=args.lr, rampdown=args.lr_rampdown, rampup=args.lr_rampup, min_loss_init=args.min_loss_init)
    eng = GradientProjectionEngine(G, ta.cuda(), latent_mean.cuda(), 1.0, args, percept=None, eps=eps.cuda(), noise_mode="const", use_graph=True,
                                   target_b=tb.cuda(), morph_alpha=al)
    imgs, traj = [], []
    for i in range(steps):
        eng.run(1)
        torch.cuda.synchronize()
        imgs.append(G.img[:1].cpu().clone())
        traj.append(eng.latent_in.cpu().clone())
    losses = eng.losses.cpu().numpy().reshape(-1)
    for i in range(steps):
        want = args.beta * float(pair_loss(imgs[i]))
        assert abs(losses[i] - want) <= 1e-6 * abs(want), (i, losses[i], want)       # the value on the image the engine made
        assert float((traj[i] - ref[4][i]).abs().max()) < 0.05 * args.lr * (i + 1), i
    want = np.array([float(v) for v in ref[3]])
    print(f"OBS pair: losses {losses.tolist()} oracle {want.tolist()}")
    assert np.abs(losses - want).max() < 1e-3 * np.abs(want).max()
    assert float((traj[-1] - latent_mean).abs().max()) > 0.5 * args.lr        # (step 0 has lr = 0 under the ramp-up; the later ones move)


def test_literal_engine_scores_candidates_with_msssim(tiny):
    """The literal loop, batch = 3: each candidate's pixel loss against the reference on the image the engine generated, the best step a
    host-side argmin; and behind pool_above (the v1 driver's block mean) on the pooled image."""
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine
    G, tsd, cfg = tiny
    steps, B = 6, 3
    target, latent_mean, eps = loop_inputs(tsd, cfg, steps)
    for pool, levels in ((0, LEVELS), (32, 2)):
        tgt = torch.nn.functional.avg_pool2d(target, 2) if pool else target
        args = ProjectionArgs(step=steps, pixel_term="msssim", msssim_levels=levels, pool_above=pool, min_loss_init=1e4)
        eng = ProjectionEngine(G, tgt.cuda(), latent_mean.cuda(), 1.0, args, percept=None, use_mse=True, eps=eps.cuda(), noise_mode="const", batch=B)
        want = []
        for s in range(steps // B):
            eng.run(B)
            torch.cuda.synchronize()
            kept = (eng.pooled if pool else G.img)[:B].cpu().clone()
            want += msssim_torch(kept, tgt[0], levels).tolist()
        lat, bstep, bloss, losses = eng.result()
        want = np.array(want)
        print(f"OBS literal pool_above={pool}: losses {losses.tolist()} max rel {np.abs(losses - want).max() / np.abs(want).max():.3e}")
        assert (np.abs(losses - want) <= 1e-6 * np.abs(want)).all(), (losses, want)
        assert 0 < want.min() < 1 and bstep == int(np.argmin(losses)) and bloss == float(losses.min())


def test_msssim_refusals_of_the_engines(tiny):
    from morphganformer_amd._lib import MgfError
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, ProjectionEngine
    G, tsd, cfg = tiny
    tgt, lm = torch.zeros(1, 3, 64, 64, device="cuda"), torch.zeros(cfg.k, cfg.z_dim, device="cuda")
    ok = ProjectionArgs(step=2, pixel_term="msssim", msssim_levels=LEVELS)
    for cls in (GradientProjectionEngine, ProjectionEngine):
        with pytest.raises(MgfError, match="region_weight"):
            cls(G, tgt, lm, 1.0, ok, region_weight=torch.ones(1, 64, 64))
        with pytest.raises(MgfError, match=r"msssim_levels=4.*64x64 image allows 3 level"):
            cls(G, tgt, lm, 1.0, ProjectionArgs(step=2, pixel_term="msssim", msssim_levels=4))
        cls(G, tgt, lm, 1.0, ok)                                            # accepted
    with pytest.raises(MgfError, match="no backward pass"):
        GradientProjectionEngine(G, tgt, lm, 1.0, ProjectionArgs(step=2, pixel_term="msssim", msssim_levels=2, pool_above=32))
    with pytest.raises(MgfError, match="msssim_levels"):
        ProjectionArgs(step=2, pixel_term="msssim", msssim_levels=6)


def test_cli_project_gradient_mode_with_the_msssim_term(tmp_path):
    from morphganformer_amd import cli, drivers
    from test_host_and_abi import _tiny_snapshot
    from PIL import Image
    pkl = str(tmp_path / "net.pkl")
    _tiny_snapshot(pkl, seed=3)
    Image.fromarray((np.random.default_rng(0).random((64, 64, 3)) * 255).astype(np.uint8)).save(tmp_path / "a.png")
    argv = ["project", "--model", pkl, "--image", str(tmp_path / "a.png"), "--path_to_gen", str(tmp_path / "p"), "--size", "64", "--step", "6",
            "--n_mean_latent", "200", "--seed", "0", "--mode", "gradient", "--pixel-term", "msssim", "--msssim-levels", "3", "--lpips-random-backbone"]
    assert cli.main(argv) == 0
    files = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path / "p") for f in fs]
    mats = [f for f in files if f.endswith(".mat")]
    assert len(mats) == 1 and any(f.endswith(".png") for f in files), files
    w = drivers.load_latent_mat(mats[0])
    assert np.isfinite(w).all() and w.size > 0
    a = cli.build_parser().parse_args(["morph", "--model", pkl, "--w1", "a.mat", "--w2", "b.mat", "--out", "o", "--refine", "--pixel-term", "msssim",
                                       "--msssim-levels", "3"])
    assert (a.pixel_term, a.msssim_levels) == ("msssim", 3)
