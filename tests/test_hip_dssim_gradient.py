"""Gradient mode's DSSIM pixel term on the GPU: mgf_dssim_f32 / mgf_dssim_grad_f32 against torch autograd in float64 through
tests/dssim_torch_ref.py (pinned on oracle.loss_ref by tests/test_dssim_gradient_ref.py), and GradientProjectionEngine(pixel_term="dssim")
against autograd + Adam through the CPU restatement of the generator.

Kernel tolerances follow from float64 arithmetic with float32 stores -- the only roundings are the store and, when accumulating, the add:
value |got - want| <= 1e-6 |want|; gradient |got - want| <= 2 * 2^-23 (|want| + |prior|) per element + 1e-9 max |want| for the reordered
float64 sums."""
import os

import numpy as np
import pytest
import torch

from dssim_torch_ref import dssim_torch, dssim_torch_grad

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 7, 7), (1, 3, 9, 40), (2, 3, 64, 64), (1, 3, 70, 45), (3, 1, 33, 97), (1, 3, 1024, 1024)]


def _scratch(n, c, h, w):
    from morphganformer_amd import _lib
    return torch.empty(int(_lib.lib().mgf_dssim_scratch_bytes(n, c, h, w)) // 8, dtype=torch.float64, device="cuda")


def _value(img, tgt, scale=1.0, prior=None, fn="mgf_dssim_f32"):
    from morphganformer_amd import _lib
    n, c, h, w = img.shape
    out = torch.full([n], float("nan"), device="cuda") if prior is None else prior.clone()
    scratch = _scratch(n, c, h, w)
    _lib.check(getattr(_lib.lib(), fn)(out.data_ptr(), img.data_ptr(), tgt.data_ptr(), n, c, h, w, 0 if tgt.ndim == 3 else c * h * w, 255.0, scale,
                                       0 if prior is None else 1, scratch.data_ptr(), _lib.stream_ptr()), fn)
    return out


def _grad(img, tgt, scale=1.0, prior=None, with_out=True, out_prior=None):
    from morphganformer_amd import _lib
    n, c, h, w = img.shape
    dimg = torch.full_like(img, float("nan")) if prior is None else prior.clone()
    out = None if not with_out else (torch.full([n], float("nan"), device="cuda") if out_prior is None else out_prior.clone())
    scratch = _scratch(n, c, h, w)
    _lib.check(_lib.lib().mgf_dssim_grad_f32(dimg.data_ptr(), _lib.ptr(out), img.data_ptr(), tgt.data_ptr(), n, c, h, w,
                                             0 if tgt.ndim == 3 else c * h * w, 255.0, scale, 0 if prior is None else 1,
                                             0 if out_prior is None else 1, scratch.data_ptr(), _lib.stream_ptr()), "dssim_grad")
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


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dssim_kernels_vs_autograd(shape):
    """Value and gradient against float64 autograd: a shared target and per-sample targets, writing and accumulating onto a random prior,
    scale != 1, images that leave [-1, 1] (the generator's output is unclamped); the value of the fused pass is the value kernel's, bit for
    bit, and a second call gives the same bits."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(h * 1009 + w)
    img = torch.randn(shape, generator=g) * 0.7                             # |x| > 1 in places
    tgts = torch.rand(shape, generator=g) * 2 - 1
    prior = torch.randn(shape, generator=g) * 1e-4                          # about the size of the gradient: the add's rounding counts
    for shared in (True, False):
        tgt = tgts[0].contiguous() if shared else tgts
        tag = f"{shape} {'shared' if shared else 'per-sample'}"
        v_ref, g_ref = dssim_torch_grad(img, tgt)
        d_img, d_tgt = img.cuda(), tgt.cuda()
        val = _value(d_img, d_tgt)
        _check_value(tag, val, v_ref.numpy())
        dimg, out = _grad(d_img, d_tgt)
        _check_grad(tag + " write", dimg, g_ref)
        assert torch.equal(out, val), (tag, out, val)                       # the fused pass' value: the same bits
        dimg2, out2 = _grad(d_img, d_tgt)
        assert torch.equal(dimg, dimg2) and torch.equal(out, out2), tag      # same inputs, same bits
        assert torch.equal(_value(d_img, d_tgt), val)
        dimg_only, none = _grad(d_img, d_tgt, with_out=False)               # out may be NULL
        assert none is None and torch.equal(dimg_only, dimg)
        scale = 0.37
        dacc, oacc = _grad(d_img, d_tgt, scale=scale, prior=prior.cuda(), out_prior=torch.full([n], 2.0, device="cuda"))
        _check_grad(tag + " scale 0.37, accumulate", dacc, scale * g_ref, prior)
        _check_value(tag + " accumulated out (unscaled)", oacc, 2.0 + v_ref.numpy())
        _check_grad(tag + " scale -2.5", _grad(d_img, d_tgt, scale=-2.5)[0], -2.5 * g_ref)
        _check_value(tag + " value scale 0.5 onto 2", _value(d_img, d_tgt, scale=0.5, prior=torch.full([n], 2.0, device="cuda")),
                     2.0 + 0.5 * v_ref.numpy())


def test_dssim_gradient_of_a_smooth_image():
    """A smooth image with 1 % noise -- what a projection target looks like -- where uxx - ux^2 cancels: float32 arithmetic loses 2e-4 of the
    gradient here, float64 keeps the gate of the random images."""
    shape = (1, 3, 128, 128)
    g = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 128), torch.linspace(0, 1, 128), indexing="ij")
    base = torch.stack([0.8 * torch.sin(3 * xx + 2 * yy), 0.6 * torch.cos(4 * yy - xx), 0.9 * xx * yy - 0.2])[None]
    tgt = (base + 0.01 * torch.randn(shape, generator=g))[0].contiguous()
    img = base + 0.01 * torch.randn(shape, generator=g)
    v_ref, g_ref = dssim_torch_grad(img, tgt)
    dimg, out = _grad(img.cuda(), tgt.cuda())
    _check_value("smooth", out, v_ref.numpy())
    _check_grad("smooth", dimg, g_ref)


def test_dssim_of_identical_images_is_zero_with_no_gradient():
    shape = (2, 3, 70, 45)
    g = torch.Generator().manual_seed(11)
    img = torch.randn(shape, generator=g) * 0.7
    dimg, out = _grad(img.cuda(), img.cuda())
    assert torch.equal(out, torch.zeros(2, device="cuda")), out
    assert torch.equal(_value(img.cuda(), img.cuda()), torch.zeros(2, device="cuda"))
    pert, _ = _grad((img + 0.05 * torch.randn(shape, generator=g)).cuda(), img.cuda())
    ratio = float(dimg.abs().max() / pert.abs().max())
    print(f"OBS identical images: max |gradient| {float(dimg.abs().max()):.3e}, on a perturbed image {float(pert.abs().max()):.3e}, ratio {ratio:.3e}")
    assert ratio < 1e-12


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (1, 3, 70, 45), (1, 3, 1024, 1024)], ids=lambda s: "x".join(map(str, s)))
def test_continuous_dssim_equals_the_quantised_kernel_on_the_uint8_grid(shape):
    """On images that lie on the uint8 grid the quantisation of mgf_dssim_u8_f32 is the identity: the two kernels agree to 1e-6."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(h + w)
    img = ((torch.randint(0, 256, shape, generator=g).double() - 127.5) / 127.5).float().cuda()
    tgt = ((torch.randint(0, 256, shape[1:], generator=g).double() - 127.5) / 127.5).float().cuda()
    cont, quant = _value(img, tgt), _value(img, tgt, fn="mgf_dssim_u8_f32")
    print(f"OBS uint8 grid {shape}: continuous {cont.tolist()} quantised {quant.tolist()}")
    assert float(((cont - quant).abs() / quant.abs()).max()) <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- the projection loop
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


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("terms", ["lpips+wing+dssim", "dssim"])
def test_gradient_projection_with_dssim_matches_autograd_adam(tiny, use_graph, terms):
    """The gradient-mode loop against torch autograd + torch.optim.Adam through the CPU oracle (the gates of
    test_hip_gradient.py::test_gradient_projection_matches_autograd_adam): LPIPS + lamda Wing + beta DSSIM with a skipped ("no face") step and
    injected noise streams, and DSSIM as the ONLY term -- there the latent moves on this gradient alone."""
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, synthetic_landmarks
    from morphganformer_amd.synth_weights import synthetic_latents
    from oracle.generator_ref import generator_ref
    from oracle.loss_ref import backbone_random, lpips_ref, projection_gradient_ref, wing_loss_ref
    G, tsd, cfg = tiny
    full = terms != "dssim"
    steps = 10
    rng = np.random.Generator(np.random.PCG64(4))
    latent_mean = torch.from_numpy(rng.standard_normal((cfg.k, cfg.z_dim)).astype(np.float32))
    eps = torch.from_numpy(rng.standard_normal((steps, 1, cfg.k, cfg.z_dim)).astype(np.float32))
    target = generator_ref(tsd, torch.from_numpy(synthetic_latents(cfg, 1, 1001)), cfg, "const").clamp(-1, 1)
    lm_t, lm_s = synthetic_landmarks(steps, 64, 9)
    valid = np.ones(steps, np.int32)
    if full:
        valid[3] = 0
    # beta: d dssim / d latent is about 1/110 of d MSE / d latent on these images (max |gradient| 0.055 against 6.0 at step 0), so beta = 100 gives
    # the pixel term the share of the gradient that it has in the test this one is modelled on.  That share matters: the random-backbone LPIPS
    # gradient differs from the CPU oracle's by up to 1.5e-2 of the total on single steps (ReLU / max-pool ties that float32 rounding decides
    # differently; teacher-forced, step by step, with pixel_term="mse" as well), which Adam amplifies -- at beta = 1 the run ends 1e-2 from the oracle's
    # losses with the per-step losses and DSSIM gradients still at 1e-7 / 1e-5.  The run on DSSIM alone takes beta = 0.8.
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.2, pixel_term="dssim", beta=100.0 if full else 0.8, min_loss_init=1e4)
    bb, lins = backbone_random("squeeze", 0), _squeeze_lins()

    def loss_fn(i, img):
        if not valid[i]:
            return None
        d = args.beta * dssim_torch(img, target[0])[0]
        if not full:
            return d
        return lpips_ref(bb, lins, img, target).sum() + args.lamda * wing_loss_ref(torch.from_numpy(lm_s[i]), torch.from_numpy(lm_t)) + d

    ref = projection_gradient_ref(lambda z: generator_ref(tsd, z, cfg, "const"), loss_fn, latent_mean, 1.0, eps, steps, lr=args.lr,
                                  rampdown=args.lr_rampdown, rampup=args.lr_rampup, min_loss_init=args.min_loss_init)
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
          f"{max(float((traj[i] - ref[4][i]).abs().max()) / (args.lr * (i + 1)) for i in range(steps)):.3e}, moved {moved:.3f}")
    for i in range(steps):
        assert float((traj[i] - ref[4][i]).abs().max()) < 0.05 * args.lr * (i + 1), i
    if full:
        assert np.isnan(losses[3]) and ref[3][3] is None
    assert np.abs(got - want).max() < 1e-3 * np.abs(want).max()
    assert bstep == ref[1]
    assert float((lat - ref[0]).abs().max()) < 0.05 * args.lr * steps


def test_wplus_gradient_projection_with_dssim_matches_autograd_adam(tiny):
    """latent_space="w+" with LPIPS + beta DSSIM against autograd + Adam on ws through the CPU restatement's synthesis network (the gates of
    test_hip_gradient.py::test_wplus_gradient_projection_matches_autograd_adam)."""
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    from morphganformer_amd.synth_weights import synthetic_latents
    from oracle.generator_ref import generator_ref, mapping_ref, synthesis_ref
    from oracle.loss_ref import backbone_random, lpips_ref, projection_gradient_ref
    G, tsd, cfg = tiny
    steps = 8
    rng = np.random.Generator(np.random.PCG64(14))
    w_mean = mapping_ref(tsd, torch.from_numpy(synthetic_latents(cfg, 1, 77)), cfg)[0].detach()
    eps = torch.from_numpy(rng.standard_normal((steps, 1, cfg.k, cfg.num_ws, cfg.w_dim)).astype(np.float32))
    target = generator_ref(tsd, torch.from_numpy(synthetic_latents(cfg, 1, 1001)), cfg, "const").clamp(-1, 1)
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.2, pixel_term="dssim")
    w_std = float(w_mean.std()) * 4
    bb, lins = backbone_random("squeeze", 0), _squeeze_lins()
    loss_fn = lambda i, img: lpips_ref(bb, lins, img, target).sum() + args.beta * dssim_torch(img, target[0])[0]
    start = w_mean[:, None, :].expand(cfg.k, cfg.num_ws, cfg.w_dim).contiguous()
    ref = projection_gradient_ref(lambda ws: synthesis_ref(tsd, ws, cfg, "const"), loss_fn, start, w_std, eps, steps, lr=args.lr,
                                  rampdown=args.lr_rampdown, rampup=args.lr_rampup)
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


def test_lockstep_targets_with_dssim_equal_single_runs_teacher_forced(tiny):
    """B = 3 targets in one engine (per-target images: t_batch_stride = c h w) against three single-target engines, teacher-forced: step 0 has
    lr = 0 under the ramp-up, then every single engine takes the lockstep engine's state of its target and both take ONE step with lr > 0.
    The first step's losses and the latents after the second agree to 1e-5.  The objective is DSSIM + Wing: with the LPIPS term the THIRD lockstep
    sample's image gradient differs from its single-target run by 2e-2 .. 4e-2 of its maximum -- with pixel_term="mse" just the same, and not at
    all without LPIPS (2.4e-6 on all three) -- which is the LPIPS backward at n = 3, not this term; the existing lockstep tests run B = 2."""
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, synthetic_landmarks
    G, tsd, cfg = tiny
    steps, B = 4, 3
    torch.manual_seed(23)
    latent_mean = torch.randn(cfg.k, cfg.z_dim, device="cuda")
    eps = torch.randn(steps, B, cfg.k, cfg.z_dim, device="cuda")
    targets = G(torch.randn(B, cfg.k, cfg.z_dim, device="cuda"), None, noise_mode="const")[0].clamp(-1, 1).clone()
    lms = [synthetic_landmarks(steps, 64, 9 + j) for j in range(B)]
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.5, pixel_term="dssim")
    percept = lambda: None                                                # (see the docstring)
    multi = GradientProjectionEngine(G, targets, latent_mean, 1.0, args, percept=percept(), lm_target=np.stack([l[0] for l in lms]),
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
        e = GradientProjectionEngine(G, targets[j:j + 1].contiguous(), latent_mean, 1.0, args, percept=percept(), lm_target=lms[j][0],
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
        upd = float((after[j] - single).abs().max() / (single - state[0][j].cpu()).abs().max())
        print(f"OBS lockstep target {j}: latent_in max rel diff {err:.3e} (relative to the update: {upd:.3e})")
        assert err <= 1e-5, (j, err)


def test_objectives_without_a_gradient_stay_refused(tiny):
    from morphganformer_amd._lib import MgfError
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    G, tsd, cfg = tiny
    tgt, lm = torch.zeros(1, 3, 64, 64, device="cuda"), torch.zeros(cfg.k, cfg.z_dim, device="cuda")
    for kw in (dict(pixel_term="psnr"), dict(pixel_term="lbp"), dict(pool_above=256), dict(pixel_term="dssim", pool_above=256)):
        with pytest.raises(MgfError, match="no backward pass"):
            GradientProjectionEngine(G, tgt, lm, 1.0, ProjectionArgs(step=2, **kw))
    with pytest.raises(MgfError, match="latent_copies"):
        GradientProjectionEngine(G, tgt, lm, 1.0, ProjectionArgs(step=2, pixel_term="dssim", latent_copies=18))
    GradientProjectionEngine(G, tgt, lm, 1.0, ProjectionArgs(step=2, pixel_term="dssim"))             # accepted


def test_cli_project_gradient_mode_with_the_dssim_term(tmp_path):
    from morphganformer_amd import cli, drivers
    from test_host_and_abi import _tiny_snapshot
    from PIL import Image
    pkl = str(tmp_path / "net.pkl")
    _tiny_snapshot(pkl, seed=3)
    Image.fromarray((np.random.default_rng(0).random((64, 64, 3)) * 255).astype(np.uint8)).save(tmp_path / "a.png")
    argv = ["project", "--model", pkl, "--image", str(tmp_path / "a.png"), "--path_to_gen", str(tmp_path / "p"), "--size", "64", "--step", "6",
            "--n_mean_latent", "200", "--seed", "0", "--mode", "gradient", "--pixel-term", "dssim", "--lpips-random-backbone"]
    assert cli.main(argv) == 0
    files = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path / "p") for f in fs]
    mats = [f for f in files if f.endswith(".mat")]
    assert len(mats) == 1 and any(f.endswith(".png") for f in files), files
    w = drivers.load_latent_mat(mats[0])
    assert np.isfinite(w).all() and w.size > 0
