"""Two-identity morph refinement in gradient mode: the pair kernel against float64 autograd, the blended LPIPS taps
and the pair biometric term against the explicit two-target sums, the engine against the CPU oracle's loop on the explicit objective, its end
points against the single-target engine, lockstep pairs, the driver and the command line."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-3        # tests/test_hip_gradient.py's gate on gradients


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def relf(a, b):
    """rel() for quantities that can be exactly 0 (a cosine distance of parallel vectors): a reference below 1e-9 holds only float64 rounding,
    so the denominator stops there -- differences under 1e-15 pass, nothing larger does that would not pass rel()."""
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-9))


@pytest.fixture(scope="module")
def tiny():
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.grad import GeneratorGrad
    from morphganformer_amd.synth_weights import TINY, make_state_dict
    from oracle.generator_ref import to_torch_state
    sd = make_state_dict(TINY, seed=0)
    G = Generator(sd, TINY, "cuda", max_batch=3)
    return GeneratorGrad(G), to_torch_state(sd), TINY


@pytest.fixture(scope="module")
def pair_images(tiny):
    """Two target images of the tiny generator (the two identities), and a third to start from."""
    gg, tsd, cfg = tiny
    gen = torch.Generator(device="cuda")
    gen.manual_seed(77)
    z = torch.randn(2, cfg.k, cfg.z_dim, device="cuda", generator=gen)
    img = gg.G(z, None, noise_mode="const")[0].clamp(-1, 1).clone()
    return img[0:1].contiguous(), img[1:2].contiguous(), z.cpu()


# ------------------------------------------------------------------------------------------------------------------ the kernel
def pair_launch(emb, ta, tb, alpha, gamma, delta, metric, loss=None, accumulate=0, want_demb=True, trace=None, step=None):
    from morphganformer_amd import _lib
    n, width = emb.shape
    loss = torch.zeros(n, device="cuda") if loss is None else loss
    demb = torch.full((n, width), float("nan"), device="cuda") if want_demb else None
    stride = width if ta.ndim == 2 else 0
    _lib.check(_lib.lib().mgf_embed_pair_loss_f32(loss.data_ptr(), _lib.ptr(demb), _lib.ptr(trace), emb.data_ptr(), ta.data_ptr(), tb.data_ptr(),
                                                  alpha.data_ptr(), n, width, stride, gamma, delta, metric, accumulate, _lib.ptr(step),
                                                  0 if trace is None else trace.shape[1], _lib.stream_ptr()), "embed_pair_loss")
    torch.cuda.synchronize()
    return loss, demb


def pair_ref(emb, ta, tb, alpha, gamma, delta, metric):
    """float64 torch autograd on the float32 inputs."""
    e = emb.double().cpu().requires_grad_(True)
    a = alpha.double().cpu()

    def d(t):
        t = t.double().cpu().expand_as(e)
        if metric == 0:
            return (e - t).square().mean(1)
        return 1.0 - torch.nn.functional.cosine_similarity(e, t, dim=1, eps=1e-8)

    da, db = d(ta), d(tb)
    val = gamma * ((1 - a) * da + a * db) + delta * (da - db).abs()
    (g,) = torch.autograd.grad(val.sum(), e)
    return val.detach(), g, da.detach(), db.detach()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("width", [1, 63, 64, 65, 512, 513])
def test_pair_kernel_matches_float64_autograd(width, n, metric):
    """Widths around the wave (63, 64, 65), one element, and past the block's 256 threads (512, 513: further passes of the strided loop);
    shared and per-sample targets; per-sample alpha including 0 and 1; delta 0 and > 0; accumulate; demb NULL; the trace row from the counter.
    float64 arithmetic on float32 inputs: value and gradient within 1e-6 of max|.| (the float32 rounding of the outputs)."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 * width + 10 * n + metric)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    emb = r(n, width)
    alpha = torch.tensor([0.3, 0.0, 1.0][:n], device="cuda")
    gamma = 0.75
    for shared in (True, False):
        ta, tb = (r(width), r(width)) if shared else (r(n, width), r(n, width))
        for delta in (0.0, 0.25):
            val, g, da, db = pair_ref(emb, ta, tb, alpha, gamma, delta, metric)
            rows = 4
            trace = torch.full((n, rows, 2), float("nan"), dtype=torch.float64, device="cuda")
            step = torch.tensor([2], dtype=torch.int32, device="cuda")
            loss, demb = pair_launch(emb, ta, tb, alpha, gamma, delta, metric, trace=trace, step=step)
            assert relf(loss, val) < 1e-6, (shared, delta)
            if metric == 1 and width == 1:
                # the cosine of two scalars is +-1: the exact gradient is 0, and both sides hold the float64 rounding of two cancelling terms of
                # size (gamma + delta) / |e| -- a relative comparison of the two would compare noise with noise
                bound = 1e-12 / emb.double().cpu().abs()
                assert (demb.double().cpu().abs() <= bound).all() and (g.abs() <= bound).all()
            else:
                assert rel(demb, g) < 1e-6, (shared, delta)
            tr = trace.cpu()
            assert torch.isnan(tr[:, [0, 1, 3]]).all()
            assert relf(tr[:, 2, 0], da) < 1e-10 and relf(tr[:, 2, 1], db) < 1e-10
            # accumulate adds the float32 value to what is there; without demb the value is the same
            pre = torch.full((n,), 0.5, device="cuda")
            acc, none = pair_launch(emb, ta, tb, alpha, gamma, delta, metric, loss=pre.clone(), accumulate=1, want_demb=False)
            assert none is None and torch.equal(acc, pre + loss)
            # a counter past the table lands on its last row
            step.fill_(9)
            pair_launch(emb, ta, tb, alpha, gamma, delta, metric, trace=trace, step=step)
            assert torch.equal(trace[:, 3].cpu(), tr[:, 2])


@pytest.mark.parametrize("metric", [0, 1])
def test_pair_kernel_special_points(metric):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5 + metric)
    n, width = 3, 130
    emb, ta = torch.randn(n, width, device="cuda", generator=gen), torch.randn(width, device="cuda", generator=gen)
    alpha = torch.tensor([0.3, 0.5, 0.9], device="cuda")
    # d_a == d_b exactly (ta == tb): the balance term contributes 0 to value and gradient, as d|x|/dx at 0 is 0 in torch
    l0, g0 = pair_launch(emb, ta, ta.clone(), alpha, 0.75, 0.0, metric)
    l1, g1 = pair_launch(emb, ta, ta.clone(), alpha, 0.75, 0.5, metric)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    val, g, _, _ = pair_ref(emb, ta, ta.clone(), alpha, 0.75, 0.5, metric)
    assert rel(l1, val) < 1e-6 and rel(g1, g) < 1e-6
    # e == ta: finite, and the reference's value
    tb = torch.randn(width, device="cuda", generator=gen)
    e2 = ta.expand(n, width).contiguous()
    l2, g2 = pair_launch(e2, ta, tb, alpha, 0.75, 0.5, metric)
    val, g, _, _ = pair_ref(e2, ta, tb, alpha, 0.75, 0.5, metric)
    assert torch.isfinite(l2).all() and torch.isfinite(g2).all()
    assert rel(l2, val) < 1e-6 and rel(g2, g) < 1e-6


def test_pair_kernel_cosine_of_a_zero_embedding_follows_the_eps_rule():
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    n, width = 2, 65
    emb = torch.randn(n, width, device="cuda", generator=gen)
    emb[1].zero_()
    ta, tb = torch.randn(width, device="cuda", generator=gen), torch.randn(width, device="cuda", generator=gen)
    alpha = torch.tensor([0.4, 0.4], device="cuda")
    loss, demb = pair_launch(emb, ta, tb, alpha, 1.0, 0.25, 1)
    val, g, _, _ = pair_ref(emb, ta, tb, alpha, 1.0, 0.25, 1)
    assert torch.isfinite(loss).all() and torch.isfinite(demb).all()
    assert rel(loss, val) < 1e-6
    for i in range(n):                               # per row: the zero row's gradient is 1 / eps times larger than the other's
        assert rel(demb[i], g[i]) < 1e-6, i


# ------------------------------------------------------------------------------------------------------------------ the two loss objects
@pytest.mark.parametrize("net,size,alphas", [("squeeze", 64, (0.3,)), ("vgg", 32, (0.3,)), ("squeeze", 64, (0.3, 0.7))])
def test_perceptual_pair_matches_the_explicit_two_target_sum(net, size, alphas):
    from morphganformer_amd.lpips import PerceptualLoss, WEIGHTS_DIR
    from oracle.loss_ref import backbone_random, lpips_ref
    torch.manual_seed(size + len(alphas))
    n = len(alphas)
    pred = (torch.rand(n, 3, size, size) * 2 - 1).requires_grad_(True)
    ta, tb = torch.rand(n, 3, size, size) * 2 - 1, torch.rand(n, 3, size, size) * 2 - 1
    al = torch.tensor(alphas)
    bb = backbone_random(net, 0)
    lin = np.load(os.path.join(WEIGHTS_DIR, f"lpips_lin_{net}.npz"))
    lins = [torch.from_numpy(lin[f"lin{i}"]).float().reshape(-1) for i in range(len(lin.files))]
    val = (1 - al) * lpips_ref(bb, lins, pred, ta, net=net).reshape(n) + al * lpips_ref(bb, lins, pred, tb, net=net).reshape(n)
    (ref,) = torch.autograd.grad(val.sum() * 0.7, pred)
    pl = PerceptualLoss(net=net, allow_random_backbone=True)
    pl.set_target_pair(ta.cuda(), tb.cuda(), list(alphas))
    ptrs = [t.data_ptr() for t in pl._target_taps] + [pl.pair_offset.data_ptr()]
    pl.set_target_pair(ta.cuda(), tb.cuda(), list(alphas))               # same geometry: rewritten in place
    assert ptrs == [t.data_ptr() for t in pl._target_taps] + [pl.pair_offset.data_ptr()]
    out = torch.empty(n, device="cuda")
    pl.distance_into(out, pred.detach().cuda(), keep_taps=True)
    print("value", rel(out + pl.pair_offset, val))
    assert rel(out + pl.pair_offset, val) < 1e-4
    dimg = torch.zeros(n, 3, size, size, device="cuda")
    pl.grad_into(dimg, scale=0.7)
    print("gradient", rel(dimg, ref))
    assert rel(dimg, ref) < GRAD_TOL
    # alpha exactly 0 / 1: that target's own taps, bit for bit, and no offset
    single = PerceptualLoss(net=net, allow_random_backbone=True)
    for a, t in ((0.0, ta), (1.0, tb)):
        pl.set_target_pair(ta.cuda(), tb.cuda(), a)
        single.set_target(t.cuda())
        assert all(torch.equal(p, q) for p, q in zip(pl._target_taps, single._target_taps))
        assert float(pl.pair_offset.abs().max()) == 0.0
    pl.set_target(ta.cuda())
    assert pl.pair_offset is None


def test_biometric_pair_matches_the_mean_of_two_single_target_terms():
    """mse metric, id_balance 0, alpha 0.5: the value is the mean of two single-target BiometricLoss values, the gradient that of the
    float64 oracle (median / rms gate of test_biometric_gradient_matches_autograd: PReLU sign flips make the maximum unstable)."""
    from morphganformer_amd.iresnet import BiometricLoss, IResNetEmbedder, random_state
    from oracle.embed_ref import biometric_loss_ref
    torch.manual_seed(112)
    size, n = 112, 1
    sd_np = random_state(18, seed=3)
    sd64 = {k: torch.from_numpy(v).double() for k, v in sd_np.items()}
    pred = (torch.rand(n, 3, size, size, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    ta, tb = (torch.rand(1, 3, size, size, dtype=torch.float64) * 2 - 1 for _ in range(2))
    val = 0.5 * biometric_loss_ref(sd64, pred, ta, 18) + 0.5 * biometric_loss_ref(sd64, pred, tb, 18)
    (ref,) = torch.autograd.grad(val.sum() * 0.3, pred)
    p32 = pred.detach().float().cuda()
    singles = []
    for t in (ta, tb):
        b = BiometricLoss(IResNetEmbedder(sd_np, depth=18, n=n, device="cuda"))
        b.set_target(t.float().cuda())
        singles.append(b.distance_into(torch.empty(n, device="cuda"), p32).clone())
    bio = BiometricLoss(IResNetEmbedder(sd_np, depth=18, n=n, device="cuda"))
    bio.set_target_pair(ta.float().cuda(), tb.float().cuda(), 0.5)
    out = bio.distance_into(torch.empty(n, device="cuda"), p32)
    assert rel(out, 0.5 * (singles[0] + singles[1])) < 1e-4
    assert rel(out, val) < 1e-4
    dimg = torch.full((n, 3, size, size), 0.5, device="cuda")
    bio.grad_into(dimg, scale=0.3, accumulate=True)                        # (another scale than distance_into's: the pair launch runs again)
    err = (dimg.double().cpu() - 0.5 - ref).abs() / ref.abs().max()
    print("median", float(err.median()), "rms", float(err.square().mean().sqrt()))
    assert float(err.median()) < 1e-5 and float(err.square().mean().sqrt()) < 1e-3
    bio.set_target(ta.float().cuda())                                      # a later set_target clears the pair
    assert rel(bio.distance_into(torch.empty(n, device="cuda"), p32), singles[0]) < 1e-6


# ------------------------------------------------------------------------------------------------------------------ the engine
@pytest.mark.parametrize("use_graph", [False, True])
def test_pair_engine_matches_autograd_adam_on_the_explicit_objective(tiny, use_graph):
    """LPIPS(squeeze) + Wing + MSE against two targets, alpha = 0.4, a skipped step: the oracle's loss is the explicit weighted two-target
    sum, the engine runs the blended single-target kernels plus the constants.  Gates of test_gradient_projection_matches_autograd_adam."""
    from morphganformer_amd.lpips import PerceptualLoss, WEIGHTS_DIR
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, synthetic_landmarks
    from morphganformer_amd.synth_weights import synthetic_latents
    from oracle.generator_ref import generator_ref
    from oracle.loss_ref import backbone_random, lpips_ref, mse_ref, projection_gradient_ref, wing_loss_ref
    gg, tsd, cfg = tiny
    steps, al = 10, 0.4
    rng = np.random.Generator(np.random.PCG64(4))
    latent_mean = torch.from_numpy(rng.standard_normal((cfg.k, cfg.z_dim)).astype(np.float32))
    eps = torch.from_numpy(rng.standard_normal((steps, 1, cfg.k, cfg.z_dim)).astype(np.float32))
    ta = generator_ref(tsd, torch.from_numpy(synthetic_latents(cfg, 1, 1001)), cfg, "const").clamp(-1, 1)
    tb = generator_ref(tsd, torch.from_numpy(synthetic_latents(cfg, 1, 1002)), cfg, "const").clamp(-1, 1)
    lm_a, lm_s = synthetic_landmarks(steps, 64, 9)
    lm_b, _ = synthetic_landmarks(steps, 64, 10)
    valid = np.ones(steps, np.int32)
    valid[3] = 0
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.2)
    bb = backbone_random("squeeze", 0)
    lin = np.load(os.path.join(WEIGHTS_DIR, "lpips_lin_squeeze.npz"))
    lins = [torch.from_numpy(lin[f"lin{i}"]).float().reshape(-1) for i in range(7)]
    lm_t = torch.from_numpy((1 - al) * lm_a + al * lm_b)

    def loss_fn(i, img):
        if not valid[i]:
            return None
        w = wing_loss_ref(torch.from_numpy(lm_s[i]), lm_t)
        lp = (1 - al) * lpips_ref(bb, lins, img, ta).sum() + al * lpips_ref(bb, lins, img, tb).sum()
        return lp + args.lamda * w + args.beta * ((1 - al) * mse_ref(img, ta) + al * mse_ref(img, tb))

    ref = projection_gradient_ref(lambda z: generator_ref(tsd, z, cfg, "const"), loss_fn, latent_mean, 1.0, eps, steps, lr=args.lr,
                                  rampdown=args.lr_rampdown, rampup=args.lr_rampup)
    pl = PerceptualLoss(net="squeeze", allow_random_backbone=True)
    eng = GradientProjectionEngine(gg.G, ta.cuda(), latent_mean.cuda(), 1.0, args, percept=pl, lm_target=lm_a, lm_steps=lm_s, lm_valid=valid,
                                   eps=eps.cuda(), noise_mode="const", use_graph=use_graph, target_b=tb.cuda(), morph_alpha=al, lm_target_b=lm_b)
    traj = []
    for i in range(steps):
        eng.run(1)
        traj.append(eng.latent_in.cpu().clone())
    lat, bstep, bloss, losses = eng.result()
    assert float((ref[4][-1] - latent_mean).abs().max()) > 5 * args.lr * 0.2, "the oracle run must actually move the latent"
    for i in range(steps):
        assert float((traj[i] - ref[4][i]).abs().max()) < 0.05 * args.lr * (i + 1), i
    got = np.array([v for v in losses if not np.isnan(v)])
    want = np.array([v for v in ref[3] if v is not None])
    assert np.isnan(losses[3]) and ref[3][3] is None
    print("losses", np.abs(got - want).max() / np.abs(want).max())
    assert np.abs(got - want).max() < 1e-3 * np.abs(want).max()
    assert bstep == ref[1]


@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_pair_engine_end_points_are_the_single_target_engine(tiny, pair_images, alpha):
    from morphganformer_amd.iresnet import BiometricLoss, IResNetEmbedder
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, synthetic_landmarks
    gg, tsd, cfg = tiny
    ta, tb, _ = pair_images
    steps = 6
    torch.manual_seed(3)
    latent_mean = torch.randn(cfg.k, cfg.z_dim, device="cuda")
    eps = torch.randn(steps, 1, cfg.k, cfg.z_dim, device="cuda")
    lm_t, lm_s = synthetic_landmarks(steps, 64, 9)
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.25)
    mk = lambda target, **kw: GradientProjectionEngine(gg.G, target, latent_mean, 1.0, args, percept=PerceptualLoss(net="squeeze", allow_random_backbone=True),
                                                       lm_target=lm_t, lm_steps=lm_s, eps=eps, noise_mode="const", use_graph=True, **kw).run()
    single = mk(tb if alpha else ta)
    pair = mk(ta, target_b=tb, morph_alpha=alpha)
    assert torch.equal(pair.losses, single.losses) and torch.equal(pair.latent_in, single.latent_in)
    assert torch.equal(pair.best_latent, single.best_latent) and torch.equal(pair.best_step, single.best_step)
    # with the identity term (id_balance 0): the pair kernel sums in another order than mgf_mse_f32 -- the first loss to 1e-5
    bio = lambda: dict(biometric=BiometricLoss(IResNetEmbedder(None, depth=18, n=1, device="cuda")), gamma=0.5)
    s1 = mk(tb if alpha else ta, **bio())
    p1 = mk(ta, target_b=tb, morph_alpha=alpha, **bio())
    a, b = float(p1.losses[0]), float(s1.losses[0])
    assert abs(a - b) < 1e-5 * abs(b), (a, b)


def test_identity_terms_are_scored_traced_and_move_the_latent(tiny, pair_images):
    """id_balance > 0 with the cosine metric: finite losses, a moving latent, id_trace rows that are the distances of the step's own image,
    and a step-0 loss that is the sum of its separately computed terms."""
    import torch.nn.functional as F
    from morphganformer_amd.iresnet import BiometricLoss, IResNetEmbedder
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    gg, tsd, cfg = tiny
    ta, tb, _ = pair_images
    steps, al, gamma, bal = 5, 0.35, 0.5, 0.25
    torch.manual_seed(8)
    latent_mean = torch.randn(cfg.k, cfg.z_dim, device="cuda")
    eps = torch.randn(steps, 1, cfg.k, cfg.z_dim, device="cuda")
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.25, min_loss_init=1e30)
    eng = GradientProjectionEngine(gg.G, ta, latent_mean, 1.0, args, percept=PerceptualLoss(net="squeeze", allow_random_backbone=True), eps=eps,
                                   noise_mode="const", use_graph=False, biometric=BiometricLoss(IResNetEmbedder(None, depth=18, n=1, device="cuda")),
                                   gamma=gamma, target_b=tb, morph_alpha=al, id_balance=bal, id_metric="cosine")
    net = IResNetEmbedder(None, depth=18, n=1, device="cuda")
    emb = lambda img: net.embed_image(img).double().clone()
    ea, eb = emb(ta), emb(tb)
    dist = lambda img: tuple(float(1.0 - F.cosine_similarity(emb(img), t, dim=1, eps=1e-8)) for t in (ea, eb))
    imgs = []
    for i in range(steps):
        eng.run(1)
        imgs.append(gg.G.img.clone())
    losses, trace = eng.losses.cpu().numpy(), eng.id_trace.cpu().numpy()
    assert np.isfinite(losses).all() and np.isfinite(trace).all()
    assert float((eng.latent_in[0] - latent_mean).abs().max()) > 0.01
    for i in range(steps):
        da, db = dist(imgs[i])
        assert abs(trace[0, i, 0] - da) < 1e-5 and abs(trace[0, i, 1] - db) < 1e-5, i
    single = PerceptualLoss(net="squeeze", allow_random_backbone=True)
    lp = []
    for t in (ta, tb):
        single.set_target(t)
        lp.append(float(single.distance_into(torch.empty(1, device="cuda"), imgs[0])))
    da, db = dist(imgs[0])
    mse = lambda t: float((imgs[0].double() - t.double()).square().mean())
    want = ((1 - al) * lp[0] + al * lp[1]) + args.beta * ((1 - al) * mse(ta) + al * mse(tb)) + gamma * ((1 - al) * da + al * db) + bal * abs(da - db)
    assert abs(losses[0] - want) < 1e-4 * abs(want), (losses[0], want)
    # the DSSIM pixel term is evaluated against both targets: its step-0 value is the weighted sum of the two single-target values
    from morphganformer_amd import _lib
    a2 = ProjectionArgs(step=2, lr=0.05, pixel_term="dssim", min_loss_init=1e30)
    e2 = GradientProjectionEngine(gg.G, ta, latent_mean, 1.0, a2, percept=None, eps=eps[:2].contiguous(), noise_mode="const", use_graph=True,
                                  target_b=tb, morph_alpha=al).run()
    vals = []
    img0 = gg.G(latent_mean[None] + eps[0] * eng.sigma[0], None, noise_mode="const")[0].contiguous()
    scratch = torch.empty(int(_lib.lib().mgf_dssim_scratch_bytes(1, 3, 64, 64)) // 8, dtype=torch.float64, device="cuda")
    for t in (ta, tb):
        o = torch.zeros(1, device="cuda")
        _lib.check(_lib.lib().mgf_dssim_f32(o.data_ptr(), img0.data_ptr(), t.data_ptr(), 1, 3, 64, 64, 0, 255.0, 1.0, 0, scratch.data_ptr(), _lib.stream_ptr()))
        vals.append(float(o))
    want = a2.beta * ((1 - al) * vals[0] + al * vals[1])
    assert abs(float(e2.losses[0]) - want) < 1e-4 * abs(want)
    assert float((e2.latent_in[0] - latent_mean).abs().max()) > 1e-4


def test_lockstep_pairs_equal_single_pair_engines(tiny, pair_images):
    """Three pairs (alpha 0.25, 0.5, 0.75) in one engine against three single-pair engines on the same noise streams: the gates of
    test_gradient_projection_lockstep_targets_equal_single_runs."""
    from morphganformer_amd.iresnet import BiometricLoss, IResNetEmbedder
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    gg, tsd, cfg = tiny
    ta, tb, _ = pair_images
    # 6 steps at lr 0.02: the run ends inside the steep descent, where consecutive losses lie further apart than the 5e-2 the two dispatches may
    # drift, so "the best step" is a property of the objective and not of rounding (Adam's young, sign-like updates amplify 1e-6 differences
    # 5 - 10 x per step, see test_gradient_projection_lockstep_targets_equal_single_runs; at lr 0.05 the latent overshoots from step 5 on and
    # the last losses of a run tie to 0.3 %)
    steps, alphas = 6, [0.25, 0.5, 0.75]
    B = len(alphas)
    torch.manual_seed(21)
    starts = torch.randn(B, cfg.k, cfg.z_dim, device="cuda")
    eps = torch.randn(steps, B, cfg.k, cfg.z_dim, device="cuda")
    args = ProjectionArgs(step=steps, lr=0.02, lr_rampup=0.25, min_loss_init=1e30)
    kw = lambda n: dict(percept=PerceptualLoss(net="squeeze", allow_random_backbone=True), noise_mode="const", gamma=0.5, id_balance=0.1,
                        biometric=BiometricLoss(IResNetEmbedder(None, depth=18, n=n, device="cuda")))
    singles = []
    for j in range(B):
        e = GradientProjectionEngine(gg.G, ta, starts[j:j + 1], 1.0, args, eps=eps[:, j:j + 1].contiguous(), use_graph=False, target_b=tb,
                                     morph_alpha=alphas[j], **kw(1)).run()
        singles.append((e.result(), e.id_trace.cpu().numpy()[0]))
    rep = lambda t: t.expand(B, -1, -1, -1).contiguous()
    multi = GradientProjectionEngine(gg.G, rep(ta), starts, 1.0, args, eps=eps, use_graph=True, target_b=rep(tb), morph_alpha=alphas, **kw(B)).run()
    lat, bstep, bloss, losses = multi.result()
    trace = multi.id_trace.cpu().numpy()
    for j in range(B):
        (slat, sstep, sloss, slosses), strace = singles[j]
        scale = np.abs(slosses).max()
        print(j, "lockstep", losses[j].tolist(), "single", slosses.tolist(), "d_a - d_b", (strace[:, 0] - strace[:, 1]).tolist(),
              (trace[j, :, 0] - trace[j, :, 1]).tolist())
        assert np.abs(losses[j][:2] - slosses[:2]).max() < 1e-5 * scale, j
        assert np.abs(losses[j] - slosses).max() < 5e-2 * scale, j
        assert int(bstep[j]) == sstep
        assert np.abs(trace[j, :2] - strace[:2]).max() < 1e-5 * np.abs(strace).max()


def test_pair_engine_refusals(tiny, pair_images):
    from morphganformer_amd._lib import MgfError
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    gg, tsd, cfg = tiny
    ta, tb, _ = pair_images
    lm = torch.zeros(cfg.k, cfg.z_dim, device="cuda")
    mk = lambda **kw: GradientProjectionEngine(gg.G, ta, lm, 1.0, ProjectionArgs(step=2), noise_mode="const", **{"target_b": tb, **kw})

    class FakeMdf:
        differentiable = True

    with pytest.raises(MgfError, match="mdf"):
        mk(mdf=FakeMdf())
    with pytest.raises(MgfError, match="optimize_noise"):
        mk(optimize_noise=True)
    with pytest.raises(ValueError, match="id_balance"):
        mk(id_balance=0.5)
    with pytest.raises(ValueError, match="pair up"):
        mk(target_b=tb[:, :, :32].contiguous())
    with pytest.raises(ValueError, match="pair up"):
        mk(target_b=torch.cat([tb, tb]))
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            mk(morph_alpha=bad)
    with pytest.raises(ValueError, match="one per pair"):
        mk(morph_alpha=[0.2, 0.4])
    with pytest.raises(ValueError, match="id_metric"):
        mk(id_metric="euclid")
    with pytest.raises(ValueError, match="target_b"):
        mk(target_b=None, id_balance=0.5)


# ------------------------------------------------------------------------------------------------------------------ driver and command line
def test_refine_morph_driver(tiny, pair_images, tmp_path):
    from morphganformer_amd import drivers
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import ProjectionArgs
    gg, tsd, cfg = tiny
    ta, tb, z = pair_images
    w1, w2 = z[0:1].numpy(), z[1:2].numpy()
    alphas = (0.25, 0.5)
    args = ProjectionArgs(step=8, lr=0.05, lr_rampup=0.25, min_loss_init=1e30)
    kw = dict(args=args, latent_std=1.0, seed=4, noise_mode="const")
    res = drivers.refine_morph(gg.G, w1, w2, ta, tb, alphas, lockstep=True, percept=PerceptualLoss(net="squeeze", allow_random_backbone=True),
                               out_prefix=str(tmp_path / "m" / "a+b"), **kw)
    lat, _ = drivers.merge_morph(gg.G, w1, w2, alphas, noise_mode="const")
    assert [r["alpha"] for r in res] == list(alphas)
    for j, r in enumerate(res):
        assert np.array_equal(r["w_start"], lat[j])
        assert r["best_loss"] <= r["losses"][0] and r["best_loss"] == r["losses"][r["best_step"]]
        assert tuple(r["w"].shape) == (1, cfg.k, cfg.z_dim) and r["id_distances"] is None
    assert sorted(os.listdir(tmp_path / "m")) == ["a+b_a0.25_refined.mat", "a+b_a0.25_refined.png", "a+b_a0.50_refined.mat", "a+b_a0.50_refined.png"]
    assert np.array_equal(drivers.load_latent_mat(str(tmp_path / "m" / "a+b_a0.50_refined.mat")), res[1]["w"].numpy())
    one = drivers.refine_morph(gg.G, w1, w2, ta, tb, alphas, lockstep=False, percept=PerceptualLoss(net="squeeze", allow_random_backbone=True), **kw)
    for r, s in zip(res, one):
        scale = np.abs(s["losses"]).max()
        print(r["alpha"], "lockstep", r["losses"].tolist(), "single", s["losses"].tolist())
        assert np.abs(r["losses"][:2] - s["losses"][:2]).max() < 1e-5 * scale
        assert np.abs(r["losses"] - s["losses"]).max() < 5e-2 * scale
        assert r["best_step"] == s["best_step"]


def test_cli_morph_refine(tmp_path):
    from PIL import Image
    from morphganformer_amd import cli, drivers
    from morphganformer_amd.synth_weights import TINY
    from test_host_and_abi import _tiny_snapshot
    pkl = str(tmp_path / "net.pkl")
    _tiny_snapshot(pkl, seed=3)
    assert cli.main(["generate", "--model", pkl, "--output-dir", str(tmp_path / "g"), "--images-num", "2", "--seed", "1"]) == 0
    rng = np.random.Generator(np.random.PCG64(2))
    for name in ("a", "b"):
        drivers.save_latent_mat(str(tmp_path / f"{name}.mat"), rng.standard_normal((1, TINY.k, TINY.z_dim)).astype(np.float32))
    argv = ["morph", "--model", pkl, "--w1", str(tmp_path / "a.mat"), "--w2", str(tmp_path / "b.mat"), "--alphas", "0.5", "--out", str(tmp_path / "m" / "a+b"),
            "--refine", "--image-a", str(tmp_path / "g" / "sample_000000.png"), "--image-b", str(tmp_path / "g" / "sample_000001.png"), "--size", "64",
            "--step", "6", "--n_mean_latent", "200", "--seed", "0", "--lpips-random-backbone", "--biometric", "iresnet18", "--biometric-random",
            "--gamma", "0.1", "--id-balance", "0.05", "--id-metric", "cosine"]
    with pytest.raises(SystemExit, match="image-a"):
        cli.main(argv[:argv.index("--image-a")] + ["--size", "64"])
    assert cli.main(argv) == 0
    assert sorted(os.listdir(tmp_path / "m")) == ["a+b_a0.50.jpg", "a+b_a0.50.mat", "a+b_a0.50_refined.mat", "a+b_a0.50_refined.png"]
    w = drivers.load_latent_mat(str(tmp_path / "m" / "a+b_a0.50_refined.mat"))
    assert w.shape == (1, TINY.k, TINY.z_dim) and np.isfinite(w).all()
    assert Image.open(tmp_path / "m" / "a+b_a0.50_refined.png").size == (64, 64)
