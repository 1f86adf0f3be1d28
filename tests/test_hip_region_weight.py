"""Region-weighted LPIPS and pixel terms: the weighted tap / pixel kernels against float64, PerceptualLoss with a
weight against the float64 helper (tests/region_weight_torch_ref.py), both projection engines, target pairs, retarget, refusals and the
command line.  Tolerances are the ones the same kernel families are held to elsewhere: 1e-5 of the maximum for a tap kernel on given taps
(test_hip_lpips_spatial.py), 1e-4 for an LPIPS value through the backbone and GRAD_TOL for its gradient (test_hip_gradient.py), rtol 1e-6 for
MSE (test_hip_gradient.py)."""
import os

import numpy as np
import pytest
import torch

from region_weight_torch_ref import lpips_weighted_ref, mse_weighted_ref, weights

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-3        # tests/test_hip_gradient.py's gate on gradients


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def flat_weights(kind, n, hw, seed):
    """n normalised weight maps over hw pixels as float32 [n, hw]: random positive, a half with exact zeros, a feathered disc (a feathered
    interval where hw is no square)."""
    out = []
    for j in range(n):
        side = int(round(hw ** 0.5))
        if kind == "random":
            w = weights("random", 1, hw, seed + j)[0]
        elif kind == "half":
            w = (torch.arange(hw) >= (hw // 2 if j == 0 else hw // 3)).double()
        elif side * side == hw and side >= 3:
            w = weights("disc", side, side).reshape(-1).roll(j)
        else:
            p = torch.arange(hw, dtype=torch.float64)
            w = ((0.3 * hw - (p - hw / 2 - j).abs()) / (0.05 * hw + 1) + 0.5).clamp(0.0, 1.0)
        out.append((w / w.sum()).float())
    return torch.stack(out)


def tap_map64(f0, f1_unit, lin):
    """m[p] = sum_c lin[c] (f0 / (|f0| + 1e-10) - f1_unit)^2 in float64 on the CPU, [n, hw]; f1_unit is taken as given (already normalised)."""
    from oracle.loss_ref import normalize_tensor_ref
    d = (normalize_tensor_ref(f0.double().cpu()) - f1_unit.double().cpu()).square()
    return (d * lin.double().cpu().reshape(1, -1, 1)).sum(1)


def unit_taps(f):
    from morphganformer_amd import _lib
    out = torch.empty_like(f)
    n, c, hw = f.shape
    _lib.check(_lib.lib().mgf_lpips_unit_f32(out.data_ptr(), f.data_ptr(), n, c, hw, _lib.stream_ptr()))
    return out


def finish(scratch, nparts, n, scale=1.0):
    import ctypes as C
    from morphganformer_amd import _lib
    L = _lib.lib()
    out = torch.full((n,), float("nan"), device="cuda")
    _lib.check(L.mgf_lpips_finish_taps_f32(out.data_ptr(), scratch.data_ptr(), n * int(L.mgf_reduce_scratch_floats()), 1, (C.c_int32 * 8)(nparts),
                                           (C.c_float * 8)(scale), n, 0, _lib.stream_ptr()))
    return out


def defer_weighted(f0, f1, lin, om, per_sample_w, stats=None, f1_stride=None):
    import ctypes as C
    from morphganformer_amd import _lib
    L = _lib.lib()
    n, c, hw = f0.shape
    scratch = torch.full((n * int(L.mgf_reduce_scratch_floats()),), float("nan"), device="cuda")
    got = C.c_int32(0)
    _lib.check(L.mgf_lpips_layer_defer_weighted_f32(scratch.data_ptr(), _lib.ptr(stats), f0.data_ptr(), f1.data_ptr(), lin.data_ptr(), om.data_ptr(), n, c,
                                                    hw, c * hw if f1_stride is None else f1_stride, hw if per_sample_w else 0, C.byref(got),
                                                    _lib.stream_ptr()))
    return finish(scratch, got.value, n)


# ------------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("kind", ["random", "half", "disc"])
@pytest.mark.parametrize("n,c,hw", [(2, 64, 961), (1, 128, 225), (3, 384, 49), (2, 512, 9), (2, 100, 4999), (1, 16, 65539)])
def test_weighted_tap_forward_matches_float64(n, c, hw, kind):
    """mgf_lpips_layer_defer_weighted_f32 on random ReLU taps: shared and per-sample weights, with and without stats; stats bit-equal to the
    un-weighted entry's; omega = 1 / hw against the un-weighted entry; identical taps exactly 0.  (2,100,4999): a ragged last block;
    (1,16,65539): the 64-pixel dispatch."""
    import ctypes as C
    from morphganformer_amd import _lib
    L = _lib.lib()
    torch.manual_seed(c + hw)
    f0 = torch.relu(torch.randn(n, c, hw, device="cuda"))
    f1 = unit_taps(torch.relu(torch.randn(n, c, hw, device="cuda")))
    lin = torch.rand(c, device="cuda")
    m = tap_map64(f0, f1, lin)
    # un-weighted entry: stats and the value the uniform weight must reproduce
    stats0 = torch.full((n, 3, hw), float("nan"), device="cuda")
    scratch = torch.empty(n * int(L.mgf_reduce_scratch_floats()), device="cuda")
    got = C.c_int32(0)
    _lib.check(L.mgf_lpips_layer_defer_f32(scratch.data_ptr(), stats0.data_ptr(), f0.data_ptr(), f1.data_ptr(), lin.data_ptr(), n, c, hw, c * hw,
                                           C.byref(got), _lib.stream_ptr()))
    plain = finish(scratch, got.value, n, 1.0 / hw)
    for per_sample in (False, True):
        om = flat_weights(kind, n if per_sample else 1, hw, seed=hw).cuda().contiguous()
        want = (om.double().cpu() * m).sum(1)
        for with_stats in (False, True):
            stats = torch.full((n, 3, hw), float("nan"), device="cuda") if with_stats else None
            out = defer_weighted(f0, f1, lin, om, per_sample, stats)
            print(n, c, hw, kind, per_sample, with_stats, "value", rel(out, want))
            assert rel(out, want) < 1e-5
            if with_stats:
                assert torch.equal(stats, stats0)
    uniform = torch.full((1, hw), 1.0 / hw, device="cuda")
    assert rel(defer_weighted(f0, f1, lin, uniform, False), plain) < 1e-5
    same = defer_weighted(f0, unit_taps(f0), lin, flat_weights(kind, 1, hw, seed=1).cuda().contiguous(), False)
    assert float(same.abs().max()) == 0.0


@pytest.mark.parametrize("c,split,hw,behind", [(128, 64, 20000, True), (64, 64, 17000, True), (48, 16, 300, True), (512, 256, 49, False),
                                                 (100, 40, 5000, True), (130, 130, 4999, False), (64, 32, 961, True)])
def test_weighted_tap_backward_matches_float64_autograd(c, split, hw, behind):
    """mgf_lpips_layer_bwd_weighted_f32 against float64 autograd of scale * sum_p omega[p] m[p] on the same taps; the relu_stats form (with the
    forward's stats and without) against the plain form followed by mgf_relu_bwd_split_f32; omega = 0 pixels give exactly relu_mask * din;
    omega = 1 / hw against the un-weighted entries.  The shapes of the fused-backward test of test_hip_gradient.py plus (2,64,961)."""
    from morphganformer_amd import _lib
    L, st = _lib.lib(), _lib.stream_ptr()
    torch.manual_seed(c + hw)
    n, scale = 2, 0.7
    f0 = torch.relu(torch.randn(n, c, hw, device="cuda"))
    f1 = torch.nn.functional.normalize(torch.rand(n, c, hw, device="cuda"), dim=1)
    lin = torch.rand(c, device="cuda")
    dy = torch.randn(n, c, hw, device="cuda")
    bp = lambda t: t.data_ptr() if split < c else None
    for kind, per_sample in (("random", True), ("half", False), ("disc", True)):
        om = flat_weights(kind, n if per_sample else 1, hw, seed=c).cuda().contiguous()
        ws = hw if per_sample else 0
        x = f0.double().cpu().requires_grad_(True)
        m = tap_map64(x, f1, lin)
        (ref,) = torch.autograd.grad(scale * (om.double().cpu() * m).sum(), x)
        df = torch.full_like(f0, float("nan"))
        _lib.check(L.mgf_lpips_layer_bwd_weighted_f32(df.data_ptr(), f0.data_ptr(), f1.data_ptr(), lin.data_ptr(), om.data_ptr(), n, c, hw, c * hw, ws,
                                                      scale, 0, st))
        print(c, hw, kind, "gradient", rel(df, ref))
        assert rel(df, ref) < 1e-5
        # the plain form accumulating into the gradient from behind, then the ReLU backward with its split
        acc = dy.clone() if behind else torch.full_like(dy, float("nan"))
        _lib.check(L.mgf_lpips_layer_bwd_weighted_f32(acc.data_ptr(), f0.data_ptr(), f1.data_ptr(), lin.data_ptr(), om.data_ptr(), n, c, hw, c * hw, ws,
                                                      scale, int(behind), st))
        a0, b0 = torch.empty(n, split, hw, device="cuda"), torch.empty(n, max(c - split, 1), hw, device="cuda")
        _lib.check(L.mgf_relu_bwd_split_f32(a0.data_ptr(), bp(b0), acc.data_ptr(), f0.data_ptr(), n, c, split, hw, st))
        stats = torch.full((n, 3, hw), float("nan"), device="cuda")
        defer_weighted(f0, f1, lin, om, per_sample, stats)
        for sp in (None, stats):
            a1, b1 = torch.full_like(a0, float("nan")), torch.full_like(b0, float("nan"))
            _lib.check(L.mgf_lpips_layer_bwd_relu_stats_weighted_f32(a1.data_ptr(), bp(b1), dy.data_ptr() if behind else None, f0.data_ptr(),
                                                                     f1.data_ptr(), lin.data_ptr(), _lib.ptr(sp), om.data_ptr(), n, c, split, hw,
                                                                     c * hw, ws, scale, st))
            assert rel(a1, a0) < 1e-5 and (split == c or rel(b1, b0) < 1e-5)
            if kind == "half":          # omega = 0: the gradient from behind through the ReLU mask, unchanged
                zero = (om[0] == 0)
                assert int(zero.sum()) > 0
                full = torch.cat([a1, b1], dim=1) if split < c else a1
                want = torch.where(f0 > 0, dy, torch.zeros_like(dy)) if behind else torch.zeros_like(dy)
                assert torch.equal(full[:, :, zero], want[:, :, zero])
    # the uniform weight against the un-weighted entries
    uni = torch.full((1, hw), 1.0 / hw, device="cuda")
    d0, d1 = torch.empty_like(f0), torch.empty_like(f0)
    _lib.check(L.mgf_lpips_layer_bwd_f32(d0.data_ptr(), f0.data_ptr(), f1.data_ptr(), lin.data_ptr(), n, c, hw, c * hw, scale, 0, st))
    _lib.check(L.mgf_lpips_layer_bwd_weighted_f32(d1.data_ptr(), f0.data_ptr(), f1.data_ptr(), lin.data_ptr(), uni.data_ptr(), n, c, hw, c * hw, 0,
                                                  scale, 0, st))
    assert rel(d1, d0) < 1e-5
    a0, b0 = torch.empty(n, split, hw, device="cuda"), torch.empty(n, max(c - split, 1), hw, device="cuda")
    a1, b1 = torch.empty_like(a0), torch.empty_like(b0)
    _lib.check(L.mgf_lpips_layer_bwd_relu_stats_f32(a0.data_ptr(), bp(b0), dy.data_ptr() if behind else None, f0.data_ptr(), f1.data_ptr(),
                                                    lin.data_ptr(), None, n, c, split, hw, c * hw, scale, st))
    _lib.check(L.mgf_lpips_layer_bwd_relu_stats_weighted_f32(a1.data_ptr(), bp(b1), dy.data_ptr() if behind else None, f0.data_ptr(), f1.data_ptr(),
                                                             lin.data_ptr(), None, uni.data_ptr(), n, c, split, hw, c * hw, 0, scale, st))
    assert rel(a1, a0) < 1e-5 and (split == c or rel(b1, b0) < 1e-5)


@pytest.mark.parametrize("c,hw", [(3, 81), (3, 4489), (1, 4096)])
def test_weighted_mse_value_and_gradient(c, hw):
    """mgf_mse_weighted_f32 / mgf_mse_weighted_grad_f32 against float64 at rtol 1e-6: shared and per-sample targets and weights, accumulate 0
    and 1, and a weight pointer offset by one float (the scalar path), which gives the bits of the 16-byte path where both exist."""
    from morphganformer_amd import _lib
    L, st = _lib.lib(), _lib.stream_ptr()
    torch.manual_seed(hw)
    n, scale = 2, 0.5
    a = torch.randn(n, c, hw, device="cuda")
    scratch = torch.empty(n * int(L.mgf_reduce_scratch_floats()), device="cuda")
    for nt in (1, n):
        b = torch.randn(nt, c, hw, device="cuda")
        for kind, nw in (("random", 1), ("half", n), ("disc", n), ("random", n)):
            om = (flat_weights(kind, nw, hw, seed=c) / c).cuda().contiguous()                 # W / (C sum W)
            shifted = torch.empty(nw * hw + 1, device="cuda")[1:].view(nw, hw)                # the same values one float off the alignment
            shifted.copy_(om)
            d = (a.double() - b.double()).cpu()
            want_v = scale * (om.double().cpu()[:, None] * d.square()).sum(dim=(1, 2))
            want_g = scale * 2.0 * om.double().cpu()[:, None] * d
            outs = []
            for w in (om, shifted):
                for accumulate in (0, 1):
                    out = torch.full((n,), 3.0, device="cuda")
                    _lib.check(L.mgf_mse_weighted_f32(out.data_ptr(), a.data_ptr(), b.data_ptr(), w.data_ptr(), n, c, hw, c * hw if nt > 1 else 0,
                                                      hw if nw > 1 else 0, scale, accumulate, scratch.data_ptr(), st))
                    assert torch.allclose(out.double().cpu(), want_v + 3.0 * accumulate, rtol=1e-6, atol=0.0), (kind, nt, accumulate)
                    g = torch.ones_like(a)
                    _lib.check(L.mgf_mse_weighted_grad_f32(g.data_ptr(), a.data_ptr(), b.data_ptr(), w.data_ptr(), n, c, hw, c * hw if nt > 1 else 0,
                                                           hw if nw > 1 else 0, scale, accumulate, st))
                    assert torch.allclose(g.double().cpu(), want_g + accumulate, rtol=1e-6, atol=1e-7 * float(want_g.abs().max())), (kind, nt, accumulate)
                    outs.append((out, g))
            for (o0, g0), (o1, g1) in zip(outs[:2], outs[2:]):
                assert torch.equal(o0, o1) and torch.equal(g0, g1)


# ------------------------------------------------------------------------------------------------------------------ the module
def _lins(net):
    from morphganformer_amd.lpips import WEIGHTS_DIR
    lin = np.load(os.path.join(WEIGHTS_DIR, f"lpips_lin_{net}.npz"))
    return [torch.from_numpy(lin[f"lin{i}"]).float().reshape(-1) for i in range(len(lin.files))]


@pytest.mark.parametrize("net,size", [("squeeze", 64), ("squeeze", 67), ("vgg", 48), ("alex", 96)])
def test_perceptual_loss_with_a_region_weight(net, size):
    """distance_into / grad_into with a weight against the float64 helper: one target and one weight, n targets with n weights; the per-tap
    values; set_region_weight(None) afterwards reproduces the un-weighted values bit for bit."""
    from morphganformer_amd.lpips import PerceptualLoss
    from oracle.loss_ref import backbone_random
    torch.manual_seed(size)
    n = 2
    pred = torch.rand(n, 3, size, size) * 2 - 1
    bb, lins = backbone_random(net, 0), _lins(net)
    pl = PerceptualLoss(net=net, allow_random_backbone=True)
    out, dimg = torch.empty(n, device="cuda"), torch.empty(n, 3, size, size, device="cuda")
    target0 = (torch.rand(1, 3, size, size) * 2 - 1).cuda()
    pl.set_target(target0)
    pl.distance_into(out, pred.cuda(), keep_taps=True)
    plain_val = out.clone()
    plain_grad = pl.grad_into(dimg, scale=0.7).clone()
    plain_fused = pl.distance_into(torch.empty(n, device="cuda"), pred.cuda()).clone()
    for nt, kinds in ((1, ("half",)), (1, ("disc",)), (n, ("random", "half"))):
        target = torch.rand(nt, 3, size, size) * 2 - 1
        W = torch.stack([weights(k, size, size, seed=size + j) for j, k in enumerate(kinds)])
        x = pred.clone().requires_grad_(True)
        val, per = lpips_weighted_ref(bb, lins, x, target, W, net=net, per_layer=True)
        (ref,) = torch.autograd.grad(val.sum() * 0.7, x)
        pl.set_region_weight(W[:, None] if len(kinds) > 1 else W[0])
        pl.set_target(target.cuda())
        pl.distance_into(out, pred.cuda(), keep_taps=True)
        print(net, size, kinds, "value", rel(out, val))
        assert rel(out, val) < 1e-4
        pl.grad_into(dimg, scale=0.7)
        print(net, size, kinds, "gradient", rel(dimg, ref))
        assert rel(dimg, ref) < GRAD_TOL
        assert torch.equal(pl.distance_into(torch.empty(n, device="cuda"), pred.cuda()), out)      # without keep_taps: still the un-fused path
        assert rel(pl.distance_per_tap(pred.cuda()), torch.stack(per)) < 1e-4
        if nt == 1:
            single = pl(pred[:1].cuda(), target.cuda())
            assert tuple(single.shape) == (1, 1, 1, 1) and rel(single.reshape(1), val[:1]) < 1e-4
    pl.set_region_weight(None)
    pl.set_target(target0)
    pl.distance_into(out, pred.cuda(), keep_taps=True)
    assert torch.equal(out, plain_val) and torch.equal(pl.grad_into(dimg, scale=0.7), plain_grad)
    assert torch.equal(pl.distance_into(torch.empty(n, device="cuda"), pred.cuda()), plain_fused)


def test_region_weight_refusals_of_the_module():
    from morphganformer_amd.lpips import PerceptualLoss
    pl = PerceptualLoss(net="squeeze", allow_random_backbone=True)
    good = torch.ones(64, 64)
    for bad, what in ((-good, ">= 0"), (good * float("nan"), "finite"), (good * float("inf"), "finite"), (good * 0, "all-zero"),
                      (torch.ones(3, 64, 64), r"\[H,W\]"), (torch.ones(2, 3, 64, 64), r"\[H,W\]")):
        with pytest.raises(ValueError, match=what):
            pl.set_region_weight(bad)
    pl.set_region_weight(good)
    pl.set_target(torch.zeros(1, 3, 48, 48, device="cuda"))
    with pytest.raises(ValueError, match="64x64"):
        pl.distance_into(torch.empty(1, device="cuda"), torch.zeros(1, 3, 48, 48, device="cuda"))
    pl.set_region_weight(torch.ones(3, 1, 64, 64))
    pl.set_target(torch.zeros(1, 3, 64, 64, device="cuda"))
    with pytest.raises(ValueError, match="3 region weights"):
        pl.distance_into(torch.empty(2, device="cuda"), torch.zeros(2, 3, 64, 64, device="cuda"))


# ------------------------------------------------------------------------------------------------------------------ the engines
@pytest.fixture(scope="module")
def tiny():
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.grad import GeneratorGrad
    from morphganformer_amd.synth_weights import TINY, make_state_dict
    from oracle.generator_ref import to_torch_state
    sd = make_state_dict(TINY, seed=0)
    G = Generator(sd, TINY, "cuda", max_batch=4)
    return GeneratorGrad(G), to_torch_state(sd), TINY


@pytest.mark.parametrize("use_graph", [False, True])
def test_gradient_engine_with_a_region_weight_matches_autograd_adam(tiny, use_graph):
    """10 steps of LPIPS(squeeze) + Wing + MSE with one skipped step and a half-plane weight against projection_gradient_ref on the weighted
    loss: the gates of test_gradient_projection_matches_autograd_adam."""
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, synthetic_landmarks
    from morphganformer_amd.synth_weights import synthetic_latents
    from oracle.generator_ref import generator_ref
    from oracle.loss_ref import backbone_random, projection_gradient_ref, wing_loss_ref
    gg, tsd, cfg = tiny
    steps = 10
    rng = np.random.Generator(np.random.PCG64(4))
    latent_mean = torch.from_numpy(rng.standard_normal((cfg.k, cfg.z_dim)).astype(np.float32))
    eps = torch.from_numpy(rng.standard_normal((steps, 1, cfg.k, cfg.z_dim)).astype(np.float32))
    target = generator_ref(tsd, torch.from_numpy(synthetic_latents(cfg, 1, 1001)), cfg, "const").clamp(-1, 1)
    lm_t, lm_s = synthetic_landmarks(steps, 64, 9)
    valid = np.ones(steps, np.int32)
    valid[3] = 0
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.2)
    bb, lins = backbone_random("squeeze", 0), _lins("squeeze")
    W = weights("half", 64, 64)

    def loss_fn(i, img):
        if not valid[i]:
            return None
        w = wing_loss_ref(torch.from_numpy(lm_s[i]), torch.from_numpy(lm_t))
        return (lpips_weighted_ref(bb, lins, img, target, W).sum() + args.lamda * w + args.beta * mse_weighted_ref(img, target, W).sum()).float()

    ref = projection_gradient_ref(lambda z: generator_ref(tsd, z, cfg, "const"), loss_fn, latent_mean, 1.0, eps, steps, lr=args.lr,
                                  rampdown=args.lr_rampdown, rampup=args.lr_rampup)
    pl = PerceptualLoss(net="squeeze", allow_random_backbone=True)
    eng = GradientProjectionEngine(gg.G, target.cuda(), latent_mean.cuda(), 1.0, args, percept=pl, lm_target=lm_t, lm_steps=lm_s,
                                   lm_valid=valid, eps=eps.cuda(), noise_mode="const", use_graph=use_graph, region_weight=W)
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
    assert float((lat - ref[0]).abs().max()) < 0.05 * args.lr * steps


def test_lockstep_targets_with_two_region_weights_equal_single_runs(tiny):
    """B = 2 lockstep targets with two different weights against two single-target engines: the gates of
    test_gradient_projection_lockstep_targets_equal_single_runs."""
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, synthetic_landmarks
    gg, tsd, cfg = tiny
    G = gg.G
    steps, B = 8, 2
    torch.manual_seed(21)
    latent_mean = torch.randn(cfg.k, cfg.z_dim, device="cuda")
    eps = torch.randn(steps, B, cfg.k, cfg.z_dim, device="cuda")
    targets = G(torch.randn(B, cfg.k, cfg.z_dim, device="cuda"), None, noise_mode="const")[0].clamp(-1, 1).clone()
    lms = [synthetic_landmarks(steps, 64, 9 + j) for j in range(B)]
    W = torch.stack([weights("half", 64, 64), weights("disc", 64, 64)])
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.25)
    singles = []
    for j in range(B):
        e = GradientProjectionEngine(G, targets[j:j + 1].contiguous(), latent_mean, 1.0, args, percept=PerceptualLoss(net="squeeze", allow_random_backbone=True),
                                     lm_target=lms[j][0], lm_steps=lms[j][1], eps=eps[:, j:j + 1].contiguous(), noise_mode="const", use_graph=False,
                                     region_weight=W[j]).run()
        singles.append((e.result(), e.latent_in.cpu().clone()))
    multi = GradientProjectionEngine(G, targets, latent_mean, 1.0, args, percept=PerceptualLoss(net="squeeze", allow_random_backbone=True),
                                     lm_target=np.stack([l[0] for l in lms]), lm_steps=np.stack([l[1] for l in lms]), eps=eps, noise_mode="const",
                                     use_graph=True, region_weight=W[:, None]).run()
    lat, bstep, bloss, losses = multi.result()
    for j in range(B):
        (slat, sstep, sloss, slosses), sfinal = singles[j]
        print(j, "lockstep", losses[j].tolist(), "single", slosses.tolist())
        assert np.abs(losses[j][:2] - slosses[:2]).max() < 1e-5 * np.abs(slosses).max()
        assert np.abs(losses[j] - slosses).max() < 5e-2 * np.abs(slosses).max()
        assert int(bstep[j]) == sstep
        assert float((multi.latent_in[j].cpu() - sfinal[0]).abs().max()) < 0.25 * args.lr * steps
    assert not np.allclose(singles[0][0][3], singles[1][0][3])


@pytest.mark.parametrize("pool_above,pipeline", [(0, False), (0, True), (32, False)])
def test_literal_engine_with_a_region_weight(golden, pool_above, pipeline):
    """batch = 4, 12 steps, injected eps: every recorded loss within 1e-4 of the float64 helper evaluated one candidate at a time on the
    oracle's images, the best step equal; with pool_above = 32 the weight is given at 32^2; the pipelined loop gives the same bits."""
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine
    from morphganformer_amd.synth_weights import TINY, make_state_dict
    from oracle.generator_ref import generator_ref, to_torch_state
    from oracle.loss_ref import backbone_random, pool_above_ref
    g = golden("loop_tiny.npz")
    steps = 12
    sd = make_state_dict(TINY, seed=0)
    tsd = to_torch_state(sd)
    side = 32 if pool_above else 64
    target = torch.from_numpy(pool_above_ref(g["target"], pool_above).astype(np.float32)) if pool_above else torch.from_numpy(g["target"])
    W = weights("disc", side, side)
    mk = lambda pipe: ProjectionEngine(Generator(sd, TINY, "cuda", max_batch=1), target.cuda(), torch.from_numpy(g["latent_mean"]).cuda(),
                                       float(g["latent_std"]), ProjectionArgs(step=steps, pool_above=pool_above),
                                       percept=PerceptualLoss(net="squeeze", allow_random_backbone=True), eps=torch.from_numpy(g["eps"][:steps]).cuda(),
                                       noise_mode="const", batch=4, pipeline=pipe, region_weight=W).run()
    eng = mk(pipeline)
    lat, bstep, bloss, losses = eng.result()
    if pipeline:
        plain = mk(False)
        assert torch.equal(plain.losses, eng.losses) and torch.equal(plain.best_latent, eng.best_latent)
        return
    bb, lins = backbone_random("squeeze", 0), _lins("squeeze")
    want = []
    for i in range(steps):
        sigma = np.float32(np.float32(float(g["latent_std"])) * np.float32(0.05)) * np.float32(max(0, 1 - (i / steps) / 0.75) ** 2)
        z = torch.from_numpy(g["latent_mean"])[None] + torch.from_numpy(g["eps"][i]) * float(sigma)
        with torch.no_grad():
            img = generator_ref(tsd, z, TINY, "const")
            if pool_above:
                img = torch.from_numpy(pool_above_ref(img.numpy(), pool_above))
            want.append(float(lpips_weighted_ref(bb, lins, img, target, W).sum() + mse_weighted_ref(img, target, W).sum()))
    want = np.array(want)
    print("literal", pool_above, (np.abs(losses - want) / np.abs(want)).max())
    assert (np.abs(losses - want) < 1e-4 * np.abs(want)).all()
    assert bstep == int(np.argmin(want))


@pytest.mark.parametrize("alpha", [0.0, 0.3, 1.0])
def test_target_pair_with_a_region_weight(tiny, alpha):
    """The pair engine's losses against (1 - alpha) L_W(x, Ta) + alpha L_W(x, Tb), L_W = LPIPS_W + beta MSE_W by two single-target weighted
    evaluations of the same images (1e-4, the value gate of test_perceptual_pair_matches_the_explicit_two_target_sum)."""
    from morphganformer_amd import _lib
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    gg, tsd, cfg = tiny
    gen = torch.Generator(device="cuda")
    gen.manual_seed(77)
    imgs_t = gg.G(torch.randn(2, cfg.k, cfg.z_dim, device="cuda", generator=gen), None, noise_mode="const")[0].clamp(-1, 1).clone()
    ta, tb = imgs_t[0:1].contiguous(), imgs_t[1:2].contiguous()
    steps = 4
    torch.manual_seed(8)
    latent_mean = torch.randn(cfg.k, cfg.z_dim, device="cuda")
    eps = torch.randn(steps, 1, cfg.k, cfg.z_dim, device="cuda")
    W = weights("disc", 64, 64)
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.25, min_loss_init=1e30)
    eng = GradientProjectionEngine(gg.G, ta, latent_mean, 1.0, args, percept=PerceptualLoss(net="squeeze", allow_random_backbone=True), eps=eps,
                                   noise_mode="const", use_graph=False, target_b=tb, morph_alpha=alpha, region_weight=W)
    imgs = []
    for i in range(steps):
        eng.run(1)
        imgs.append(gg.G.img.clone())
    losses = eng.losses.cpu().numpy()
    single = PerceptualLoss(net="squeeze", allow_random_backbone=True)
    single.set_region_weight(W)
    L = _lib.lib()
    pix = (W / (3 * W.sum())).float().reshape(1, -1).cuda()
    scratch = torch.empty(int(L.mgf_reduce_scratch_floats()), device="cuda")
    for i in range(steps):
        vals = []
        for t in (ta, tb):
            single.set_target(t)
            lp = float(single.distance_into(torch.empty(1, device="cuda"), imgs[i]))
            o = torch.zeros(1, device="cuda")
            _lib.check(L.mgf_mse_weighted_f32(o.data_ptr(), imgs[i].data_ptr(), t.data_ptr(), pix.data_ptr(), 1, 3, 64 * 64, 0, 0, 1.0, 0,
                                              scratch.data_ptr(), _lib.stream_ptr()))
            vals.append(lp + args.beta * float(o))
        want = (1 - alpha) * vals[0] + alpha * vals[1]
        print("pair", alpha, i, abs(losses[i] - want) / abs(want))
        assert abs(losses[i] - want) < 1e-4 * abs(want), (i, losses[i], want)


def test_retarget_with_a_new_region_weight_equals_a_fresh_engine(golden):
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine, synthetic_landmarks
    from morphganformer_amd.synth_weights import TINY, make_state_dict, synthetic_latents
    g = golden("loop_tiny.npz")
    G = Generator(make_state_dict(TINY, seed=0), TINY, "cuda", max_batch=1)
    steps, batch = 16, 4
    mean, std = torch.from_numpy(g["latent_mean"]).cuda(), float(g["latent_std"])
    targets = [G(torch.from_numpy(synthetic_latents(TINY, 1, 3000 + j)).cuda(), None, noise_mode="const")[0].clamp(-1, 1) for j in range(2)]
    lms = [synthetic_landmarks(steps, 64, 20 + j) for j in range(2)]
    Ws = [weights("half", 64, 64), weights("disc", 64, 64)]

    def fresh(j, w):
        P = PerceptualLoss(net="squeeze", allow_random_backbone=True)
        return ProjectionEngine(G, targets[j], mean, std, ProjectionArgs(step=steps), percept=P, lm_target=lms[j][0], lm_steps=lms[j][1],
                                noise_mode="const", seed=100 + j, batch=batch, use_graph=True, region_weight=w)

    want = fresh(1, Ws[1]).run().result()
    kept = fresh(1, Ws[0]).run().result()
    eng = fresh(0, Ws[0]).run()
    graph = eng.graph
    eng.retarget(targets[1], lm_target=lms[1][0], lm_steps=lms[1][1], seed=101, region_weight=Ws[1])
    got = eng.run().result()
    assert eng.graph is graph and graph is not None
    assert got[1] == want[1] and got[2] == want[2] and torch.equal(got[0], want[0]) and np.array_equal(got[3], want[3])
    assert not np.array_equal(got[3], kept[3])                               # the weight really changed the objective
    eng.retarget(targets[1], lm_target=lms[1][0], lm_steps=lms[1][1], seed=101)          # without the argument the weight stays
    again = eng.run().result()
    assert np.array_equal(again[3], want[3])


def test_engine_refusals(golden, tiny):
    from morphganformer_amd._lib import MgfError
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, ProjectionEngine
    gg, tsd, cfg = tiny
    g = golden("loop_tiny.npz")
    target, mean = torch.from_numpy(g["target"]).cuda(), torch.from_numpy(g["latent_mean"]).cuda()
    good = torch.ones(64, 64)
    lit = lambda w, **a: ProjectionEngine(gg.G, target, mean, 1.0, ProjectionArgs(step=2, **a), noise_mode="const", region_weight=w,
                                          lbp_target=np.zeros((224, 224), np.uint8) if a.get("pixel_term") == "lbp" else None)
    grad = lambda w, **a: GradientProjectionEngine(gg.G, target, mean, 1.0, ProjectionArgs(step=2, **a), noise_mode="const", region_weight=w)
    for mk in (lit, grad):
        for bad, what in ((-good, ">= 0"), (good * float("nan"), "finite"), (good * 0, "all-zero"), (torch.ones(32, 32), "image-space losses see"),
                          (torch.ones(2, 1, 64, 64), "2 region weights")):
            with pytest.raises(ValueError, match=what):
                mk(bad)
        with pytest.raises(MgfError, match="weighted window forms"):
            mk(good, pixel_term="dssim")
    for term in ("psnr", "lbp"):
        with pytest.raises(MgfError, match="weighted window forms"):
            lit(good, pixel_term=term)
    with pytest.raises(MgfError, match="latent_copies"):
        lit(good, latent_copies=2)
    eng = lit(None)
    with pytest.raises(MgfError, match="without a region_weight"):
        eng.retarget(target, region_weight=good)


# ------------------------------------------------------------------------------------------------------------------ drivers and command line
def test_cli_project_and_morph_refine_with_a_region_weight(tmp_path, capsys):
    """`project --mode gradient --region-from-landmarks 1,0.1,2` and `morph --refine --region-weight FILE` end to end at 64^2: the runs differ
    from the un-weighted ones (the best loss each run prints; the best latent of a short run can be step 0's in both)."""
    import re
    from morphganformer_amd import cli, drivers
    from morphganformer_amd.projection import synthetic_landmarks
    from morphganformer_amd.synth_weights import TINY
    from test_host_and_abi import _tiny_snapshot
    pkl = str(tmp_path / "net.pkl")
    _tiny_snapshot(pkl, seed=3)
    assert cli.main(["generate", "--model", pkl, "--output-dir", str(tmp_path / "g"), "--images-num", "2", "--seed", "1"]) == 0
    lm_t, lm_s = synthetic_landmarks(6, 64, 1)
    np.savez(tmp_path / "lm.npz", target=lm_t, steps=lm_s)
    img = str(tmp_path / "g" / "sample_000000.png")
    base = ["project", "--model", pkl, "--image", img, "--landmarks", str(tmp_path / "lm.npz"), "--size", "64", "--step", "6", "--n_mean_latent", "200",
            "--seed", "0", "--mode", "gradient", "--lpips-random-backbone"]
    def best_loss(argv, pattern=r"best step \d+  loss ([0-9.]+)"):
        capsys.readouterr()
        assert cli.main(argv) == 0
        return float(re.search(pattern, capsys.readouterr().out).group(1))

    l0 = best_loss(base + ["--path_to_gen", str(tmp_path / "p0")])
    l1 = best_loss(base + ["--path_to_gen", str(tmp_path / "p1"), "--region-from-landmarks", "1,0.1,2"])
    w1 = drivers.load_latent_mat(str(tmp_path / "p1" / "sample_000000.mat"))
    assert np.isfinite(w1).all() and np.isfinite(l1) and abs(l1 - l0) > 1e-3 * abs(l0)
    # a weight file through `project --region-weight` equals the same weight from the landmarks
    np.save(tmp_path / "w.npy", drivers.face_region_weight(lm_t, 64, 1.0, 0.1, 2.0))
    # (to 1 %, not to the bit: the command line runs with noise_mode="random", whose per-layer noise follows torch's global generator from
    # run to run -- 2e-4 of the loss here, against the 27 % between the weighted and the un-weighted objective)
    l2 = best_loss(base + ["--path_to_gen", str(tmp_path / "p2"), "--region-weight", str(tmp_path / "w.npy")])
    assert abs(l2 - l1) < 1e-2 * abs(l1) and abs(l2 - l0) > 1e-1 * abs(l0)
    rng = np.random.Generator(np.random.PCG64(2))
    for name in ("a", "b"):
        drivers.save_latent_mat(str(tmp_path / f"{name}.mat"), rng.standard_normal((1, TINY.k, TINY.z_dim)).astype(np.float32))
    morph = lambda out: ["morph", "--model", pkl, "--w1", str(tmp_path / "a.mat"), "--w2", str(tmp_path / "b.mat"), "--alphas", "0.5", "--out",
                         str(tmp_path / out / "a+b"), "--refine", "--image-a", img, "--image-b", str(tmp_path / "g" / "sample_000001.png"), "--size", "64",
                         "--step", "6", "--n_mean_latent", "200", "--seed", "0", "--lpips-random-backbone"]
    pat = r"alpha 0.50: best step \d+  loss ([0-9.]+)"
    m0 = best_loss(morph("m0"), pat)
    m1 = best_loss(morph("m1") + ["--region-weight", str(tmp_path / "w.npy")], pat)
    r1 = drivers.load_latent_mat(str(tmp_path / "m1" / "a+b_a0.50_refined.mat"))
    assert np.isfinite(r1).all() and np.isfinite(m1) and abs(m1 - m0) > 1e-3 * abs(m0)


def test_project_many_with_region_weights(golden):
    """project_many(region_weights=): one weight for all items, or one per item -- the same results as project_image item by item."""
    from morphganformer_amd import drivers
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.projection import ProjectionArgs
    from morphganformer_amd.synth_weights import TINY, make_state_dict, synthetic_latents
    g = golden("loop_tiny.npz")
    G = Generator(make_state_dict(TINY, seed=0), TINY, "cuda", max_batch=1)
    targets = [G(torch.from_numpy(synthetic_latents(TINY, 1, 3000 + j)).cuda(), None, noise_mode="const")[0].clamp(-1, 1).clone() for j in range(2)]
    Ws = [weights("half", 64, 64), weights("disc", 64, 64)]
    kw = dict(args=ProjectionArgs(step=8), latent_mean=torch.from_numpy(g["latent_mean"]).cuda(), latent_std=float(g["latent_std"]), seed=3,
              noise_mode="const", batch=4)
    many = drivers.project_many(G, targets, region_weights=Ws, **kw)
    for j in range(2):
        one = drivers.project_image(G, targets[j], None, None, region_weight=Ws[j], **kw)
        assert torch.equal(many["latents"][j:j + 1].cpu(), one["w"]) and float(many["losses"][j]) == one["loss"]
    shared = drivers.project_many(G, targets, region_weights=Ws[0], **kw)
    assert torch.equal(shared["latents"][0], many["latents"][0]) and float(shared["losses"][0]) == float(many["losses"][0])
    assert float(shared["losses"][1]) != float(many["losses"][1])                 # (the best candidate itself can be the same one)
    with pytest.raises(ValueError, match="region weights"):
        drivers.project_many(G, targets, region_weights=Ws[:1], **kw)
