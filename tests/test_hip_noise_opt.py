"""Noise-map optimisation of gradient mode (csrc/noise_opt.hip, GeneratorGrad(dnoises=), GradientProjectionEngine(optimize_noise=True)):
every kernel on its own at small shapes against float64 torch, then the generator's noise gradient against autograd through the CPU
oracle, then the loop against torch autograd + torch.optim.Adam over [latent] + noises + noise_normalize_ (tests/noise_opt_torch_ref.py,
pinned on the reference's own regulariser by tests/test_noise_opt_host.py).

Kernel gates are stated as m x the distance of torch's OWN float32 evaluation from its float64 one on the same input, m = 4, per element
relative to max |float64 result|, with a floor of 4 * 2^-23 (four float32 roundings of the largest element: a kernel that accumulates in
float64 and rounds once can land below torch's float32 error, which is then no yardstick).  Every gate prints both distances (OBS lines)."""
import functools
import os

import numpy as np
import pytest
import torch

from noise_opt_torch_ref import noise_regularize_grad, projection_noise_ref

pytestmark = pytest.mark.gpu

M = 4
FLOOR = 4 * 2.0 ** -23
GRAD_TOL = 1e-3                       # the latent-gradient gate of tests/test_hip_gradient.py


def dist(a, ref):
    """max |a - ref| / max |ref|, in float64 on the CPU."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


def gate(name, got, t32, t64):
    d_hip, d_t32 = dist(got, t64), dist(t32, t64)
    bound = max(M * d_t32, FLOOR)
    print(f"OBS {name}: hip-vs-f64 {d_hip:.3e}  torch32-vs-f64 {d_t32:.3e}  bound {bound:.3e}")
    assert d_hip <= bound, (name, d_hip, bound)


def make_map(side, kind, seed):
    """white: randn (both means ~ 0, the gradient tiny: ill-conditioned, a wrong stencil could pass).  smooth: a 3 x 3 circular box filter
    of randn, renormalised to unit variance: the neighbour means are O(0.5) and every term of the gradient counts."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(side, side, generator=g, dtype=torch.float64)
    if kind == "smooth":
        x = sum(torch.roll(x, (i, j), (0, 1)) for i in (-1, 0, 1) for j in (-1, 0, 1))
        x = (x - x.mean()) / x.std()
    return x.float()


def reg_scratch(L, side):
    return torch.empty(int(L.mgf_noise_regularize_scratch_bytes(side)) // 8, dtype=torch.float64, device="cuda")


# ---------------------------------------------------------------------------------------------- regulariser
@pytest.mark.parametrize("kind", ["white", "smooth"])
@pytest.mark.parametrize("side", [4, 8, 16, 64])
def test_regulariser_value_and_gradient(side, kind):
    """Sides 4 (one level, every neighbour index wraps within two steps), 8 (one level, exactly at the break), 16 (two levels), 64 (four
    levels); value and gradient from one call, the value entry and a repeated call give the same bits."""
    from morphganformer_amd import _lib
    L, st = _lib.lib(), _lib.stream_ptr()
    x = make_map(side, kind, 100 + side)
    scale = 3.0
    v64, g64 = noise_regularize_grad(x, torch.float64)
    v32, g32 = noise_regularize_grad(x, torch.float32)
    xd = x.cuda()
    sc = reg_scratch(L, side)
    dx = torch.full_like(xd, float("nan"))
    val = torch.full([1], float("nan"), device="cuda")
    _lib.check(L.mgf_noise_regularize_grad_f32(dx.data_ptr(), val.data_ptr(), xd.data_ptr(), side, scale, 0, 0, sc.data_ptr(), st))
    gate(f"reg grad {side} {kind}", dx, scale * g32, scale * g64)
    gate(f"reg value(grad entry) {side} {kind}", val, (scale * v32).reshape(1), (scale * v64).reshape(1))
    val2 = torch.full([1], float("nan"), device="cuda")
    _lib.check(L.mgf_noise_regularize_f32(val2.data_ptr(), xd.data_ptr(), side, scale, 0, sc.data_ptr(), st))
    assert torch.equal(val, val2)                                  # the value entry is the same pass
    # deterministic: a second call on fresh scratch gives the same bits
    dx2, val3 = torch.empty_like(dx), torch.empty_like(val)
    sc2 = reg_scratch(L, side)
    _lib.check(L.mgf_noise_regularize_grad_f32(dx2.data_ptr(), val3.data_ptr(), xd.data_ptr(), side, scale, 0, 0, sc2.data_ptr(), st))
    assert torch.equal(dx, dx2) and torch.equal(val, val3)


def test_regulariser_accumulates_onto_a_prior():
    from morphganformer_amd import _lib
    L, st = _lib.lib(), _lib.stream_ptr()
    side, scale = 16, 2.5
    x = make_map(side, "smooth", 7)
    prior = make_map(side, "white", 8) * 0.01
    v64, g64 = noise_regularize_grad(x, torch.float64)
    v32, g32 = noise_regularize_grad(x, torch.float32)
    dx, val, xd, sc = prior.cuda().clone(), torch.tensor([0.75], device="cuda"), x.cuda(), reg_scratch(L, side)
    _lib.check(L.mgf_noise_regularize_grad_f32(dx.data_ptr(), val.data_ptr(), xd.data_ptr(), side, scale, 1, 1, sc.data_ptr(), st))
    gate("reg grad accumulate", dx, prior + (scale * g32), prior.double() + scale * g64)
    gate("reg value accumulate", val, (torch.tensor(0.75) + scale * v32).reshape(1), (0.75 + scale * v64).reshape(1))


def test_regulariser_refuses_sides_it_does_not_take():
    from morphganformer_amd import _lib
    L = _lib.lib()
    t = torch.zeros(64, device="cuda")
    assert int(L.mgf_noise_regularize_scratch_bytes(12)) == 0
    assert L.mgf_noise_regularize_f32(t.data_ptr(), t.data_ptr(), 12, 1.0, 0, t.data_ptr(), _lib.stream_ptr()) != 0
    assert L.mgf_noise_regularize_grad_f32(t.data_ptr(), None, t.data_ptr(), 4, 1.0, 0, 0, t.data_ptr(), _lib.stream_ptr()) != 0     # dx aliases x


# ---------------------------------------------------------------------------------------------- normalise
@pytest.mark.parametrize("side", [4, 64])
def test_normalise(side):
    from morphganformer_amd import _lib
    L, st = _lib.lib(), _lib.stream_ptr()
    x = make_map(side, "white", 40 + side) * 1.7 + 0.3
    t64 = (x.double() - x.double().mean()) / x.double().std()
    t32 = x.clone()
    t32.add_(-t32.mean()).div_(t32.std())                           # noise_normalize_ (:55-60) in float32
    xd = x.cuda()
    sc = torch.empty(int(L.mgf_noise_normalize_scratch_bytes()) // 8, dtype=torch.float64, device="cuda")
    _lib.check(L.mgf_noise_normalize_f32(xd.data_ptr(), side * side, None, None, 0, sc.data_ptr(), st))
    gate(f"normalise {side}", xd, t32, t64)
    assert abs(float(xd.double().mean())) <= 1e-6 and abs(float(xd.double().std(unbiased=True)) - 1.0) <= 1e-6
    # gated: a skipped step (valid = 0) and a step past the end leave the map bit-unchanged, a live one does the same as above
    step = torch.tensor([1], dtype=torch.int32, device="cuda")
    valid = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
    y = x.cuda()
    _lib.check(L.mgf_noise_normalize_f32(y.data_ptr(), side * side, step.data_ptr(), valid.data_ptr(), 3, sc.data_ptr(), st))
    assert torch.equal(y, x.cuda())
    step.fill_(3)
    _lib.check(L.mgf_noise_normalize_f32(y.data_ptr(), side * side, step.data_ptr(), valid.data_ptr(), 3, sc.data_ptr(), st))
    assert torch.equal(y, x.cuda())
    step.fill_(2)
    _lib.check(L.mgf_noise_normalize_f32(y.data_ptr(), side * side, step.data_ptr(), valid.data_ptr(), 3, sc.data_ptr(), st))
    assert torch.equal(y, xd)


# ---------------------------------------------------------------------------------------------- channel sum
@pytest.mark.parametrize("c,hw,acc", [(8, 16, 0), (512, 16, 0), (70, 4096, 1), (5, 67, 0), (130, 67, 1), (33, 70000, 0), (3, 1 << 18, 1)])
def test_noise_grad_channel_sum(c, hw, acc):
    """The 4 x 4 map with few and with many channels, 64^2 with a channel count that leaves the slices ragged, a pixel count that is no
    multiple of 4 (scalar path, both slice forms), more than one block per slice form, and the one-thread-per-pixel-group form (>= 2^16 groups)."""
    from morphganformer_amd import _lib
    L = _lib.lib()
    torch.manual_seed(c + hw)
    d = torch.randn(c, hw)
    prior = torch.randn(hw)
    s = torch.tensor([0.37])
    want64 = (prior.double() if acc else 0) + float(s) * d.double().sum(0)
    t32 = (prior if acc else 0) + s * d.sum(0)
    out = prior.cuda().clone() if acc else torch.full([hw], float("nan"), device="cuda")
    dd, sd = d.cuda(), s.cuda()
    _lib.check(L.mgf_noise_grad_f32(out.data_ptr(), dd.data_ptr(), sd.data_ptr(), c, hw, acc, _lib.stream_ptr()))
    gate(f"noise_grad c={c} hw={hw} acc={acc}", out, t32, want64)


# ---------------------------------------------------------------------------------------------- Adam
def _adam_args(n, seed, steps=4):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (10.0 ** -(i % 3)) for i in range(steps)]
    lr = torch.tensor([0.01, 0.02, 0.03, 0.015][:steps])
    return p, grads, lr


def _run_adam(fn, p, grads, lr, valid=None, weight_decay=0.0):
    from morphganformer_amd import _lib
    n = p.numel()
    pd, m, v = p.cuda().clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    t = torch.zeros(1, dtype=torch.int32, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    lrd = lr.cuda()
    vd = None if valid is None else torch.tensor(valid, dtype=torch.int32, device="cuda")
    snaps = []
    for i, g in enumerate(grads):
        gd = g.cuda()
        _lib.check(fn(pd.data_ptr(), m.data_ptr(), v.data_ptr(), t.data_ptr(), gd.data_ptr(), lrd.data_ptr(), step.data_ptr(), _lib.ptr(vd), n,
                      len(grads), 0.9, 0.999, 1e-8, weight_decay, _lib.stream_ptr()))
        step.add_(1)
        snaps.append((pd.clone(), m.clone(), v.clone(), int(t.item())))
    return snaps


@pytest.mark.parametrize("n", [544, (1 << 20) - 4])
def test_elementwise_adam_is_bit_identical_to_the_single_workgroup_step(n):
    from morphganformer_amd import _lib
    L = _lib.lib()
    p, grads, lr = _adam_args(n, n % 1000, steps=3)
    for wd in (0.0, 1e-4):
        a = _run_adam(L.mgf_adam_step_f32, p, grads, lr, weight_decay=wd)
        b = _run_adam(L.mgf_adam_elementwise_f32, p, grads, lr, weight_decay=wd)
        for (pa, ma, va, ta), (pb, mb, vb, tb) in zip(a, b):
            assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and ta == tb


def test_elementwise_adam_past_the_single_workgroup_limit_matches_torch_adam():
    """2^20 + 12 elements (mgf_adam_step_f32 refuses them) against torch.optim.Adam in float64, with a skipped step in the middle: the
    skipped step leaves parameter, moments and the optimizer's step count untouched."""
    from morphganformer_amd import _lib
    L = _lib.lib()
    n = (1 << 20) + 12
    p, grads, lr = _adam_args(n, 5, steps=4)
    valid = [1, 1, 0, 1]
    t = torch.zeros(1, device="cuda")
    assert L.mgf_adam_step_f32(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), None, n, 4, 0.9,
                               0.999, 1e-8, 0.0, _lib.stream_ptr()) != 0
    snaps = _run_adam(L.mgf_adam_elementwise_f32, p, grads, lr, valid=valid)
    q = p.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=0.01)
    for i, g in enumerate(grads):
        if valid[i]:
            opt.param_groups[0]["lr"] = float(lr[i])
            q.grad = g.double()
            opt.step()
        d = dist(snaps[i][0], q)
        print(f"OBS adam step {i}: {d:.3e}")
        assert d <= 1e-6
    assert [s[3] for s in snaps] == [1, 2, 2, 3]
    assert all(torch.equal(a, b) for a, b in zip(snaps[1][:3], snaps[2][:3]))


# ---------------------------------------------------------------------------------------------- d noise through the generator
@pytest.fixture(scope="module")
def tiny():
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import TINY, make_state_dict
    from oracle.generator_ref import to_torch_state
    sd = make_state_dict(TINY, seed=0)
    return Generator(sd, TINY, "cuda", max_batch=2), to_torch_state(sd), TINY


def _noise_layers(G):
    return [lp for lp in G.plan.layers if lp.noise_strength is not None]


def test_generator_noise_gradient_wrt_z(tiny):
    """Two samples sharing one map per layer (the maps' gradient sums over the samples), every noise layer; conv_last and ToRGB get none."""
    from morphganformer_amd.grad import GeneratorGrad
    from oracle.generator_ref import generator_ref
    G, tsd, cfg = tiny
    gg = GeneratorGrad(G)
    torch.manual_seed(21)
    z = torch.randn(2, cfg.k, cfg.z_dim, requires_grad=True)
    dimg = torch.randn(2, 3, cfg.img_resolution, cfg.img_resolution)
    maps = {lp.name: torch.randn(1, lp.res, lp.res, requires_grad=True) for lp in _noise_layers(G)}
    assert len(maps) == 2 * len(cfg.block_resolutions) - 1
    img_ref = generator_ref(tsd, z, cfg, "inject", maps)
    grads = torch.autograd.grad(img_ref, [z] + list(maps.values()), dimg)
    noises = {k: v.detach().cuda() for k, v in maps.items()}
    dn = {k: torch.full_like(v, float("nan")) for k, v in noises.items()}
    R = cfg.img_resolution
    others = [lp.name for lp in G.plan.layers if lp.noise_strength is None]
    assert f"synthesis.b{R}.conv_last" in others and f"synthesis.b{R}.torgb" in others
    for name in others:
        dn[name] = torch.full([1, R, R], 7.0, device="cuda")
    img = gg.forward(z.detach().cuda(), noise_mode="inject", noises=noises)
    dz = gg.backward(dimg.cuda(), dnoises=dn)
    assert dist(img, img_ref) < 1e-3 and dist(dz, grads[0]) < GRAD_TOL
    for (name, _), ref in zip(maps.items(), grads[1:]):
        d = dist(dn[name], ref)
        print(f"OBS dnoise {name}: {d:.3e}")
        assert d < GRAD_TOL, name
    for name in others:
        assert bool((dn[name] == 7.0).all()), name
    assert gg.noise_grads and not gg._fir_mode


def test_generator_noise_gradient_through_backward_ws(tiny):
    from morphganformer_amd.grad import GeneratorGrad
    from oracle.generator_ref import mapping_ref, synthesis_ref
    G, tsd, cfg = tiny
    gg = GeneratorGrad(G)
    torch.manual_seed(22)
    z = torch.randn(1, cfg.k, cfg.z_dim)
    dimg = torch.randn(1, 3, cfg.img_resolution, cfg.img_resolution)
    ws = (mapping_ref(tsd, z, cfg).detach()[:, :, None, :] + 0.1 * torch.randn(1, cfg.k, cfg.num_ws, cfg.w_dim)).requires_grad_(True)
    maps = {lp.name: torch.randn(1, lp.res, lp.res, requires_grad=True) for lp in _noise_layers(G)}
    img_ref = synthesis_ref(tsd, ws, cfg, "inject", maps)
    grads = torch.autograd.grad(img_ref, [ws] + list(maps.values()), dimg)
    noises = {k: v.detach().cuda() for k, v in maps.items()}
    dn = {k: torch.full_like(v, float("nan")) for k, v in noises.items()}
    gg.forward(ws=ws.detach().cuda(), noise_mode="inject", noises=noises)
    dws = gg.backward_ws(dimg.cuda(), dnoises=dn)
    assert dist(dws, grads[0]) < GRAD_TOL
    for (name, _), ref in zip(maps.items(), grads[1:]):
        assert dist(dn[name], ref) < GRAD_TOL, name


def test_dnoises_none_is_the_call_without_the_keyword(tiny, monkeypatch):
    from morphganformer_amd import _lib
    from morphganformer_amd.grad import GeneratorGrad
    G, tsd, cfg = tiny
    gg = GeneratorGrad(G)
    torch.manual_seed(23)
    z = torch.randn(1, cfg.k, cfg.z_dim, device="cuda")
    img = gg.forward(z, noise_mode="const")
    dimg = torch.sin(img * 3.0)
    a = gg.backward(dimg).clone()
    calls = _count_calls(monkeypatch, ["mgf_noise_grad_f32"])
    b = gg.backward(dimg, dnoises=None).clone()
    assert torch.equal(a, b) and calls["mgf_noise_grad_f32"] == 0 and not gg.noise_grads and gg._fir_mode


NEW_CALLS = ["mgf_noise_grad_f32", "mgf_noise_regularize_f32", "mgf_noise_regularize_grad_f32", "mgf_noise_normalize_f32",
             "mgf_adam_elementwise_f32", "mgf_noise_regularize_scratch_bytes", "mgf_noise_normalize_scratch_bytes",
             "mgf_noise_sets_scratch_bytes", "mgf_noise_sets_regularize_grad_f32", "mgf_noise_sets_normalize_f32", "mgf_noise_sets_grad_f32",
             "mgf_noise_sets_pack_f32", "mgf_adam_sets_f32"]


class _Counting:
    """A stand-in for the loaded library that counts the calls of the named entries and passes everything on."""

    def __init__(self, lib, names):
        self._lib, self.counts = lib, {n: 0 for n in names}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name in self.counts:
            def counted(*a, _fn=fn, _name=name):
                self.counts[_name] += 1
                return _fn(*a)
            return counted
        return fn


def _count_calls(monkeypatch, names):
    """Wrap the library handle every caller gets from _lib.lib() for the rest of the test; returns the live {entry: calls} dict."""
    from morphganformer_amd import _lib
    proxy = _Counting(_lib.lib(), names)
    monkeypatch.setattr(_lib, "_lib", proxy)
    return proxy.counts


# ---------------------------------------------------------------------------------------------- the loop
STEPS, LR = 10, 0.05
SKIPPED = 3
# Adam's epsilon in the loop tests.  Adam moves an element by lr * m / (sqrt(v) + eps): with torch's default 1e-8 an element whose gradient lies
# within float32 rounding of zero takes a rounding-dependent share of a full lr step, and the gate (0.05 lr per step) then measures rounding luck:
# the 64^2 maps' gradients are ~5e-5 (median; 5e-4 max) and the float32 generator backward is good to ~2e-5 of the max, i.e. 1e-8 absolute -- the
# default eps -- and about one of their 4096 elements per step lies inside that band (the CPU oracle's own float32 run drifts 0.47 lr from its
# float64 run by step 9).  eps = 1e-6 is 100 x that error and 2 % of the median gradient: Adam still normalises, and a gradient error of 1e-8 moves
# an element by at most 0.01 lr.  Engine and oracle get the same value; the default (1e-8) is what the kernel tests above run with.
ADAM_EPS = 1e-6


@functools.lru_cache(maxsize=None)
def _loop_case(objective, noise_init, dtype=torch.float64):
    """Inputs and the CPU oracle run of one loop case, computed once per session and read-only afterwards.  The synthesis network, the
    losses and the maps of the oracle run in float64 on the float32 inputs, so that the trajectory gate is spent on the engine's rounding
    and not on the reference's own (`dtype=torch.float32` gives the all-float32 oracle, for comparison by hand)."""
    from morphganformer_amd.lpips import WEIGHTS_DIR
    from morphganformer_amd.projection import ProjectionArgs, synthetic_landmarks
    from morphganformer_amd.synth_weights import TINY as cfg, make_state_dict, synthetic_latents
    from oracle.generator_ref import generator_ref, mapping_ref, synthesis_ref, to_torch_state
    from oracle.loss_ref import backbone_random, lpips_ref, mse_ref, wing_loss_ref
    sd = make_state_dict(cfg, seed=0)
    tsd32 = to_torch_state(sd)
    tsd = {k: v.to(dtype) for k, v in tsd32.items()}
    rng = np.random.Generator(np.random.PCG64(31))
    latent_mean = torch.from_numpy(rng.standard_normal((cfg.k, cfg.z_dim)).astype(np.float32))
    eps = torch.from_numpy(rng.standard_normal((STEPS, 1, cfg.k, cfg.z_dim)).astype(np.float32))
    target = generator_ref(tsd32, torch.from_numpy(synthetic_latents(cfg, 1, 1001)), cfg, "const").clamp(-1, 1)
    tgt = target.to(dtype)
    lm_t, lm_s = synthetic_landmarks(STEPS, 64, 9)
    valid = np.ones(STEPS, np.int32)
    valid[SKIPPED] = 0
    args = ProjectionArgs(step=STEPS, lr=LR, lr_rampup=0.2, noise_regularize=REG_WEIGHT[objective])
    names = [k[:-len(".noise_strength")] for k in sd if k.endswith(".noise_strength")]
    if noise_init == "const":
        start = {k: tsd32[k + ".noise_const"].detach().clone().reshape(1, *tsd32[k + ".noise_const"].shape[-2:]) for k in names}
    else:
        g = torch.Generator().manual_seed(77)
        start = {k: torch.randn(1, *tsd32[k + ".noise_const"].shape[-2:], generator=g) for k in names}
    if objective == "mse":
        loss_fn = lambda i, img: None if not valid[i] else args.beta * mse_ref(img, tgt)
    else:
        bb = {k: v.to(dtype) for k, v in backbone_random("squeeze", 0).items()}
        lin = np.load(os.path.join(WEIGHTS_DIR, "lpips_lin_squeeze.npz"))
        lins = [torch.from_numpy(lin[f"lin{i}"]).to(dtype).reshape(-1) for i in range(7)]

        def loss_fn(i, img):
            if not valid[i]:
                return None
            w = wing_loss_ref(torch.from_numpy(lm_s[i]), torch.from_numpy(lm_t))
            return lpips_ref(bb, lins, img, tgt).sum() + args.lamda * w + args.beta * mse_ref(img, tgt)

    # (the oracle's mapping network is float32 by construction -- it casts its input -- so the latent and its 544-element path stay float32
    # on both sides; the synthesis network, the losses and the maps run in `dtype`)
    gen_fn = lambda z, maps: synthesis_ref(tsd, mapping_ref(tsd32, z, cfg).to(dtype), cfg, "inject", maps)
    ref = projection_noise_ref(gen_fn, loss_fn, latent_mean, 1.0, eps, {k: v.to(dtype) for k, v in start.items()}, STEPS, args.noise_regularize,
                               lr=args.lr, rampdown=args.lr_rampdown, rampup=args.lr_rampup, adam_eps=ADAM_EPS)
    return dict(cfg=cfg, sd=sd, latent_mean=latent_mean, eps=eps, target=target, lm_t=lm_t, lm_s=lm_s, valid=valid, args=args, start=start, ref=ref)


# The regulariser's weight in the loop tests.  The drivers' 1e5 is sized for 1024^2 maps, whose regulariser is ~1e-6; on the TINY generator's
# nine maps (4^2 .. 64^2) the CPU oracle gives, at step 0: seeded N(0, 1) maps, regulariser 0.089 against an MSE of 2.4 -- weight 10 makes
# it a quarter of the total; the layers' noise_const maps, 0.50 against LPIPS + Wing + MSE = 2.5 -- weight 4 makes it 45 %.  The share is
# asserted below on the oracle's own figures.
REG_WEIGHT = {"mse": 10.0, "lpips": 4.0}


def _engine(case, objective, noise_init, use_graph, G):
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine
    kw = dict(lm_valid=case["valid"], eps=case["eps"].cuda(), noise_mode="const", use_graph=use_graph, optimize_noise=True, noise_init=noise_init,
              adam_eps=ADAM_EPS)
    if objective == "lpips":
        kw.update(percept=PerceptualLoss(net="squeeze", allow_random_backbone=True), lm_target=case["lm_t"], lm_steps=case["lm_s"])
    eng = GradientProjectionEngine(G, case["target"].cuda(), case["latent_mean"].cuda(), 1.0, case["args"], **kw)
    if noise_init == "randn":          # the engine's own seeded draw is a device stream: the comparison runs on the oracle's start maps
        for k, v in case["start"].items():
            eng.noises[k].copy_(v)
    return eng


def _run(eng):
    traj, ntraj, imgs = [], [], []
    for i in range(STEPS):
        eng.run(1)
        traj.append(eng.latent_in.cpu().clone())
        ntraj.append({k: v.cpu().clone() for k, v in eng.noises.items()})
        imgs.append(eng.G.img.clone())
    return traj, ntraj, imgs


@pytest.mark.parametrize("objective,noise_init,use_graph", [("mse", "randn", True), ("mse", "randn", False), ("lpips", "const", True)])
def test_noise_projection_matches_autograd_adam(tiny, objective, noise_init, use_graph):
    """The loop with optimize_noise against autograd + Adam over [latent] + maps + noise_normalize_ on the CPU: MSE + regulariser (seeded
    N(0, 1) start maps; hipGraph replay and eager) and LPIPS(squeeze, random backbone) + Wing + MSE + regulariser (maps started from the
    layers' noise_const), a skipped ("no face") step, injected eps.  Gates of test_gradient_projection_matches_autograd_adam."""
    G, tsd, cfg = tiny
    case = _loop_case(objective, noise_init)
    ref, args = case["ref"], case["args"]
    eng = _engine(case, objective, noise_init, use_graph, G)
    if noise_init == "const":
        for k, v in case["start"].items():
            assert torch.equal(eng.noises[k].cpu(), v), k
    traj, ntraj, imgs = _run(eng)
    lat, bstep, bloss, losses = eng.result()
    # the oracle run is no no-op: latent and maps moved, and the regulariser is a visible share of the total
    assert float((ref["traj"][-1] - case["latent_mean"]).abs().max()) > 5 * args.lr * 0.2
    for k, v in case["start"].items():
        assert float((ref["noise_traj"][-1][k] - v).abs().max()) > 5 * args.lr * 0.2, k
    share = ref["reg"][0] / ref["losses"][0]
    print(f"OBS regulariser share of the total at step 0: {share:.3f} (total {ref['losses'][0]:.4f})")
    assert 0.1 < share < 0.9
    for i in range(STEPS):
        bound = 0.05 * args.lr * (i + 1)
        assert float((traj[i] - ref["traj"][i]).abs().max()) < bound, i
        for k in case["start"]:
            assert float((ntraj[i][k] - ref["noise_traj"][i][k]).abs().max()) < bound, (i, k)
    # the skipped step moved nothing
    assert torch.equal(traj[SKIPPED], traj[SKIPPED - 1])
    assert all(torch.equal(ntraj[SKIPPED][k], ntraj[SKIPPED - 1][k]) for k in case["start"])
    got = np.array([v for v in losses if not np.isnan(v)])
    want = np.array([v for v in ref["losses"] if v is not None])
    assert np.isnan(losses[SKIPPED]) and ref["losses"][SKIPPED] is None
    assert np.abs(got - want).max() < 1e-3 * np.abs(want).max()
    assert bstep == ref["best_step"] and bstep > 0
    assert float((lat - ref["best_latent"]).abs().max()) < 0.05 * args.lr * STEPS
    # best_noises: the maps the best step's image was generated with, i.e. as they stood BEFORE that step's update
    for k in case["start"]:
        before = ntraj[bstep - 1][k]
        assert torch.equal(eng.best_noises[k].cpu(), before), k
        assert float((eng.best_noises[k].cpu() - ref["best_noises"][k]).abs().max()) < 0.05 * args.lr * (bstep + 1), k
        assert not torch.equal(ntraj[bstep][k], before), k
    # G(best_latent, noises = best_noises) is the scored image: bit for bit through the same forward, and through the plain generator
    again = eng.gg.forward(lat.cuda(), noise_mode="inject", noises=eng.best_noises)
    assert torch.equal(again, imgs[bstep])
    plain = G.forward_workspace(lat.cuda(), None, noise_mode="inject", noises=eng.best_noises)[0]
    assert dist(plain, imgs[bstep]) < 1e-4


def test_graph_and_eager_give_the_same_trajectory(tiny):
    G, tsd, cfg = tiny
    case = _loop_case("mse", "randn")
    runs = []
    for use_graph in (True, False):
        eng = _engine(case, "mse", "randn", use_graph, G)
        traj, ntraj, _ = _run(eng)
        runs.append((traj, ntraj, eng.result()))
    for i in range(STEPS):
        assert torch.equal(runs[0][0][i], runs[1][0][i]), i
        assert all(torch.equal(runs[0][1][i][k], runs[1][1][i][k]) for k in runs[0][1][i]), i
    assert runs[0][2][1] == runs[1][2][1] and np.array_equal(runs[0][2][3], runs[1][2][3], equal_nan=True)


def test_wplus_with_noise_optimisation_runs_and_moves_the_maps(tiny):
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, mapping_only
    G, tsd, cfg = tiny
    case = _loop_case("mse", "randn")
    w_mean = mapping_only(G, case["latent_mean"][None].cuda())[0]
    args = ProjectionArgs(step=4, lr=LR, lr_rampup=0.2, noise_regularize=1.0)
    eng = GradientProjectionEngine(G, case["target"].cuda(), w_mean, 1.0, args, noise_mode="const", use_graph=True, latent_space="w+",
                                   optimize_noise=True, seed=3)
    start = {k: v.clone() for k, v in eng.noises.items()}
    lat, bstep, bloss, losses = eng.run().result()
    assert tuple(lat.shape) == (1, cfg.k, cfg.num_ws, cfg.w_dim) and np.isfinite(losses).all()
    for k, v in eng.noises.items():
        assert not torch.equal(v, start[k]) and abs(float(v.double().mean())) < 1e-6 and abs(float(v.double().std()) - 1) < 1e-6, k
    assert any(bool(v.abs().max() > 0) for v in eng.best_noises.values())
    eng.rewind()
    assert int(eng.step_ctr.item()) == 0 and int(eng.noise_slot.count.item()) == 0 and all(not bool(v.any()) for v in eng.best_noises.values())


# ---------------------------------------------------------------------------------------------- refusals, defaults, CLI
def test_lockstep_targets_with_noise_optimisation_are_refused(tiny):
    from morphganformer_amd import _lib
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    G, tsd, cfg = tiny
    case = _loop_case("mse", "randn")
    tg = case["target"].cuda().expand(2, -1, -1, -1).contiguous()
    with pytest.raises(_lib.MgfError, match="optimize_noise runs with one target per engine"):
        GradientProjectionEngine(G, tg, case["latent_mean"].cuda(), 1.0, ProjectionArgs(step=2), optimize_noise=True)
    with pytest.raises(ValueError, match="noise_init"):
        GradientProjectionEngine(G, case["target"].cuda(), case["latent_mean"].cuda(), 1.0, ProjectionArgs(step=2), noise_init="zeros")


def test_default_engine_makes_none_of_the_new_calls(tiny, monkeypatch):
    from morphganformer_amd import _lib
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    G, tsd, cfg = tiny
    case = _loop_case("mse", "randn")
    counts = _count_calls(monkeypatch, NEW_CALLS)
    for use_graph in (False, True):
        eng = GradientProjectionEngine(G, case["target"].cuda(), case["latent_mean"].cuda(), 1.0, ProjectionArgs(step=3, lr=LR), eps=case["eps"][:3].cuda(),
                                       noise_mode="const", use_graph=use_graph)
        eng.run().result()
        assert eng.noises is None and eng.best_noises is None and not eng.gg.noise_grads
    assert counts == {n: 0 for n in NEW_CALLS}
    # ... and the counter does count: the same run with the switch on, one eager step (one target is a set of one: one set call each)
    GradientProjectionEngine(G, case["target"].cuda(), case["latent_mean"].cuda(), 1.0, ProjectionArgs(step=3, lr=LR, noise_regularize=1.0),
                             eps=case["eps"][:3].cuda(), use_graph=False, optimize_noise=True).run(1)
    nmaps = len(_noise_layers(G))
    assert counts["mgf_noise_grad_f32"] == nmaps
    assert counts["mgf_noise_sets_regularize_grad_f32"] == counts["mgf_noise_sets_normalize_f32"] == counts["mgf_adam_sets_f32"] == 1
    assert counts["mgf_noise_sets_pack_f32"] == counts["mgf_noise_sets_grad_f32"] == 0
    assert counts["mgf_noise_regularize_f32"] == counts["mgf_noise_regularize_grad_f32"] == 0
    assert counts["mgf_noise_normalize_f32"] == counts["mgf_adam_elementwise_f32"] == 0


def test_cli_project_with_optimised_noise_writes_the_maps(tmp_path):
    import scipy.io as sio
    from morphganformer_amd import cli, drivers
    from test_host_and_abi import _tiny_snapshot
    pkl = str(tmp_path / "net.pkl")
    _tiny_snapshot(pkl, seed=3)
    assert cli.main(["generate", "--model", pkl, "--output-dir", str(tmp_path / "g"), "--images-num", "1", "--seed", "1"]) == 0
    img = str(tmp_path / "g" / "sample_000000.png")
    argv = ["project", "--model", pkl, "--image", img, "--path_to_gen", str(tmp_path / "p"), "--size", "64", "--step", "4", "--n_mean_latent", "200",
            "--seed", "0", "--no-lpips", "--optimize-noise", "--noise-init", "const", "--noise_regularize", "1"]
    with pytest.raises(SystemExit, match="--optimize-noise is for project --mode gradient"):
        cli.main(argv)
    assert cli.main(argv + ["--mode", "gradient"]) == 0
    files = sorted(os.listdir(tmp_path / "p"))
    assert len([f for f in files if f.endswith(".png")]) == 1 and [f for f in files if f.endswith(".mat")] == ["sample_000000.mat"]
    m = sio.loadmat(str(tmp_path / "p" / "sample_000000.mat"))
    keys = sorted(k for k in m if k.startswith("noise_"))
    assert drivers.noise_mat_key("synthesis.b4.conv1") in keys and len(keys) == 9 and m["noise_b64_conv1"].shape == (64, 64)
    assert m["w"].ndim == 3 and np.isfinite(m["noise_b64_conv1"]).all() and float(m["noise_b64_conv1"].std()) > 0.5
