"""The MDF objective's backward pass on MI355X (csrc/mdf.hip, the masked form-3 Winograd epilogue of csrc/wino3.hip, MDFLoss(differentiable=True)):
each new kernel against float64, the gradient against the reference's own (tests/golden/mdf_grad_tiny.npz) and float64 autograd up to
1024^2, batch invariance and determinism, autograd through `forward`, GradientProjectionEngine(mdf=) against torch autograd + Adam, and
the CLI's gradient mode."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

from test_mdf_grad_host import GOLDEN_GRAD, ring  # noqa: E402
from test_mdf_host import GOLDEN, mdf_taps64  # noqa: E402

SLOPE = 0.2
# gradient gates against float64 autograd: float32 against float64 flips the LeakyReLU slope (1 vs 0.2) wherever a pre-activation rounds
# across 0, and such isolated kinks set the error.  The reference's own float32 gradient sits at relative L2 1.5e-4 / max 1.8e-3 of max|g|
# from float64 on tests/golden/mdf_grad_tiny.npz (test_mdf_grad_host); this build's observed values are printed ("OBS") by the tests
GATE_L2, GATE_MAX = 5e-4, 1e-2
FRAMES = [(11, 11), (13, 12), (23, 31), (64, 64), (16, 1024)]


def _L():
    from morphganformer_amd import _lib
    return _lib, _lib.lib()


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def _dl(a):
    return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, SLOPE))


def _adj(w):
    from morphganformer_amd.mdf import adjoint_weights
    return torch.as_tensor(adjoint_weights(w.double().cpu().numpy()), device="cuda")


def _check_ring(got, ref, r, tol=2e-5):
    """got == ref (relative to max|ref|) on ring r, exactly 0 outside it."""
    h, w = got.shape[-2:]
    m = ring(h, w, r, "cuda").bool()
    assert torch.isfinite(got).all()
    assert bool((got[..., ~m] == 0).all()), "values outside the ring must be exactly 0"
    err = float((got.double() - ref)[..., m].abs().max() / ref[..., m].abs().max())
    assert err <= tol, err


# ------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("c", [32, 64, 128])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("hw", FRAMES)
def test_tail_backward_against_float64(c, n, hw):
    _lib, L = _L()
    h, w = hw
    x2 = _rand((n, c, h, w), 1).cuda()
    x2t = _rand((c, h, w), 2).cuda()
    x3 = _rand((n, h, w), 3).cuda()
    x3t = _rand((h, w), 4).cuda()
    r5 = ring(h, w, 5, "cuda").bool()
    x3[:, ~r5] = float("nan")                     # x3 holds values on ring 5 only: nothing outside may be read
    x3t[~r5] = float("nan")
    wt = _rand((1, c, 3, 3), 5, 0.2).cuda()
    d3 = torch.full((n, c, h, w), float("nan"), device="cuda")
    c2, c3 = 0.37, 1.9
    _lib.check(L.mgf_mdf_tail_backward_f32(d3.data_ptr(), x2.data_ptr(), x2t.data_ptr(), x3.data_ptr(), x3t.data_ptr(), wt.data_ptr(), n, c, h, w,
                                           4, c2, c3, SLOPE, _lib.stream_ptr()))
    g3 = torch.where(r5, c3 * (x3.double() - x3t.double()), torch.zeros((), dtype=torch.float64, device="cuda"))
    ref = (F.conv2d(g3[:, None], _adj(wt), padding=1) + c2 * (x2.double() - x2t.double())) * _dl(x2.double())
    _check_ring(d3, ref, 4)


@pytest.mark.parametrize("c", [32, 64, 128])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("hw", FRAMES)
def test_masked_body_adjoint_against_float64(c, n, hw):
    from morphganformer_amd import conv as cv
    _lib, L = _L()
    h, w = hw
    r = {32: 1, 64: 2, 128: 3}[c]
    g = _rand((n, c, h, w), 6).cuda() * ring(h, w, r + 1, "cuda").float()        # the incoming gradient lives on ring r + 1
    a = _rand((n, c, h, w), 7).cuda()
    W = _rand((c, c, 3, 3), 8, (2.0 / (9 * c)) ** 0.5).cuda()
    u = cv.winograd2_weights(_adj(W).float())
    d = torch.full((n, c, h, w), float("nan"), device="cuda")
    _lib.check(L.mgf_mdf_body_backward_f32(d.data_ptr(), g.data_ptr(), u.data_ptr(), a.data_ptr(), n, c, h, w, r, SLOPE, _lib.stream_ptr()))
    ref = F.conv2d(g.double(), _adj(W), padding=1) * _dl(a.double())
    _check_ring(d, ref, r)
    if n > 1:                                      # the batch-invariant dispatch: a sample's bits do not depend on the batch
        d1 = torch.empty(1, c, h, w, device="cuda")
        g1, a1 = g[n - 1:].contiguous(), a[n - 1:].contiguous()
        _lib.check(L.mgf_mdf_body_backward_f32(d1.data_ptr(), g1.data_ptr(), u.data_ptr(), a1.data_ptr(), 1, c, h, w, r, SLOPE, _lib.stream_ptr()))
        assert torch.equal(d1[0], d[n - 1])


@pytest.mark.parametrize("c", [32, 64, 128])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("hw", FRAMES)
def test_head_backward_against_float64(c, n, hw):
    _lib, L = _L()
    h, w = hw
    r1 = ring(h, w, 1, "cuda")
    d0m = _rand((n, c, h, w), 9).cuda() * r1.float()
    x1 = _rand((n, c, h, w), 10).cuda()
    x1t = _rand((c, h, w), 11).cuda()
    W = _rand((c, 3, 3, 3), 12, 0.3).cuda()
    wc = W.reshape(c, 27).contiguous()
    base = _rand((n, 3, h, w), 13).cuda()
    c1 = 0.61
    d0 = (d0m.double() + c1 * (x1.double() - x1t.double()) * _dl(x1.double())) * r1
    ref = F.conv2d(d0, _adj(W), padding=1)
    for acc in (0, 1):
        dimg = base.clone()
        _lib.check(L.mgf_mdf_head_backward_f32(dimg.data_ptr(), d0m.data_ptr(), x1.data_ptr(), x1t.data_ptr(), wc.data_ptr(), n, c, h, w, c1,
                                               SLOPE, acc, _lib.stream_ptr()))
        want = ref + (base.double() if acc else 0)
        err = float((dimg.double() - want).abs().max() / ref.abs().max())
        assert err <= 2e-5, (acc, err)


# ------------------------------------------------------------------------------------------------------------ MDFLoss
def _grad64_gpu(Ds, order, t, y):
    """d/dy of the batch mean of sum over the discriminators and taps of mean((D(y_i)_t - D(t)_t)^2): float64 autograd on the device."""
    yy = y.cuda().double().requires_grad_()
    tot = 0.0
    for i in order:
        sd = {k: torch.as_tensor(v, dtype=torch.float64, device="cuda") for k, v in Ds[i].items()}
        with torch.no_grad():
            tx = mdf_taps64(sd, t.cuda().double())
        ty = mdf_taps64(sd, yy)
        tot = tot + sum(((ty[k] - tx[k]) ** 2).mean(dim=(1, 2, 3)).sum() for k in range(3))
    (tot / y.shape[0]).backward()
    return yy.grad


def _gate(got, ref, what):
    got, ref = got.double().to(ref.device), ref.double()
    rel, mx = float((got - ref).norm() / ref.norm()), float((got - ref).abs().max() / ref.abs().max())
    print(f"OBS {what}: relative L2 {rel:.3e}, max |diff| / max |g| {mx:.3e}")
    return rel, mx


@pytest.mark.parametrize("case", ["asc8", "asc5", "desc9"])
def test_gradient_matches_reference_fixture(case):
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    g, gg = np.load(GOLDEN), np.load(GOLDEN_GRAD)
    seed, nd, scales, asc = (int(v) for v in g[f"{case}_cfg"])
    Ds = random_discriminators(seed, (32,) * 4 + (64,) * 4 + ((128,) if nd == 9 else ()))
    crit = MDFLoss(Ds, num_scales=scales, is_ascending=asc, differentiable=True)
    x = torch.from_numpy(g["target"]).cuda()
    y = torch.from_numpy(g["candidates"]).cuda().requires_grad_()
    loss = crit(x, y)
    loss.backward()
    assert abs(float(loss) - float(gg[f"{case}_mean"])) <= 1e-5 * float(gg[f"{case}_mean"])
    # the reference is float32 (LeakyReLU kinks flip against float64 where a pre-activation rounds across 0): see test_mdf_grad_host
    rel, mx = _gate(y.grad, torch.from_numpy(gg[f"{case}_grad"]), f"fixture {case}")
    assert rel <= 5e-4 and mx <= 5e-3
    order = [i if asc else len(Ds) - 1 - i for i in range(scales)]
    rel, mx = _gate(y.grad, _grad64_gpu(Ds, order, x.cpu(), y.detach().cpu()), f"float64 {case}")
    assert rel <= GATE_L2 and mx <= GATE_MAX


@pytest.mark.parametrize("res,n,scales,asc", [(64, 3, 8, 1), (256, 2, 8, 0), (256, 1, 6, 1), (1024, 1, 8, 1)])
def test_gradient_against_float64(res, n, scales, asc):
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    Ds = random_discriminators(5)
    t = torch.tanh(_rand((1, 3, res, res), 50 + res))
    y = (t + 0.3 * _rand((n, 3, res, res), 51 + res)).clamp(-1, 1)
    crit = MDFLoss(Ds, num_scales=scales, is_ascending=asc, differentiable=True)
    crit.set_target(t.cuda())
    yc = y.cuda()
    dimg = torch.full_like(yc, float("nan"))
    out = torch.zeros(n, device="cuda")
    crit.distance_into(out, yc, dimg=dimg)
    order = [i if asc else len(Ds) - 1 - i for i in range(scales)]
    rel, mx = _gate(dimg, _grad64_gpu(Ds, order, t, y) * n, f"{res}^2 n={n} scales={scales} asc={asc}")
    assert rel <= GATE_L2 and mx <= GATE_MAX


@pytest.mark.parametrize("res", [64, 256])
def test_gradient_batch_invariant_deterministic_and_loss_bits(res):
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    crit = MDFLoss(random_discriminators(1), differentiable=True)
    lit = MDFLoss(random_discriminators(1))
    t = torch.tanh(_rand((1, 3, res, res), 60))
    y = (t + 0.3 * _rand((4, 3, res, res), 61)).clamp(-1, 1).cuda()
    crit.set_target(t.cuda())
    lit.set_target(t.cuda())
    g4, g4b = torch.empty_like(y), torch.empty_like(y)
    l4, l4b, l_plain, l_lit = (torch.zeros(4, device="cuda") for _ in range(4))
    crit.distance_into(l4, y, scale=0.5, dimg=g4)
    crit.distance_into(l4b, y, scale=0.5, dimg=g4b)
    crit.distance_into(l_plain, y, scale=0.5)
    lit.distance_into(l_lit, y, scale=0.5)
    assert torch.equal(g4, g4b) and torch.equal(l4, l4b)
    assert torch.equal(l4, l_plain) and torch.equal(l4, l_lit), "the loss is the same bits with and without the backward"
    for i in (0, 3):
        g1 = torch.empty(1, 3, res, res, device="cuda")
        l1 = torch.zeros(1, device="cuda")
        crit.distance_into(l1, y[i:i + 1].contiguous(), scale=0.5, dimg=g1)
        assert torch.equal(g1[0], g4[i]) and torch.equal(l1[0], l4[i])
    # grad_accumulate adds onto what is there
    acc = torch.ones_like(y)
    crit.distance_into(l4b, y, scale=0.5, dimg=acc, grad_accumulate=True)
    assert torch.allclose(acc - 1, g4, rtol=0, atol=2e-6)        # (a few ulps of the 1 it was added onto)


def test_forward_autograd_and_detached_without_flag():
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    Ds = random_discriminators(2)
    t = torch.tanh(_rand((2, 3, 64, 64), 70))
    y = (t + 0.3 * _rand((2, 3, 64, 64), 71)).clamp(-1, 1)
    crit = MDFLoss(Ds, num_scales=4, differentiable=True)
    yc = y.cuda().requires_grad_()
    loss = crit(t.cuda(), yc)                      # paired targets: loss(x[i], y[i]) averaged
    (3.0 * loss).backward()
    ref = torch.zeros(2, 3, 64, 64, dtype=torch.float64, device="cuda")
    for i in range(2):
        ref[i:i + 1] = _grad64_gpu(Ds, range(4), t[i:i + 1], y[i:i + 1]) / 2
    rel, mx = _gate(yc.grad, 3.0 * ref, "forward paired")
    assert rel <= GATE_L2 and mx <= GATE_MAX
    plain = MDFLoss(Ds, num_scales=4)
    out = plain(t[:1].cuda(), y.cuda().requires_grad_())
    assert not out.requires_grad and out.grad_fn is None
    assert float(out) == float(crit(t[:1].cuda(), y.cuda()))


# ------------------------------------------------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def tiny():
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import TINY, make_state_dict
    from oracle.generator_ref import to_torch_state
    sd = make_state_dict(TINY, seed=0)
    return Generator(sd, TINY, "cuda", max_batch=2), to_torch_state(sd), TINY


ENGINE_DS = dict(seed=2, nfc=(32, 32, 64))


def _mdf64_loss(Ds, target):
    sds = [{k: torch.as_tensor(v, dtype=torch.float64) for k, v in sd.items()} for sd in Ds]
    with torch.no_grad():
        tt = [mdf_taps64(sd, target.double()) for sd in sds]

    def loss(img):
        tot = 0.0
        for sd, tx in zip(sds, tt):
            ty = mdf_taps64(sd, img.double())
            tot = tot + sum(((ty[k] - tx[k]) ** 2).mean() for k in range(3))
        return tot
    return loss


def _engine_case(tiny, space, lpips, use_graph=True, steps=8):
    from morphganformer_amd.lpips import PerceptualLoss, WEIGHTS_DIR
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    from morphganformer_amd.synth_weights import synthetic_latents
    from oracle.generator_ref import generator_ref, mapping_ref, synthesis_ref
    from oracle.loss_ref import backbone_random, lpips_ref
    G, tsd, cfg = tiny
    rng = np.random.Generator(np.random.PCG64(21))
    target = generator_ref(tsd, torch.from_numpy(synthetic_latents(cfg, 1, 1001)), cfg, "const").clamp(-1, 1)
    Ds = random_discriminators(**ENGINE_DS)
    mdf64 = _mdf64_loss(Ds, target)
    if lpips:
        bb = backbone_random("squeeze", 0)
        lin = np.load(os.path.join(WEIGHTS_DIR, "lpips_lin_squeeze.npz"))
        lins = [torch.from_numpy(lin[f"lin{i}"]).float().reshape(-1) for i in range(7)]
        loss_fn = lambda i, img: lpips_ref(bb, lins, img, target).sum() + mdf64(img).float()
    else:
        loss_fn = lambda i, img: mdf64(img).float()
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.2, min_loss_init=1000.0)
    if space == "z":
        start = torch.from_numpy(rng.standard_normal((cfg.k, cfg.z_dim)).astype(np.float32))
        eps = torch.from_numpy(rng.standard_normal((steps, 1, cfg.k, cfg.z_dim)).astype(np.float32))
        std, mean, gen_fn = 1.0, start, (lambda z: generator_ref(tsd, z, cfg, "const"))
    else:
        mean = mapping_ref(tsd, torch.from_numpy(synthetic_latents(cfg, 1, 77)), cfg)[0].detach()
        eps = torch.from_numpy(rng.standard_normal((steps, 1, cfg.k, cfg.num_ws, cfg.w_dim)).astype(np.float32))
        std, gen_fn = float(mean.std()) * 4, (lambda ws: synthesis_ref(tsd, ws, cfg, "const"))
        start = mean[:, None, :].expand(cfg.k, cfg.num_ws, cfg.w_dim).contiguous()
    pl = PerceptualLoss(net="squeeze", allow_random_backbone=True) if lpips else None
    crit = MDFLoss(Ds, num_scales=len(Ds), differentiable=True)
    eng = GradientProjectionEngine(G, target.cuda(), mean.cuda(), std, args, percept=pl, use_mse=False, eps=eps.cuda(), noise_mode="const",
                                   use_graph=use_graph, latent_space="w+" if space == "w+" else "z", mdf=crit)
    return eng, args, start, std, eps, gen_fn, loss_fn


@pytest.mark.parametrize("space,lpips", [("z", False), ("z", True), ("w+", False), ("w+", True)])
def test_gradient_engine_matches_autograd_adam(tiny, space, lpips):
    from oracle.loss_ref import projection_gradient_ref
    eng, args, start, std, eps, gen_fn, loss_fn = _engine_case(tiny, space, lpips)
    steps = args.step
    ref = projection_gradient_ref(gen_fn, loss_fn, start, std, eps, steps, lr=args.lr, rampdown=args.lr_rampdown, rampup=args.lr_rampup,
                                  min_loss_init=args.min_loss_init)
    traj = []
    for i in range(steps):
        eng.run(1)
        traj.append(eng.latent_in.cpu().clone())
    lat, bstep, bloss, losses = eng.result()
    assert float((ref[4][-1] - start).abs().max()) > 5 * args.lr * 0.2, "the oracle run must actually move the latent"
    for i in range(steps):
        assert float((traj[i] - ref[4][i]).abs().max()) < 0.05 * args.lr * (i + 1), i
    want = np.array(ref[3])
    print(f"OBS engine {space} lpips={lpips}: losses max rel {np.abs(losses - want).max() / np.abs(want).max():.3e}")
    # (the per-step gradient is checked teacher-forced below; over the run float32 kink flips are amplified by Adam: observed up to 1.1e-3)
    assert np.abs(losses - want).max() < 5e-3 * np.abs(want).max()
    assert bstep == ref[1]


@pytest.mark.parametrize("space", ["z", "w+"])
def test_gradient_engine_teacher_forced_step(tiny, space):
    """One Adam step with lr > 0 from the engine's own state (step 1; step 0 has lr = 0 under the ramp-up): the latent update against
    torch's gradient through the CPU restatement and the same Adam arithmetic."""
    eng, args, start, std, eps, gen_fn, loss_fn = _engine_case(tiny, space, lpips=False, use_graph=False)
    eng.run(1)
    torch.cuda.synchronize()
    lat0, m0, v0 = eng.latent_in.cpu().double(), eng.exp_avg.cpu().double(), eng.exp_avg_sq.cpu().double()
    lr1, t = float(eng.lr_table[1]), int(eng.adam_t[0]) + 1
    assert lr1 > 0
    eng.run(1)
    lat1 = eng.latent_in.cpu().double()
    z = (lat0.float() + eps[1] * float(eng.sigma[1])).requires_grad_()
    loss_fn(1, gen_fn(z)).backward()
    g = z.grad.double().reshape(lat0.shape)
    b1, b2 = eng.betas
    m, v = b1 * m0 + (1 - b1) * g, b2 * v0 + (1 - b2) * g * g
    want = lat0 - lr1 * (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eng.adam_eps)
    step_ref, step_got = want - lat0, lat1 - lat0
    err = float((step_got - step_ref).abs().max() / step_ref.abs().max())
    print(f"OBS teacher-forced {space}: max |update diff| / max |update| {err:.3e}")
    assert err <= 1e-2


def test_gradient_engine_graph_replay_is_eager_bits(tiny):
    a = _engine_case(tiny, "z", lpips=True, use_graph=True, steps=6)[0].run().result()
    b = _engine_case(tiny, "z", lpips=True, use_graph=False, steps=6)[0].run().result()
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[3], b[3])


def test_lockstep_and_flagless_mdf_refused(tiny):
    from morphganformer_amd import drivers
    from morphganformer_amd._lib import MgfError
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    G, tsd, cfg = tiny
    crit = MDFLoss(random_discriminators(0), num_scales=2, differentiable=True)
    two = torch.zeros(2, 3, 64, 64, device="cuda")
    with pytest.raises(MgfError, match="MDF"):
        GradientProjectionEngine(G, two, torch.zeros(cfg.k, cfg.z_dim, device="cuda"), 1.0, ProjectionArgs(step=2), mdf=crit)
    with pytest.raises(MgfError, match="MDF"):
        drivers._project_group(G, [two[:1], two[1:]], None, args=ProjectionArgs(step=2), latent_mean=torch.zeros(cfg.k, cfg.z_dim, device="cuda"),
                               latent_std=1.0, mdf=crit)
    with pytest.raises(MgfError, match="differentiable=True"):
        GradientProjectionEngine(G, two[:1], torch.zeros(cfg.k, cfg.z_dim, device="cuda"), 1.0, ProjectionArgs(step=2),
                                 mdf=MDFLoss(random_discriminators(0), num_scales=2))


def test_cli_project_gradient_mode_with_mdf_weight_file(tmp_path):
    from morphganformer_amd import cli
    from test_host_and_abi import _tiny_snapshot
    from test_mdf_host import _seeded_modules, _WDisc, _ConvBlock
    from PIL import Image
    import types
    pkl = str(tmp_path / "net.pkl")
    _tiny_snapshot(pkl, seed=3)
    pkg, mod = types.ModuleType("SinGAN"), types.ModuleType("SinGAN.models")
    for cls, name in ((_ConvBlock, "ConvBlock"), (_WDisc, "WDiscriminator")):
        cls.__module__, cls.__qualname__, cls.__name__ = "SinGAN.models", name, name
        setattr(mod, name, cls)
    sys.modules["SinGAN"], sys.modules["SinGAN.models"] = pkg, mod
    try:
        torch.save(_seeded_modules((32, 32, 64)), str(tmp_path / "Ds.pth"), _use_new_zipfile_serialization=False)
    finally:
        sys.modules.pop("SinGAN", None)
        sys.modules.pop("SinGAN.models", None)
    Image.fromarray((np.random.default_rng(0).random((64, 64, 3)) * 255).astype(np.uint8)).save(tmp_path / "a.png")
    argv = ["project", "--model", pkl, "--image", str(tmp_path / "a.png"), "--path_to_gen", str(tmp_path / "p"), "--size", "64", "--step", "6",
            "--n_mean_latent", "200", "--seed", "0", "--no-lpips", "--no-mse", "--min-loss-init", "1000", "--mode", "gradient",
            "--mdf", str(tmp_path / "Ds.pth"), "--mdf-scales", "3"]
    assert cli.main(argv) == 0
    files = [f for _, _, fs in os.walk(tmp_path / "p") for f in fs]
    assert any(f.endswith(".png") for f in files) and any(f.endswith(".mat") for f in files), files
