"""The MDF objective on MI355X (csrc/mdf.hip, morphganformer_amd/mdf.py): every kernel against float64, MDFLoss against the reference's
own numbers (tests/golden/mdf_tiny.npz) and a float64 restatement up to 1024^2, batch invariance, and the projection engine / CLI."""
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

from test_mdf_host import GOLDEN, mdf_loss64  # noqa: E402


def _L():
    from morphganformer_amd import _lib
    return _lib, _lib.lib()


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _part_sum(part):
    return part.double().sum(dim=-1).cpu()


SIDES = [(11, 11), (13, 12), (16, 1024)]


@pytest.mark.parametrize("c", [32, 64, 128])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("hw", SIDES)
def test_head_kernel_against_float64(c, n, hw):
    _lib, L = _L()
    h, w = hw
    img = _rand((n, 3, h, w), 1).cuda()
    wt, b = _rand((c, 3, 3, 3), 2, 0.3), _rand((c,), 3, 0.1)
    tgt = _rand((c, h, w), 4).abs().cuda()
    x1 = torch.full((n, c, h, w), float("nan"), device="cuda")
    nblk = int(L.mgf_mdf_partials(h, w))
    part = torch.empty(n, nblk, dtype=torch.float64, device="cuda")
    wc, bc = wt.cuda(), b.cuda()          # (named: a temporary could be recycled for the next one before the launch)
    _lib.check(L.mgf_mdf_head_f32(x1.data_ptr(), part.data_ptr(), img.data_ptr(), wc.data_ptr(), bc.data_ptr(), tgt.data_ptr(),
                                  n, c, h, w, 0.2, _lib.stream_ptr()))
    ref = F.leaky_relu(F.conv2d(img.cpu().double(), wt.double(), b.double()), 0.2)
    assert torch.isfinite(x1).all(), "the head writes the whole frame"
    assert _rel(x1[:, :, 1:-1, 1:-1].cpu(), ref) <= 1e-5
    l2 = ((ref - tgt[:, 1:-1, 1:-1].cpu().double()) ** 2).sum(dim=(1, 2, 3))
    assert _rel(_part_sum(part), l2) <= 1e-5


def _body(x, c, h, w, n, wt, b):
    from morphganformer_amd import conv as cv
    _lib, L = _L()
    u = cv.winograd2_weights(wt.cuda())
    y = torch.empty(n, c, h, w, device="cuda")
    bc = b.cuda()
    _lib.check(L.mgf_mdf_body_f32(y.data_ptr(), x.data_ptr(), u.data_ptr(), bc.data_ptr(), n, c, h, w, 0.2, _lib.stream_ptr()))
    return y


@pytest.mark.parametrize("c", [32, 64, 128])
@pytest.mark.parametrize("n", [1, 5, 32])
@pytest.mark.parametrize("hw", SIDES + [(64, 64)])
def test_body_kernel_against_float64_and_batch_invariant(c, n, hw):
    h, w = hw
    if w == 1024:
        n = min(n, 5)                 # (the float64 reference runs on the host)
    x = _rand((n, c, h, w), 5).cuda()
    wt, b = _rand((c, c, 3, 3), 6, (2.0 / (9 * c)) ** 0.5), _rand((c,), 7, 0.1)
    y = _body(x, c, h, w, n, wt, b)
    ref = F.leaky_relu(F.conv2d(x.cpu().double(), wt.double(), b.double()), 0.2)
    assert _rel(y[:, :, 1:-1, 1:-1].cpu(), ref) <= 1e-5
    if n > 1:                       # a sample's bits do not depend on the batch it is launched in
        y1 = _body(x[n - 1:].contiguous(), c, h, w, 1, wt, b)
        assert torch.equal(y1[0], y[n - 1])


@pytest.mark.parametrize("c", [32, 64, 128])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("hw", SIDES)
def test_tail_kernel_with_both_l2_taps_against_float64(c, n, hw):
    _lib, L = _L()
    h, w = hw
    r = 4 if min(h, w) > 10 else 0
    x2 = _rand((n, c, h, w), 8).cuda()
    wt, b = _rand((1, c, 3, 3), 9, (1.0 / (9 * c)) ** 0.5), 0.03
    x2t, x3t = _rand((c, h, w), 10).cuda(), _rand((h, w), 11).cuda()
    nblk = int(L.mgf_mdf_partials(h, w))
    p2, p3 = (torch.empty(n, nblk, dtype=torch.float64, device="cuda") for _ in range(2))
    x3 = torch.full((n, h, w), float("nan"), device="cuda")
    wc = wt.cuda()
    _lib.check(L.mgf_mdf_tail_f32(x3.data_ptr(), p2.data_ptr(), p3.data_ptr(), x2.data_ptr(), wc.data_ptr(), b, x2t.data_ptr(),
                                  x3t.data_ptr(), n, c, h, w, r, _lib.stream_ptr()))
    v2 = x2.cpu().double()[:, :, r:h - r, r:w - r]
    ref3 = F.conv2d(v2, wt.double()) + b
    assert _rel(x3[:, r + 1:h - r - 1, r + 1:w - r - 1].cpu()[:, None], ref3) <= 1e-5
    assert _rel(_part_sum(p2), ((v2 - x2t.cpu().double()[:, r:h - r, r:w - r]) ** 2).sum(dim=(1, 2, 3))) <= 1e-5
    assert _rel(_part_sum(p3), ((ref3[:, 0] - x3t.cpu().double()[r + 1:h - r - 1, r + 1:w - r - 1]) ** 2).sum(dim=(1, 2))) <= 1e-5


@pytest.mark.parametrize("n", [1, 5, 32])
def test_finish_kernel_fixed_order_scale_accumulate(n):
    import ctypes
    _lib, L = _L()
    nslots, nblk = 24, 4096
    part = (_rand((nslots, n, nblk), 12).abs().double()).cuda()
    counts = (ctypes.c_double * nslots)(*[float(1000 + 37 * s) for s in range(nslots)])
    ref = (part.cpu().sum(dim=2) / torch.tensor(list(counts), dtype=torch.float64)[:, None]).sum(dim=0)
    out = torch.full((n,), 0.5, device="cuda")
    _lib.check(L.mgf_mdf_finish_f32(out.data_ptr(), part.data_ptr(), nslots, nblk, counts, n, 1.0, 0, _lib.stream_ptr()))
    assert _rel(out.cpu(), ref) <= 1e-6
    first = out.clone()
    _lib.check(L.mgf_mdf_finish_f32(out.data_ptr(), part.data_ptr(), nslots, nblk, counts, n, 2.0, 1, _lib.stream_ptr()))
    assert _rel(out.cpu(), 3 * ref) <= 1e-6
    _lib.check(L.mgf_mdf_finish_f32(out.data_ptr(), part.data_ptr(), nslots, nblk, counts, n, 1.0, 0, _lib.stream_ptr()))
    assert torch.equal(out, first)


# ------------------------------------------------------------------------------------------------------------ MDFLoss
@pytest.mark.parametrize("case", ["asc8", "asc5", "desc9"])
def test_mdfloss_matches_reference_fixture(case):
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    g = np.load(GOLDEN)
    seed, nd, scales, asc = (int(v) for v in g[f"{case}_cfg"])
    Ds = random_discriminators(seed, (32,) * 4 + (64,) * 4 + ((128,) if nd == 9 else ()))
    crit = MDFLoss(Ds, num_scales=scales, is_ascending=asc)
    crit.set_target(torch.from_numpy(g["target"]).cuda())
    cand = torch.from_numpy(g["candidates"]).cuda()
    taps = crit.distance_per_tap(cand).numpy()
    assert np.abs(taps - g[f"{case}_taps"]).max() <= 1e-5 * np.abs(g[f"{case}_taps"]).max()
    out = torch.zeros(3, device="cuda")
    crit.distance_into(out, cand)
    assert np.allclose(out.cpu().numpy(), g[f"{case}_loss"], rtol=1e-5, atol=0)
    assert abs(float(crit(torch.from_numpy(g["target"]).cuda(), cand)) - float(g[f"{case}_mean"])) <= 1e-5 * float(g[f"{case}_mean"])


def _pair(res, n, seed):
    t = torch.tanh(_rand((1, 3, res, res), seed))
    return t, (t + 0.3 * _rand((n, 3, res, res), seed + 1)).clamp(-1, 1)


def _loss64_gpu(Ds, t, y):
    """float64 restatement on the device (torch's own float64 convolution) for the large maps."""
    from test_mdf_host import mdf_taps64
    tot = torch.zeros(y.shape[0], dtype=torch.float64)
    dev = lambda sd: {k: torch.as_tensor(v, dtype=torch.float64, device="cuda") for k, v in sd.items()}
    for sd in Ds:
        sd = dev(sd)
        tx, ty = mdf_taps64(sd, t.cuda().double()), mdf_taps64(sd, y.cuda().double())
        for k in range(3):
            tot += ((ty[k] - tx[k]) ** 2).mean(dim=(1, 2, 3)).cpu()
    return tot


def test_mdfloss_256_all_eight_against_float64():
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    Ds = random_discriminators(4)
    t, y = _pair(256, 3, 20)
    crit = MDFLoss(Ds)
    crit.set_target(t.cuda())
    out = torch.zeros(3, device="cuda")
    crit.distance_into(out, y.cuda())
    _, ref = mdf_loss64(Ds, t, y)
    assert np.allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=0)


def test_mdfloss_1024_one_candidate_against_float64():
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    Ds = random_discriminators(6)
    t, y = _pair(1024, 1, 30)
    crit = MDFLoss(Ds)
    crit.set_target(t.cuda())
    out = torch.zeros(1, device="cuda")
    crit.distance_into(out, y.cuda())
    ref = _loss64_gpu(Ds, t, y)
    assert abs(float(out[0]) - float(ref[0])) <= 1e-4 * float(ref[0])


@pytest.mark.parametrize("res", [64, 256])
def test_mdfloss_bit_identical_across_batch_and_runs(res):
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    crit = MDFLoss(random_discriminators(1))
    t, y = _pair(res, 8, 40)
    crit.set_target(t.cuda())
    y = y.cuda()
    a, b = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    crit.distance_into(a, y)
    crit.distance_into(b, y)
    assert torch.equal(a, b)
    for i in (0, 5):
        one = torch.zeros(1, device="cuda")
        crit.distance_into(one, y[i:i + 1].contiguous())
        assert torch.equal(one[0], a[i])


# ------------------------------------------------------------------------------------------------------------ engine / drivers / CLI
def _tiny_engine(mdf_loss, batch=4, use_graph=True, pipeline=False, pool_above=0, steps=12, eps_seed=3, keep_images=0):
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine
    from morphganformer_amd.synth_weights import TINY, make_state_dict, synthetic_latents
    G = Generator(make_state_dict(TINY, seed=0), TINY, "cuda", max_batch=1)
    rng = np.random.Generator(np.random.PCG64(eps_seed))
    lm = torch.from_numpy(rng.standard_normal((TINY.k, TINY.z_dim)).astype(np.float32) * 0.1).cuda()
    eps = torch.from_numpy(rng.standard_normal((steps, 1, TINY.k, TINY.z_dim)).astype(np.float32)).cuda()
    tgt = G(torch.from_numpy(synthetic_latents(TINY, 1, 1001)).cuda(), None, noise_mode="const")[0].clamp(-1, 1).clone()
    if pool_above:
        f = 64 // pool_above
        tgt = tgt.reshape(1, 3, pool_above, f, pool_above, f).mean(dim=(3, 5)).contiguous()
    args = ProjectionArgs(step=steps, min_loss_init=1000.0, pool_above=pool_above)
    eng = ProjectionEngine(G, tgt, lm, 23.3, args, percept=None, use_mse=False, eps=eps, noise_mode="const", use_graph=use_graph,
                           batch=batch, pipeline=pipeline, mdf=mdf_loss, keep_images=keep_images)
    return eng, G, lm, eps, tgt


@pytest.mark.parametrize("pool_above", [0, 32])
def test_engine_against_one_candidate_at_a_time(pool_above):
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    crit = MDFLoss(random_discriminators(2))
    eng, G, lm, eps, tgt = _tiny_engine(crit, pool_above=pool_above)
    lat, bstep, bloss, losses = eng.run().result()
    ref_crit = MDFLoss(random_discriminators(2))
    ref_crit.set_target(tgt)
    ref = []
    for i in range(eps.shape[0]):
        z = (lm + eps[i, 0] * eng.sigma[i].float()).reshape(1, *lm.shape)
        img = G(z, 0.7, noise_mode="const")[0]
        if pool_above:
            f = 64 // pool_above
            img = img.reshape(1, 3, pool_above, f, pool_above, f).mean(dim=(3, 5))
        o = torch.zeros(1, device="cuda")
        ref_crit.distance_into(o, img.contiguous())
        ref.append(float(o[0]))
    ref = np.array(ref)
    assert np.abs(losses - ref).max() <= 1e-5 * np.abs(ref).max()
    # the best step: every strict improvement, in step order (num_loss < min_loss from 1000)
    best, m = -1, 1000.0
    for i, v in enumerate(losses):
        if v < m:
            best, m = i, v
    assert bstep == best
    srt = np.sort(ref)
    if srt[1] - srt[0] > 1e-4 * srt[0]:
        assert bstep == int(np.argmin(ref))
    lat1, bstep1, _, losses1 = _tiny_engine(MDFLoss(random_discriminators(2)), batch=1, use_graph=False, pool_above=pool_above)[0].run().result()
    assert bstep1 == bstep and torch.equal(lat1, lat) and np.abs(losses1 - losses).max() <= 1e-5 * np.abs(losses).max()


def test_engine_graph_pipeline_retarget_and_keep_images():
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    Ds = random_discriminators(3)
    runs = {}
    for name, kw in (("eager", dict(use_graph=False)), ("graph", dict(use_graph=True)), ("pipe", dict(use_graph=True, pipeline=True))):
        eng = _tiny_engine(MDFLoss(Ds), keep_images=4, **kw)[0]
        runs[name] = eng.run().result()
        assert len(eng.improvements()) >= 1
    for name in ("graph", "pipe"):
        assert runs[name][1] == runs["eager"][1] and torch.equal(runs[name][0], runs["eager"][0])
        assert np.array_equal(runs[name][3], runs["eager"][3])
    # retarget: an engine pointed at another target equals a fresh engine on it
    eng_a, G, lm, eps, tgt = _tiny_engine(MDFLoss(Ds))
    eng_a.run()
    eng_b, _, _, _, tgt_b = _tiny_engine(MDFLoss(Ds), eps_seed=4)
    fresh = eng_b.run().result()
    eng_a.retarget(tgt_b, eps=eng_b.eps, latent_mean=eng_b.latent_in.reshape(lm.shape))
    again = eng_a.run().result()
    assert again[1] == fresh[1] and torch.equal(again[0], fresh[0]) and np.array_equal(again[3], fresh[3])


def test_gradient_engine_refuses_mdf():
    from morphganformer_amd._lib import MgfError
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    from morphganformer_amd.synth_weights import TINY, make_state_dict
    G = Generator(make_state_dict(TINY, seed=0), TINY, "cuda", max_batch=1)
    with pytest.raises(MgfError, match="MDF"):
        GradientProjectionEngine(G, torch.zeros(1, 3, 64, 64, device="cuda"), torch.zeros(TINY.k, TINY.z_dim, device="cuda"), 1.0,
                                 ProjectionArgs(step=2), percept=None, mdf=MDFLoss(random_discriminators(0)))


def test_1024_launch_sequence_32_candidates():
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine
    from morphganformer_amd.synth_weights import FULL1024, make_state_dict, synthetic_latents
    G = Generator(make_state_dict(FULL1024, seed=0), FULL1024, "cuda", max_batch=1)
    tgt = G(torch.from_numpy(synthetic_latents(FULL1024, 1, 1000)).cuda(), None, noise_mode="const")[0].clamp(-1, 1).clone()
    lm = torch.zeros(FULL1024.k, FULL1024.z_dim, device="cuda")
    eng = ProjectionEngine(G, tgt, lm, 1.0, ProjectionArgs(step=32, min_loss_init=1000.0), percept=None, use_mse=False, noise_mode="const",
                           batch=32, mdf=MDFLoss(random_discriminators(0)))
    lat, bstep, bloss, losses = eng.run().result()
    assert np.isfinite(losses).all() and (losses > 0).all()
    assert bstep == int(np.argmin(losses)) and bloss == pytest.approx(float(losses.min()), rel=1e-6)


def test_cli_project_with_mdf_weight_file(tmp_path):
    from morphganformer_amd import cli
    from morphganformer_amd.mdf import random_discriminators
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
            "--n_mean_latent", "200", "--batch", "4", "--seed", "0", "--no-lpips", "--no-mse", "--min-loss-init", "1000",
            "--mdf", str(tmp_path / "Ds.pth"), "--mdf-scales", "3"]
    assert cli.main(argv) == 0
    pngs = [f for f in os.listdir(tmp_path / "p") if f.endswith(".png")]
    assert len(pngs) >= 1
    assert cli.main(argv[:-4] + ["--mdf-random", "--mdf-scales", "2", "--mdf-descending", "--path_to_gen", str(tmp_path / "q")]) == 0
