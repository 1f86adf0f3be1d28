"""GPU: spatial LPIPS maps -- PerceptualLoss(spatial=True), the two kernels under it (mgf_lpips_layer_map_f32, mgf_lpips_upsample_sum_f32), the
drivers and the CLI verb -- against the reference's own PNetLin(spatial=True) outputs (tests/golden/lpips_spatial.npz) and the float64
restatement of that path (tests/lpips_spatial_torch_ref.py).

Gates: 1e-5 * max|ref| for the kernels on given taps (the gate test_lpips_distance_half_vs_reference_fixture uses for the same arithmetic),
1e-3 * max|ref| for the whole chain through the backbones (the project's whole-chain gate)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lpips_spatial_torch_ref import lpips_spatial_ref, tap_maps_ref  # noqa: E402

pytestmark = pytest.mark.gpu
NETS = {"squeeze": 7, "vgg": 5, "alex": 5}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _percept(net="squeeze", spatial=True, **kw):
    from morphganformer_amd.lpips import PerceptualLoss
    return PerceptualLoss(model="net-lin", net=net, spatial=spatial, use_gpu=True, allow_random_backbone=True, **kw)


def _upsample_sum(out, maps, accumulate=0):
    from morphganformer_amd import _lib
    n, H = out.shape[0], out.shape[-1]
    ptrs = (ctypes.c_void_p * 8)(*[m.data_ptr() for m in maps])
    sides = (ctypes.c_int32 * 8)(*[m.shape[-1] for m in maps])
    _lib.check(_lib.lib().mgf_lpips_upsample_sum_f32(out.data_ptr(), ptrs, sides, len(maps), n, H, accumulate, _lib.stream_ptr()), "upsample_sum")
    return out


@functools.lru_cache(maxsize=None)
def _fixture_maps(net):
    """The layer-map kernel on the fixture's tap tensors (n = 2, per-sample targets) -> (device maps [2,h,h], float64 reference maps, lins)."""
    from morphganformer_amd import _lib
    g = np.load(os.path.join(GOLDEN, "lpips_dist.npz"))
    P = _percept(net)
    L, st = _lib.lib(), _lib.stream_ptr()
    t0 = [g[f"{net}_tap0_{i}"] for i in range(NETS[net])]
    t1 = [g[f"{net}_tap1_{i}"] for i in range(NETS[net])]
    ref = tap_maps_ref(t0, t1, [l.cpu() for l in P.lins])
    maps, means = [], []
    scratch = torch.empty(2 * int(L.mgf_reduce_scratch_floats()), device="cuda")
    for i in range(NETS[net]):
        a, b = torch.from_numpy(t0[i]).cuda(), torch.from_numpy(t1[i]).cuda()
        n, c, h, w = a.shape
        bu = torch.empty_like(b)
        _lib.check(L.mgf_lpips_unit_f32(bu.data_ptr(), b.data_ptr(), n, c, h * w, st), "lpips_unit")
        m = torch.full((n, h, w), float("nan"), device="cuda")
        _lib.check(L.mgf_lpips_layer_map_f32(m.data_ptr(), a.data_ptr(), bu.data_ptr(), P.lins[i].data_ptr(), n, c, h * w, c * h * w, st), "lpips_layer_map")
        one = torch.zeros(n, device="cuda")
        _lib.check(L.mgf_lpips_layer_f32(one.data_ptr(), a.data_ptr(), bu.data_ptr(), P.lins[i].data_ptr(), n, c, h * w, c * h * w, 0,
                                         scratch.data_ptr(), st), "lpips_layer")
        maps.append(m)
        means.append(one.cpu().numpy())
    return maps, ref, means


@pytest.mark.parametrize("net", sorted(NETS))
def test_layer_map_kernel_on_the_fixture_taps(net):
    maps, ref, means = _fixture_maps(net)
    for i, (m, r, mean) in enumerate(zip(maps, ref, means)):
        got, want = m.cpu().numpy().astype(np.float64), r.numpy()[:, 0]
        assert got.shape == want.shape
        err, bound = np.abs(got - want).max(), 1e-5 * np.abs(want).max()
        print(f"{net} tap {i}: max abs err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (net, i)
        assert np.isfinite(got[:, 0, 0]).all()                       # the all-zero pixel of both taps: 0 / (0 + 1e-10)
        # the spatial mean of the map is the scalar kernel's value (same per-pixel statements, another summation order)
        mm = got.reshape(got.shape[0], -1).mean(1)
        assert np.abs(mm - mean).max() <= 1e-5 * np.abs(mean).max(), (net, i, mm, mean)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("sides,H", [((1, 1, 3, 7, 15), 32), ((2, 3, 7, 15, 31), 64), ((4, 8, 16, 33), 67)])
def test_upsample_sum_kernel_on_random_maps(sides, H, n, accumulate):
    """A 1x1 tap (all four neighbours are one texel), both clamps, an odd H and the scalar tail, against float64 torch."""
    rng = np.random.Generator(np.random.PCG64(1000 * H + 10 * n + accumulate))
    maps = [rng.standard_normal((n, 1, s, s)).astype(np.float32) for s in sides]
    start = rng.standard_normal((n, 1, H, H)).astype(np.float32)
    want = torch.from_numpy(start).double() if accumulate else torch.zeros(n, 1, H, H, dtype=torch.float64)
    for m in maps:
        up = torch.nn.Upsample(scale_factor=1. * H / m.shape[2], mode="bilinear", align_corners=False)(torch.from_numpy(m).double())
        assert tuple(up.shape) == (n, 1, H, H)
        want = want + up
    out = torch.from_numpy(start).cuda()
    _upsample_sum(out, [torch.from_numpy(m).cuda() for m in maps], accumulate)
    err, bound = float((out.cpu().double() - want).abs().max()), 1e-5 * float(want.abs().max())
    print(f"sides {sides} -> {H}, n {n}, accumulate {accumulate}: max abs err {err:.3e} (bound {bound:.3e})")
    assert err <= bound


@pytest.mark.parametrize("net", sorted(NETS))
def test_upsample_sum_against_the_reference_fixture(golden, net):
    """The reference's own PNetLin(spatial=True) on the fixture's taps: layer-map kernel -> up-sample-sum kernel against its `val`."""
    s = golden("lpips_spatial.npz")
    H = int(s[f"{net}_H"])
    maps, _, _ = _fixture_maps(net)
    out = torch.full((2, 1, H, H), float("nan"), device="cuda")
    _upsample_sum(out, maps)
    want = s[f"{net}_spatial_val"].astype(np.float64)
    err, bound = np.abs(out.cpu().numpy() - want).max(), 1e-5 * np.abs(want).max()
    print(f"{net} at {H}: max abs err {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    for i in range(1, NETS[net]):                                    # a tap alone (the reference's res[0] is its running total)
        one = torch.empty(2, 1, H, H, device="cuda")
        _upsample_sum(one, [maps[i]])
        w = s[f"{net}_spatial_res_{i}"].astype(np.float64)
        assert np.abs(one.cpu().numpy() - w).max() <= 1e-5 * np.abs(w).max(), i


def _images(n, H, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    a = rng.uniform(-1, 1, (n, 3, H, H)).astype(np.float32)
    b = np.clip(a + 0.3 * rng.standard_normal(a.shape), -1, 1).astype(np.float32)
    return a, b


@pytest.mark.parametrize("net,H", [("squeeze", 64), ("squeeze", 67), ("vgg", 64), ("alex", 64)])
def test_whole_chain_against_the_float64_helper(net, H):
    P = _percept(net)
    a, b = _images(2, H, 7 + H)
    val_ref, ups_ref, _ = lpips_spatial_ref(net, [l.cpu() for l in P.lins], a, b)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    val, res = P(ta, tb, retPerLayer=True)
    assert tuple(val.shape) == (2, 1, H, H) and val.dtype == torch.float32 and val.is_cuda
    err, bound = float((val.cpu().double() - val_ref).abs().max()), 1e-3 * float(val_ref.abs().max())
    print(f"{net} at {H}: max abs err {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert torch.equal(P(ta, tb), val)                               # with and without the per-tap list: the same map
    assert len(res) == NETS[net]
    for r, u in zip(res, ups_ref):                                   # un-aliased: every entry is that tap's own map
        assert float((r.cpu().double() - u).abs().max()) <= 1e-3 * float(u.abs().max())
    total = torch.stack([r.cpu().double() for r in res]).sum(0)
    assert float((total - val.cpu().double()).abs().max()) <= 1e-6 * float(val.abs().max())
    # identical images: an all-zero map exactly, per sample and against one shared target
    assert float(P(ta, ta).abs().max()) == 0.0
    assert float(P(ta[:1], ta[:1]).abs().max()) == 0.0
    if net == "vgg":
        # tap 0 has the image's size (scale factor 1: the up-sampling is the identity), so its map's spatial mean is the tap's scalar
        P.set_target(tb)
        per_tap = P.distance_per_tap(ta)[0].cpu().double()
        mean = res[0].cpu().double().mean([1, 2, 3])
        assert float((mean - per_tap).abs().max()) <= 1e-5 * float(per_tap.abs().max())


def test_batches_equal_one_at_a_time():
    """n = 3 candidates against one cached target, and 2 against 2, give the bits of the one-at-a-time maps."""
    P = _percept("squeeze")
    a, b = _images(3, 64, 21)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    one = torch.empty(1, 1, 64, 64, device="cuda")
    P.set_target(tb[:1])
    singles = [P.distance_map_into(one, ta[i:i + 1]).clone() for i in range(3)]
    out3 = P.distance_map_into(torch.empty(3, 1, 64, 64, device="cuda"), ta)
    assert float(out3.abs().max()) > 0
    assert torch.equal(out3, torch.cat(singles))
    ws = P._map_ws[(3, 64)]
    P.distance_map_into(out3, ta)
    assert P._map_ws[(3, 64)] is ws                                  # the per-tap maps are cached per (n, H)
    pairs = []
    for i in range(2):
        P.set_target(tb[i:i + 1])
        pairs.append(P.distance_map_into(one, ta[i:i + 1]).clone())
    P.set_target(tb[:2])
    out2 = P.distance_map_into(torch.empty(2, 1, 64, 64, device="cuda"), ta[:2])
    assert torch.equal(out2, torch.cat(pairs))


def _tiny_G(seed=0, max_batch=1):
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import TINY, make_state_dict
    return Generator(make_state_dict(TINY, seed=seed), TINY, "cuda", max_batch=max_batch)


def test_refusals_and_unchanged_scalar_paths():
    from morphganformer_amd import drivers
    from morphganformer_amd._lib import MgfError
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import ProjectionArgs
    P = _percept("squeeze")
    x = torch.zeros(1, 3, 64, 48, device="cuda")
    with pytest.raises(MgfError, match="square"):
        P(x, x)
    y = torch.zeros(1, 3, 96, 96, device="cuda")
    with pytest.raises(MgfError, match=r"tap 0 \(47x47\).*95.*96"):
        P(y, y)
    with pytest.raises(NotImplementedError):
        PerceptualLoss(model="net-lin", net="squeeze", colorspace="Lab", spatial=True, allow_random_backbone=True)
    with pytest.raises(NotImplementedError):
        PerceptualLoss(model="net", net="squeeze", spatial=True, allow_random_backbone=True)
    with pytest.raises(MgfError, match="spatial=False"):
        _percept("squeeze", spatial=False).distance_map_into(torch.empty(1, 1, 64, 64, device="cuda"), torch.zeros(1, 3, 64, 64, device="cuda"))
    # the scalar paths of a spatial instance are those of a non-spatial one: a projection scores exactly the same
    G = _tiny_G(max_batch=2)
    _, b = _images(1, 64, 5)
    target = torch.from_numpy(b).cuda()
    runs = []
    for spatial in (False, True):
        runs.append(drivers.project_image(G, target, None, None, args=ProjectionArgs(step=2, n_mean_latent=200), percept=_percept("squeeze", spatial=spatial),
                                          seed=0, batch=2, noise_mode="const"))
    assert np.array_equal(runs[0]["losses"], runs[1]["losses"]) and torch.equal(runs[0]["w"], runs[1]["w"]) and runs[0]["step"] == runs[1]["step"]
    with pytest.raises(ValueError, match="spatial=True"):
        drivers.project_image(G, target, None, None, args=ProjectionArgs(step=2, n_mean_latent=200), percept=_percept("squeeze", spatial=False),
                              seed=0, batch=2, noise_mode="const", lpips_map=True)
    with pytest.raises(ValueError):
        drivers.project_image(G, target, None, None, args=ProjectionArgs(step=2, n_mean_latent=200), percept=None, seed=0, batch=2,
                              noise_mode="const", lpips_map=True)


def test_drivers_and_cli_write_the_map(tmp_path):
    from PIL import Image
    from morphganformer_amd import cli, drivers
    from morphganformer_amd.projection import ProjectionArgs
    G = _tiny_G(max_batch=2)
    P = _percept("squeeze")
    _, b = _images(1, 64, 5)
    target = torch.from_numpy(b).cuda()
    out = drivers.project_image(G, target, None, None, args=ProjectionArgs(step=2, n_mean_latent=200), percept=P, seed=0, batch=2,
                                noise_mode="const", path_to_gen=str(tmp_path / "proj"), lpips_map=True)
    m = out["lpips_map"]
    assert tuple(m.shape) == (64, 64) and float(m.max()) > 0
    img = G.forward_workspace(out["w"].to(G.device), None, noise_mode="const")[0]
    assert torch.equal(m, drivers.lpips_map(P, img.float(), target)[0, 0])
    saved = np.load(tmp_path / "proj" / "best_lpips_map.npy")
    assert saved.dtype == np.float32 and np.array_equal(saved, m.cpu().numpy())
    png = np.asarray(Image.open(tmp_path / "proj" / "best_lpips_map.png"))
    assert png.dtype == np.uint8 and png.shape == (64, 64)
    assert np.array_equal(png, np.rint(255.0 * np.minimum(saved.astype(np.float64) / float(saved.max()), 1.0)).astype(np.uint8))
    # vmax clips; an all-zero map gives an all-zero PNG
    drivers.save_lpips_map(m, str(tmp_path / "clip"), vmax=0.5 * float(saved.max()))
    clip = np.asarray(Image.open(tmp_path / "clip.png"))
    assert clip.max() == 255 and np.array_equal(clip, np.rint(255.0 * np.minimum(saved.astype(np.float64) / (0.5 * float(saved.max())), 1.0)).astype(np.uint8))
    drivers.save_lpips_map(torch.zeros(1, 1, 8, 8), str(tmp_path / "zero"))
    assert not np.asarray(Image.open(tmp_path / "zero.png")).any()
    # the CLI verb needs no model: two image files in, the two map files out
    a, b2 = _images(1, 64, 9)
    for name, x in (("a", a), ("b", b2)):
        Image.fromarray(np.rint(x[0].transpose(1, 2, 0) * 127.5 + 127.5).clip(0, 255).astype(np.uint8)).save(tmp_path / f"{name}.png")
    argv = ["lpips-map", "--image-a", str(tmp_path / "a.png"), "--image-b", str(tmp_path / "b.png"), "--out", str(tmp_path / "cli" / "ab"), "--size", "64"]
    with pytest.raises(SystemExit, match="lpips-backbone"):
        cli.main(argv)
    assert cli.main(argv + ["--lpips-random-backbone"]) == 0
    got = np.load(tmp_path / "cli" / "ab.npy")
    assert got.shape == (64, 64) and got.dtype == np.float32 and got.max() > 0
    want = drivers.lpips_map(P, drivers.image_transform(str(tmp_path / "a.png"), size=64), drivers.image_transform(str(tmp_path / "b.png"), size=64))
    assert np.array_equal(got, want[0, 0].cpu().numpy())
    assert np.asarray(Image.open(tmp_path / "cli" / "ab.png")).shape == (64, 64)
