"""CPU: the host side of the region-weighted terms -- the per-tap weights, the landmark-hull helper, the float64
reference itself against the oracle's un-weighted LPIPS, and the command line's argument errors."""
import os

import numpy as np
import pytest
import torch

from region_weight_torch_ref import lpips_weighted_ref, mse_weighted_ref, tap_weights_ref, weights

SIDES = [(31, 31), (15, 15), (7, 7), (3, 3), (1, 1), (5, 9)]


@pytest.mark.parametrize("kind", ["random", "half", "disc"])
def test_region_tap_weights_sum_to_one_and_match_the_definition(kind):
    from morphganformer_amd.lpips import region_tap_weights
    W = torch.stack([weights(kind, 64, 67, seed=3), weights("random", 64, 67, seed=4)])
    om = region_tap_weights(W, SIDES)
    assert [tuple(o.shape) for o in om] == [(2, h, w) for h, w in SIDES] and all(o.dtype == torch.float32 for o in om)
    for o, side in zip(om, SIDES):
        assert float((o.double().sum(dim=(1, 2)) - 1.0).abs().max()) < 1e-6 and bool((o >= 0).all())
        assert torch.equal(o.double(), tap_weights_ref(W, side))
        pooled = torch.nn.functional.adaptive_avg_pool2d(W[:, None], side)[:, 0]
        assert float(((pooled / pooled.sum(dim=(1, 2), keepdim=True)).sum(dim=(1, 2)) - 1.0).abs().max()) < 1e-14       # the float64 form
    one = region_tap_weights(W[0], SIDES)                                                                                # [H,W] in, [h,w] out
    assert all(torch.equal(a, b[0]) for a, b in zip(one, om))


@pytest.mark.parametrize("value", [1.0, 0.37, 1e-6, 255.0])
def test_uniform_weight_gives_exactly_the_spatial_mean(value):
    from morphganformer_amd.lpips import region_tap_weights
    for o, (h, w) in zip(region_tap_weights(torch.full((64, 67), value, dtype=torch.float32), SIDES), SIDES):
        assert bool((o == np.float32(1.0 / (h * w))).all()), (h, w)


@pytest.mark.parametrize("net,size", [("squeeze", 64), ("squeeze", 67), ("vgg", 48), ("alex", 96)])
def test_float64_reference_reduces_to_the_oracle_for_a_uniform_weight(net, size):
    """The helper the GPU tests compare against, itself against oracle.loss_ref.lpips_ref and mse_ref: a constant weight is today's objective."""
    from morphganformer_amd.lpips import WEIGHTS_DIR
    from oracle.loss_ref import backbone_random, lpips_ref, mse_ref
    torch.manual_seed(size)
    a, b = torch.rand(2, 3, size, size) * 2 - 1, torch.rand(1, 3, size, size) * 2 - 1
    bb = backbone_random(net, 0)
    lin = np.load(os.path.join(WEIGHTS_DIR, f"lpips_lin_{net}.npz"))
    lins = [torch.from_numpy(lin[f"lin{i}"]).float().reshape(-1) for i in range(len(lin.files))]
    bb64 = {k: v.double() for k, v in bb.items()}
    want = lpips_ref(bb64, [l.double() for l in lins], a.double(), b.double().expand(2, -1, -1, -1), net=net).reshape(2)
    got = lpips_weighted_ref(bb, lins, a, b, torch.full((size, size), 0.7), net=net)
    assert float(((got - want) / want).abs().max()) < 1e-6
    assert torch.allclose(mse_weighted_ref(a[:1], b, torch.full((size, size), 0.7)), mse_ref(a[:1].double(), b.double()).reshape(1), rtol=1e-12)


def test_check_region_weight():
    from morphganformer_amd.lpips import check_region_weight
    good = torch.rand(5, 7) + 0.1
    assert tuple(check_region_weight(good).shape) == (1, 5, 7) and check_region_weight(good).dtype == torch.float64
    assert tuple(check_region_weight(good[None, None]).shape) == (1, 5, 7)
    assert tuple(check_region_weight(good.expand(3, 1, 5, 7)).shape) == (3, 5, 7)
    assert tuple(check_region_weight(good.numpy()).shape) == (1, 5, 7)
    for bad, what in ((-good, ">= 0"), (good * float("nan"), "finite"), (good * float("inf"), "finite"), (good * 0, "all-zero"),
                      (torch.stack([good, good * 0])[:, None], "all-zero"), (good[None], r"\[H,W\]"), (good.expand(2, 3, 5, 7), r"\[H,W\]")):
        with pytest.raises(ValueError, match=what):
            check_region_weight(bad)


def test_face_region_weight_fills_the_hull():
    from morphganformer_amd.drivers import face_region_weight
    pts = np.array([[10, 12], [40, 12], [40, 50], [10, 50], [20, 20], [30, 45], [25, 30]], dtype=np.float64)     # (x, y): a square + interior points
    w = face_region_weight(pts, 64, inside=2.0, outside=0.25)
    want = np.full((64, 64), 0.25, np.float32)
    want[12:51, 10:41] = 2.0                                                                                     # rows are y, columns x; boundary included
    assert w.dtype == np.float32 and w.shape == (64, 64) and np.array_equal(w, want)
    assert np.array_equal(face_region_weight(pts[::-1], 64), (want > 1).astype(np.float32))                      # point order does not matter
    f = face_region_weight(pts, 64, inside=1.0, outside=0.0, feather=2.0)
    row = f[30]
    assert np.all(np.diff(row[:26]) >= 0) and np.all(np.diff(row[25:]) <= 0)                                      # monotone across both edges
    assert 0.4 < row[10] < 0.75 and row[25] > 0.999 and row[0] < 1e-3 and 0.0 <= f.min() and f.max() <= 1.0
    for bad in (dict(inside=-1.0), dict(feather=-0.5), dict(inside=0.0, outside=0.0)):
        with pytest.raises(ValueError):
            face_region_weight(pts, 64, **bad)
    with pytest.raises(ValueError):
        face_region_weight(pts[:2], 64)


def test_load_region_weight(tmp_path):
    from PIL import Image
    from morphganformer_amd.drivers import load_region_weight
    w = np.random.default_rng(0).random((6, 9)).astype(np.float64)
    np.save(tmp_path / "w.npy", w)
    got = load_region_weight(str(tmp_path / "w.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, w.astype(np.float32))
    g = (np.arange(54, dtype=np.uint8) * 4).reshape(6, 9)
    Image.fromarray(g, mode="L").save(tmp_path / "w.png")
    assert np.array_equal(load_region_weight(str(tmp_path / "w.png")), g.astype(np.float32) / 255.0)
    np.save(tmp_path / "bad.npy", np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match=r"\[H,W\]"):
        load_region_weight(str(tmp_path / "bad.npy"))


def test_cli_region_argument_errors():
    """The region options are checked before anything is loaded: no model file is read, no GPU is touched."""
    from morphganformer_amd import cli
    base = ["project", "--model", "missing.pkl", "--image", "missing.png"]
    with pytest.raises(SystemExit, match="pass one of them"):
        cli.main(base + ["--landmarks", "lm.npz", "--region-weight", "w.npy", "--region-from-landmarks", "1,0"])
    with pytest.raises(SystemExit, match="needs --landmarks"):
        cli.main(base + ["--region-from-landmarks", "1,0.1,2"])
    for bad in ("1", "1,2,3,4", "a,b", "-1,0", "0,0", "1,0,-2"):
        with pytest.raises(SystemExit, match="INSIDE,OUTSIDE"):
            cli.main(base + ["--landmarks", "lm.npz", f"--region-from-landmarks={bad}"])
    a = cli.build_parser().parse_args(base + ["--landmarks", "lm.npz", "--region-from-landmarks", "1,0.1,2"])
    assert cli.region_arguments(a) == ("landmarks", 1.0, 0.1, 2.0)
    a = cli.build_parser().parse_args(base + ["--region-weight", "w.npy"])
    assert cli.region_arguments(a) == ("file", "w.npy")
    a = cli.build_parser().parse_args(["morph", "--model", "m", "--w1", "a", "--w2", "b", "--out", "o", "--refine", "--region-weight", "w.npy"])
    assert a.region_weight == "w.npy" and cli.region_arguments(a) is None


def test_engines_name_the_argument():
    import inspect
    from morphganformer_amd import drivers
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionEngine
    for fn in (ProjectionEngine.__init__, GradientProjectionEngine.__init__, ProjectionEngine.retarget, drivers.project_image, drivers.refine_morph):
        assert inspect.signature(fn).parameters["region_weight"].default is None
    assert inspect.signature(drivers.project_many).parameters["region_weights"].default is None
    assert callable(PerceptualLoss.set_region_weight)
