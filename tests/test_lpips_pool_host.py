"""PerceptualLoss(pool_above=N), host side: the one pool-factor expression, the float64 helper's adjoint identity, the declarations of
csrc/block_pool.hip, and the command line's --lpips-pool-above (the module entries that have it, and what `_lpips_term` does with it)."""
import types

import pytest
import torch

from lpips_pool_torch_ref import block_mean_adjoint_ref, block_mean_ref, pool_factor_ref


@pytest.mark.parametrize("resolution", [64, 256, 1024])
@pytest.mark.parametrize("pool_above", [0, 32, 64, 100, 256, 1024, 2048])
def test_shared_pool_factor_is_the_expression_of_projection_args(resolution, pool_above):
    """misc.pool_factor gives the values test_pool_factor_is_the_three_expressions_it_replaced lists, and ProjectionArgs calls it."""
    from morphganformer_amd import misc
    from morphganformer_amd.projection import ProjectionArgs
    r, pa = resolution, pool_above
    f = misc.pool_factor(r, pa)
    assert f == pool_factor_ref(r, pa) == ProjectionArgs(pool_above=pa).pool_factor(r)
    assert r // f == (r // (r // pa) if (pa and r > pa) else r)
    assert (f > 1) == bool(pa and r > pa and r // pa > 1) and (f <= 1 or f == r // pa)


def test_projection_args_and_the_lpips_term_share_the_helper(monkeypatch):
    from morphganformer_amd import misc
    from morphganformer_amd.projection import ProjectionArgs
    monkeypatch.setattr(misc, "pool_factor", lambda size, pool_above: 7)
    assert ProjectionArgs(pool_above=32).pool_factor(64) == 7


@pytest.mark.parametrize("h,w,f,gh,gw", [(2, 2, 2, 1, 1), (6, 10, 2, 3, 5), (12, 12, 3, 4, 4), (12, 12, 3, 3, 3), (40, 24, 8, 5, 3), (40, 24, 8, 1, 1),
                                         (64, 64, 2, 31, 31)])
def test_helper_adjoint_is_the_transpose(h, w, f, gh, gw):
    """<P x, y> = <x, P^T y> in float64, with y zero-extended to the pooled grid where it covers less."""
    g = torch.Generator().manual_seed(h * 100 + w + f)
    x = torch.randn(2, 3, h, w, generator=g, dtype=torch.float64)
    y = torch.randn(2, 3, gh, gw, generator=g, dtype=torch.float64)
    yfull = torch.zeros(2, 3, h // f, w // f, dtype=torch.float64)
    yfull[:, :, :gh, :gw] = y
    lhs = float((block_mean_ref(x, f) * yfull).sum())
    adj = block_mean_adjoint_ref(y, f, h, w)
    rhs = float((x * adj).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((x.abs() * adj.abs()).sum())
    assert float(adj[:, :, gh * f:].abs().sum()) == 0.0 and float(adj[:, :, :, gw * f:].abs().sum()) == 0.0
    # ... and it is what autograd gives through the forward helper
    xr = x.clone().requires_grad_(True)
    (auto,) = torch.autograd.grad(block_mean_ref(xr, f), xr, yfull)
    assert torch.allclose(auto, adj, rtol=1e-14, atol=0)


def test_entries_are_declared_bound_and_built():
    from morphganformer_amd import _lib, build
    assert "block_pool.hip" in build.SOURCES
    res, args = _lib._SIGS["mgf_block_mean_f32"]
    assert res is _lib.C.c_int and args == [_lib.vp, _lib.vp, _lib.i32, _lib.i32, _lib.i32, _lib.i32, _lib.vp]
    res, args = _lib._SIGS["mgf_block_mean_adjoint_f32"]
    assert res is _lib.C.c_int
    assert args == [_lib.vp, _lib.vp] + [_lib.i32] * 6 + [_lib.i64, _lib.i64, _lib.i32, _lib.vp]
    with open(_lib.HEADER_PATH) as f:
        assert "projection_example_v1.py:148-155" in f.read()


def test_module_entries_take_the_flag():
    from morphganformer_amd import demorph, evolution
    a = demorph.build_parser().parse_args(["--morph", "m.png", "--reference", "r.png", "--out", "o"])
    assert a.lpips_pool_above == 0
    a = demorph.build_parser().parse_args(["--morph", "m.png", "--reference", "r.png", "--out", "o", "--lpips-pool-above", "256"])
    assert a.lpips_pool_above == 256
    a = evolution.build_parser().parse_args(["--image", "f.png"])
    assert a.lpips_pool_above == 0 and a.pool_above == 0
    a = evolution.build_parser().parse_args(["--image", "f.png", "--lpips-pool-above", "256", "--pool-above", "512"])
    assert (a.lpips_pool_above, a.pool_above) == (256, 512)


def test_lpips_term_hands_the_flag_to_the_loss_and_refuses_a_map(monkeypatch):
    from morphganformer_amd import cli, lpips
    seen = {}

    def fake(**kw):
        seen.update(kw)
        return "term"
    monkeypatch.setattr(lpips, "PerceptualLoss", fake)
    ns = lambda **kw: types.SimpleNamespace(lpips_backbone=None, lpips_random_backbone=True, net="squeeze", **kw)
    assert cli._lpips_term(ns(lpips_pool_above=256), "demorph", device="cpu") == "term" and seen["pool_above"] == 256
    assert cli._lpips_term(ns(), "project", device="cpu") == "term" and seen["pool_above"] == 0          # a namespace without the option: off
    with pytest.raises(SystemExit, match="the map is defined at the image's own size"):
        cli._lpips_term(ns(lpips_pool_above=256), "lpips-map", spatial=True)
