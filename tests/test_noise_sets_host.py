"""CPU: the host-side surface of per-target noise maps for lockstep targets -- the set entries of csrc/noise_opt.hip declared, bound and
built, the argument checks of the engine and the drivers that need no GPU -- and the torch restatement of a set
(tests/noise_sets_torch_ref.py, the oracle of tests/test_hip_noise_sets.py) against the per-map restatement applied map by map."""
import os
import re

import pytest
import torch

from noise_opt_torch_ref import noise_regularize_grad
from noise_sets_torch_ref import SIDES, gapped_table, make_sets, map_of, normalize_sets, regularize_sets
from test_hip_noise_opt import make_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mgf_noise_sets_scratch_bytes", "mgf_noise_sets_regularize_grad_f32", "mgf_noise_sets_normalize_f32", "mgf_noise_sets_grad_f32",
           "mgf_noise_sets_pack_f32", "mgf_adam_sets_f32"]


def test_set_entries_are_declared_bound_and_built():
    from morphganformer_amd import _lib, build
    with open(os.path.join(ROOT, "include", "mgf.h")) as fh:
        hdr = fh.read()
    declared = set(re.findall(r"\b(mgf_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in include/mgf.h"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound in _lib.py"
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert "noise_opt.hip" in build.SOURCES


def test_scratch_query_and_table_checks_need_no_device():
    """The query is host arithmetic: the per-map scratch of every map plus a value slot per map, per set; 0 for a table that is refused."""
    from morphganformer_amd import _lib
    L = _lib.lib()
    sides, _, n = _lib.map_table(SIDES, [0] * len(SIDES))
    per_set = sum(int(L.mgf_noise_regularize_scratch_bytes(s)) for s in SIDES) + 8 * n
    assert int(L.mgf_noise_sets_scratch_bytes(sides, n, 1)) == per_set and int(L.mgf_noise_sets_scratch_bytes(sides, n, 3)) == 3 * per_set
    assert int(L.mgf_noise_sets_scratch_bytes(sides, n, 0)) == 0 and int(L.mgf_noise_sets_scratch_bytes(sides, 0, 1)) == 0
    assert int(L.mgf_noise_sets_scratch_bytes(None, n, 1)) == 0
    bad, _, _ = _lib.map_table([4, 12], [0, 0])
    assert int(L.mgf_noise_sets_scratch_bytes(bad, 2, 1)) == 0
    many, _, _ = _lib.map_table([4] * 33, [0] * 33)
    assert int(L.mgf_noise_sets_scratch_bytes(many, 33, 1)) == 0 and int(L.mgf_noise_sets_scratch_bytes(many, 32, 1)) > 0


def test_engine_keyword_needs_optimize_noise():
    """The check comes first of all: no generator, no device."""
    from morphganformer_amd.projection import GradientProjectionEngine
    t = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match="noise_per_target=True gives every lockstep target its own noise maps"):
        GradientProjectionEngine(None, t, None, 1.0, noise_per_target=True)
    with pytest.raises(ValueError, match="noise_init"):
        GradientProjectionEngine(None, t, None, 1.0, optimize_noise=True, noise_per_target=True, noise_init="zeros")


def test_driver_argument_checks():
    from morphganformer_amd import _lib, drivers
    t = [torch.zeros(1, 3, 8, 8)] * 2
    with pytest.raises(ValueError, match="1 output prefixes for 2 targets"):
        drivers.project_many(None, t, lockstep=2, mode="gradient", optimize_noise=True, out_prefixes=["a"])
    with pytest.raises(ValueError, match="out_prefixes go with lockstep > 1 and optimize_noise=True"):
        drivers.project_many(None, t, lockstep=2, mode="gradient", out_prefixes=["a", "b"])
    with pytest.raises(ValueError, match="out_prefixes go with lockstep > 1 and optimize_noise=True"):
        drivers.project_many(None, t, mode="gradient", optimize_noise=True, out_prefixes=["a", "b"])
    with pytest.raises(ValueError, match="noise_init must be 'randn' or 'const'"):
        drivers._project_group(None, t, None, optimize_noise=True, noise_init="zeros")
    with pytest.raises(_lib.MgfError, match="MDF objective runs one target per engine"):
        drivers._project_group(None, t, None, optimize_noise=True, mdf=object())
    # optimize_noise, noise_init and (through args) noise_regularize are arguments now; anything unknown is still refused by name
    with pytest.raises(TypeError, match=r"unsupported arguments \['noise_maps'\]"):
        drivers._project_group(None, t, None, optimize_noise=True, noise_maps=1)


@pytest.mark.parametrize("n_sets", [1, 3])
def test_set_reference_equals_the_per_map_reference_map_by_map(n_sets):
    """One autograd pass over the whole buffer against noise_regularize_grad per map, both float64: the same expression per map, the maps
    do not interact -- a few float64 roundings of the largest element; nothing outside the maps gets a gradient."""
    offsets, extent, stride = gapped_table(SIDES)
    x = make_sets(make_map, SIDES, offsets, stride, n_sets, 500)
    vals, grad = regularize_sets(x, SIDES, offsets)
    covered = torch.zeros_like(grad, dtype=torch.bool)
    for t in range(n_sets):
        for m, s in enumerate(SIDES):
            v, g = noise_regularize_grad(map_of(x, t, m, SIDES, offsets))
            assert abs(float(vals[t, m] - v)) <= 8 * 2.0 ** -52 * float(v), (t, m)
            got = map_of(grad, t, m, SIDES, offsets)
            assert float((got - g).abs().max()) <= 8 * 2.0 ** -52 * float(g.abs().max()), (t, m)
            covered[t, offsets[m]:offsets[m] + s * s] = True
    assert not bool(grad[~covered].any())
    # different data in every set: no two sets have the same value row
    assert all(not torch.equal(vals[a], vals[b]) for a in range(n_sets) for b in range(a))


def test_set_normalise_reference_moves_the_live_sets_only():
    offsets, extent, stride = gapped_table(SIDES)
    x = make_sets(make_map, SIDES, offsets, stride, 3, 600, fill=0.0) * 1.7 + 0.3
    y = normalize_sets(x, SIDES, offsets, live=[0])
    assert torch.equal(y[1:], x[1:].double())
    for m in range(len(SIDES)):
        v = map_of(y, 0, m, SIDES, offsets)
        assert abs(float(v.mean())) < 1e-14 and abs(float(v.std(unbiased=True)) - 1) < 1e-14
