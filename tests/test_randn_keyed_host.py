"""Host checks of noise_mode="keyed" (no GPU): the integer Philox4x32-10 of tests/randn_keyed_numpy_ref.py against the published
known-answer vectors and a second scalar implementation, the statistics of the restated stream, the header's declaration and the binding
derived from it, and the evolution entry's --noise-mode option."""
import os
import re

import numpy as np
import pytest

from randn_keyed_numpy_ref import map_normals, philox4x32_10, philox4x32_10_scalar, randn_keyed_ref, uniform_f32

KEY = 0x5EED0123456789AB          # the fixed key of the statistics below


@pytest.mark.parametrize("ctr, key, want", [
    # Random123's kat_vectors, philox4x32 with 10 rounds
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(ctr, key, want):
    assert tuple(philox4x32_10_scalar(ctr, key)) == want
    assert tuple(int(w) for w in philox4x32_10(*ctr, *key)) == want


def test_array_and_scalar_philox_agree():
    rng = np.random.Generator(np.random.PCG64(7))
    ctr = rng.integers(0, 2 ** 32, size=(64, 4), dtype=np.uint64)
    k0, k1 = 0x89ABCDEF, 0x01234567
    got = np.stack(philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], k0, k1), axis=1)
    want = np.array([philox4x32_10_scalar(row, (k0, k1)) for row in ctr.tolist()], dtype=np.uint64)
    assert np.array_equal(got, want)


def test_uniform_restates_the_two_float32_operations():
    u = uniform_f32(np.array([0, 1, 2 ** 24 + 1, 2 ** 32 - 1], dtype=np.uint64))
    assert u.dtype == np.float32
    assert u[0] == np.float32(0.5) * np.float32(2.0 ** -32) and u[0] > 0
    assert u[2] == np.float32(2 ** 24) * np.float32(2.0 ** -32)          # 2^24 + 1 rounds to even, + 0.5 is absorbed
    assert u[3] == np.float32(1.0)                                        # the largest word rounds up to 1: the kernel clamps it below 1


def test_statistics_of_the_restated_stream():
    """2^20 draws per map (one 1024^2 map).  Bounds: about 5 sigma (sigma of the mean 1e-3, of the variance 1.4e-3, of a correlation 1e-3)."""
    n = 1 << 20
    base = map_normals(1024, 3, 17, 1, KEY)
    assert base.shape == (n,) and np.isfinite(base).all() and np.abs(base).max() <= 6.7
    mean, var = base.mean(), base.var()
    print(f"mean {mean:.3e}  var - 1 {var - 1:.3e}")
    assert abs(mean) <= 5e-3 and abs(var - 1.0) <= 7e-3
    for name, other in (("step", map_normals(1024, 3, 18, 1, KEY)), ("layer", map_normals(1024, 4, 17, 1, KEY)),
                        ("aux", map_normals(1024, 3, 17, 2, KEY))):
        corr = np.corrcoef(base, other)[0, 1]
        print(f"corr({name}, {name} + 1) {corr:.3e}")
        assert abs(corr) <= 5e-3, (name, corr)


def test_buffer_layout_and_per_sample_key():
    sides, n = [4, 8], 3
    ref = randn_keyed_ref(sides, n, KEY, [5], step_stride=0, step_add=1, step_max=6, aux0=1, aux_add=0)
    assert ref.shape == (n * (16 + 64),)
    # layer-major: layer 0's n maps, then layer 1's; sample j sits at step min(5 + j, 6)
    assert np.array_equal(ref[16:32], map_normals(4, 0, 6, 1, KEY)) and np.array_equal(ref[32:48], map_normals(4, 0, 6, 1, KEY))
    assert np.array_equal(ref[48 + 64:48 + 128], map_normals(8, 1, 6, 1, KEY))
    per = randn_keyed_ref(sides, n, KEY, [5, 9, 2], step_stride=1, step_add=0, aux0=2, aux_add=1)
    assert np.array_equal(per[32:48], map_normals(4, 0, 2, 4, KEY))


def test_entry_point_is_declared_and_bound():
    from morphganformer_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mgf.h")).read()
    assert re.search(r"int mgf_randn_keyed_f32\(float\* out, const int32_t\* sides, int32_t n_layers, int32_t n, const uint64_t\* key,", header)
    assert "mgf_randn_keyed_f32" in _lib.EXPORTED_SYMBOLS
    res, args = _lib._SIGS["mgf_randn_keyed_f32"]
    P, I32 = _lib.vp, _lib.i32
    assert res is _lib.C.c_int and args == [P, P, I32, I32, P, P, I32, I32, I32, I32, I32, P] and len(args) == 12


def test_evolution_entry_takes_noise_mode():
    from morphganformer_amd import evolution
    ap = evolution.build_parser()
    assert ap.parse_args(["--image", "f.png"]).noise_mode == "random"                     # what the entry did before the option existed
    for mode in ("random", "const", "keyed"):
        assert ap.parse_args(["--image", "f.png", "--noise-mode", mode]).noise_mode == mode
    with pytest.raises(SystemExit):
        ap.parse_args(["--image", "f.png", "--noise-mode", "inject"])


def test_demorph_engine_refuses_keyed_by_name():
    from morphganformer_amd._lib import MgfError
    from morphganformer_amd.demorph import DemorphEngine
    with pytest.raises(MgfError, match="noise_mode='keyed'"):
        DemorphEngine(None, None, None, None, None, 1.0, noise_mode="keyed")
