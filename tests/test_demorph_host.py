"""Host side of latent de-morphing: the closed form drivers.demorph_latent against merge_morph's own blend, its refusals, the C ABI
declarations of csrc/demorph.hip and the module entry `python -m morphganformer_amd.demorph` (which adds no subcommand to cli.build_parser())."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["mgf_latent_mix_f32", "mgf_latent_mix_bwd_f32", "mgf_joint_losses_f32"]
DRAWS = 200


@pytest.mark.parametrize("shape", [(1, 17, 32), (1, 17, 18, 32)], ids=["z", "wplus"])
@pytest.mark.parametrize("alpha", [0.1, 0.3, 0.5, 0.7, 0.9])
def test_demorph_latent_inverts_the_blend(alpha, shape):
    """w_M = _blend_latents(w_A, w_B, alpha), then demorph_latent(w_M, w_A, alpha) against w_B, per element, within
    2^-22 (|w_M| + (1 - alpha) |w_A|) / alpha: four float32 roundings that do not cancel (the blend's product alpha w_B and its sum, the
    subtraction, the division: each at most 2^-24 of a quantity <= |w_M| + (1 - alpha) |w_A|, then divided by alpha).  The product
    (1 - alpha) w_A is the same float32 number on both sides and cancels."""
    from morphganformer_amd import drivers
    rng = np.random.Generator(np.random.PCG64(int(alpha * 100) + len(shape)))
    worst = 0.0
    for _ in range(DRAWS if len(shape) == 3 else DRAWS // 10):
        wa, wb = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
        wm = drivers._blend_latents(wa, wb, alpha)
        got = drivers.demorph_latent(wm, wa, alpha)
        assert got.dtype == np.float32 and got.shape == shape
        bound = 2.0 ** -22 * (np.abs(wm.astype(np.float64)) + (1.0 - alpha) * np.abs(wa.astype(np.float64))) / alpha
        err = np.abs(got.astype(np.float64) - wb.astype(np.float64))
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (alpha, float((err / bound).max()))
    print(f"OBS demorph_latent alpha {alpha} {shape}: worst error {worst:.3f} of the bound")


def test_demorph_latent_takes_tensors_and_alpha_one():
    import torch
    from morphganformer_amd import drivers
    rng = np.random.Generator(np.random.PCG64(5))
    wa, wm = rng.standard_normal((1, 17, 32)).astype(np.float32), rng.standard_normal((1, 17, 32)).astype(np.float32)
    # alpha = 1: the morph IS the other contributor (0 * w_A subtracted, divided by 1)
    assert np.array_equal(drivers.demorph_latent(torch.from_numpy(wm), torch.from_numpy(wa), 1.0), wm)


@pytest.mark.parametrize("alpha", [0.0, -0.1, 1.0001, float("nan")])
def test_demorph_latent_refuses_alpha_outside_the_half_open_interval(alpha):
    from morphganformer_amd import drivers
    w = np.zeros((1, 17, 32), np.float32)
    with pytest.raises(ValueError, match=r"alpha must lie in \(0, 1\]"):
        drivers.demorph_latent(w, w, alpha)


def test_demorph_latent_refuses_mismatched_shapes():
    from morphganformer_amd import drivers
    with pytest.raises(ValueError, match="differ in shape"):
        drivers.demorph_latent(np.zeros((1, 17, 32), np.float32), np.zeros((1, 17, 18, 32), np.float32), 0.5)


def test_new_entries_are_declared_and_bound():
    from morphganformer_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "mgf.h")).read()
    declared = set(re.findall(r"\b(mgf_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_ENTRIES:
        assert name in declared, f"{name} is not declared in include/mgf.h"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound in _lib.py"
    assert "demorph.hip" in build.SOURCES


def test_module_entry_prints_its_help():
    r = subprocess.run([sys.executable, "-m", "morphganformer_amd.demorph", "--help"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    for opt in ["--model", "--morph", "--reference", "--w-morph", "--w-ref", "--alpha", "--out", "--no-lpips", "--biometric"]:
        assert opt in out, opt


def test_the_command_line_gains_no_subcommand():
    from morphganformer_amd import cli, demorph
    sub = next(a for a in cli.build_parser()._actions if hasattr(a, "choices") and isinstance(a.choices, dict))
    assert "demorph" not in sub.choices and "demorph" not in cli.COMMANDS
    assert sorted(sub.choices) == sorted(cli.COMMANDS)
    a = demorph.build_parser().parse_args(["--morph", "m.png", "--reference", "r.png", "--out", "o"])
    assert a.alpha == 0.5 and a.w_morph is None and a.w_ref is None and a.step == 5000 and a.pixel_term == "mse"
