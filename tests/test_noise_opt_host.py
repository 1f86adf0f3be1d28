"""CPU: the torch restatement of the noise regulariser (tests/noise_opt_torch_ref.py), the oracle of tests/test_hip_noise_opt.py, against the
reference driver's own function as recorded in tests/golden/noise_opt_reg.npz (tools/make_noise_opt_golden.py), and the host-side surface of
noise optimisation: the argument defaults and the refusals that need no GPU."""
import os

import numpy as np
import pytest
import torch

from noise_opt_torch_ref import noise_normalize_, noise_regularize, noise_regularize_grad, noise_regularize_map

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noise_opt_reg.npz")


@pytest.mark.parametrize("side", [4, 8, 32])
def test_restated_regulariser_equals_the_reference_function(side):
    """Sides 4 (one level, left and right neighbour coincide modulo 4), 8 (one level, exactly at the break) and 32 (three levels), float64:
    both sides evaluate the same expression in the same dtype, so the bound is a few float64 roundings of the value."""
    g = np.load(GOLDEN)
    x = torch.from_numpy(g[f"x{side}"])
    want = float(g[f"reg{side}"])
    got = float(noise_regularize_map(x[0]))
    assert want > 0 and abs(got - want) <= 8 * np.finfo(np.float64).eps * want, (got, want)


def test_restated_regulariser_sums_over_the_maps():
    g = np.load(GOLDEN)
    maps = [torch.from_numpy(g[f"x{s}"])[0] for s in (4, 8, 32)]
    want = float(g["reg_all"])
    assert abs(float(noise_regularize(maps)) - want) <= 8 * np.finfo(np.float64).eps * want


def test_restated_gradient_is_the_stencil_of_the_documentation():
    """One level (side 8): d reg / dx = 2A/N (left + right neighbour) + 2B/N (upper + lower), A and B the two means."""
    torch.manual_seed(3)
    x = torch.randn(1, 8, 8, dtype=torch.float64)
    _, g = noise_regularize_grad(x)
    A, B = (x * torch.roll(x, 1, 2)).mean(), (x * torch.roll(x, 1, 1)).mean()
    want = 2 * A / 64 * (torch.roll(x, 1, 2) + torch.roll(x, -1, 2)) + 2 * B / 64 * (torch.roll(x, 1, 1) + torch.roll(x, -1, 1))
    assert float((g - want).abs().max()) <= 1e-15


def test_restated_normalise_is_unbiased():
    torch.manual_seed(4)
    x = torch.randn(1, 16, 16, dtype=torch.float64) * 3 + 2
    noise_normalize_([x])
    assert abs(float(x.mean())) < 1e-14 and abs(float(x.std(unbiased=True)) - 1) < 1e-14


def test_arguments_carry_the_regulariser_weight_and_the_cli_reads_it():
    from morphganformer_amd.cli import build_parser
    from morphganformer_amd.projection import ProjectionArgs
    assert ProjectionArgs().noise_regularize == 1e5                   # the drivers' default (:243)
    a = build_parser().parse_args(["project", "--image", "x.png", "--mode", "gradient", "--optimize-noise", "--noise-init", "const",
                                   "--noise_regularize", "10"])
    assert a.optimize_noise and a.noise_init == "const" and a.noise_regularize == 10.0
    a = build_parser().parse_args(["project", "--image", "x.png"])
    assert not a.optimize_noise and a.noise_init == "randn"


def test_optimize_noise_outside_gradient_mode_is_refused():
    from morphganformer_amd import drivers
    with pytest.raises(ValueError, match="optimize_noise needs mode='gradient'"):
        drivers.project_image(None, None, None, None, mode="literal", optimize_noise=True)


def test_mat_keys_of_the_noise_maps(tmp_path):
    import scipy.io as sio
    from morphganformer_amd import drivers
    assert drivers.noise_mat_key("synthesis.b64.conv0") == "noise_b64_conv0"
    p = drivers.save_latent_mat(str(tmp_path / "w.mat"), np.zeros((1, 3, 4), np.float32),
                                noises={"synthesis.b4.conv1": torch.arange(16.0).reshape(1, 4, 4)})
    m = sio.loadmat(p)
    assert m["w"].shape == (1, 3, 4) and m["noise_b4_conv1"].shape == (4, 4) and m["noise_b4_conv1"][1, 2] == 6.0
