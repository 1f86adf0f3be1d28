"""CPU pins of the MobileFaceNet embedder's ground truth: the seeded state dict has the reference module's names and shapes, and the
functional restatement the GPU tests compare against (tests/mobilefacenet_torch_ref.py) reproduces what the reference module itself
recorded in tests/golden/mobilefacenet.npz (tools/make_mobilefacenet_golden.py) -- in float32 within the module's own
float32-against-float64 distance, in float64 to rounding."""
import numpy as np
import pytest
import torch

from mobilefacenet_torch_ref import as_state, embedding_grad, fixture_gradients


@pytest.fixture(scope="module")
def fx(golden):
    from morphganformer_amd.mobilefacenet import random_state
    g = golden("mobilefacenet.npz")
    f32, f64 = fixture_gradients(g)
    return g, random_state(0), f32, f64


def test_random_state_has_the_reference_names_and_shapes(fx):
    g, sd, _, _ = fx
    assert sorted(sd) == list(g["names"])
    assert [" ".join(map(str, sd[k].shape)) for k in sorted(sd)] == list(g["shapes"])
    assert all(v.dtype == np.float32 for v in sd.values())
    stats = ("running_mean", "running_var")
    assert sum(v.size for k, v in sd.items() if not k.endswith(stats)) == 1200512 == int(g["parameters"])
    slopes = [v for k, v in sd.items() if k.endswith("layers.2.weight") and v.ndim == 1]
    assert len(slopes) == 2 + 2 * 15 + 1 and all(((s > 0.1) & (s < 0.4)).all() for s in slopes)


def test_fixture_is_one_on_which_the_reference_agrees_with_itself(fx):
    g, _, f32, f64 = fx
    for k in ("r_emb", "r_grad_l2", "r_grad_max"):
        assert np.isfinite(g[k]) and 0 < float(g[k]) < 1e-4
    assert abs(np.abs(g["embedding"] - g["embedding64"]).max() / np.abs(g["embedding64"]).max() - float(g["r_emb"])) < 1e-9
    assert abs(np.linalg.norm((f32 - f64).ravel()) / np.linalg.norm(f64.ravel()) - float(g["r_grad_l2"])) < 1e-9
    assert g["x"].shape == (2, 3, 112, 112) and np.abs(g["x"]).max() <= 1


def test_helper_float32_within_the_reference_own_distance(fx):
    g, sd, _, f64 = fx
    emb, grad = embedding_grad(as_state(sd, torch.float32), torch.from_numpy(g["x"]), torch.from_numpy(g["v"]))
    e64 = g["embedding64"]
    assert np.abs(emb.numpy() - e64).max() <= max(4 * float(g["r_emb"]), 1e-6) * np.abs(e64).max()
    d = grad.numpy().astype(np.float64) - f64
    assert np.linalg.norm(d.ravel()) <= max(4 * float(g["r_grad_l2"]), 1e-6) * np.linalg.norm(f64.ravel())
    assert np.abs(d).max() <= max(4 * float(g["r_grad_max"]), 1e-6) * np.abs(f64).max()


def test_helper_float64_reproduces_the_float64_rows(fx):
    g, sd, _, f64 = fx
    stages = []
    from mobilefacenet_torch_ref import mobilefacenet_torch
    s64 = as_state(sd, torch.float64)
    with torch.no_grad():
        mobilefacenet_torch(s64, torch.from_numpy(g["x"]).double(), stages)
    emb, grad = embedding_grad(s64, torch.from_numpy(g["x"]).double(), torch.from_numpy(g["v"]).double())
    assert np.abs(emb.numpy() - g["embedding64"]).max() <= 1e-12 * np.abs(g["embedding64"]).max()
    assert np.abs(grad.numpy() - f64).max() <= 1e-12 * np.abs(f64).max()
    # the recorded stage statistics are the float32 module's: the float64 helper sits within float32 rounding of them
    assert len(stages) == 9
    for s, m, r in zip(stages, g["stage_mean"], g["stage_rms"]):
        assert abs(float(s.mean()) - m) <= 1e-5 * r and abs(float(s.square().mean().sqrt()) - r) <= 1e-5 * r
