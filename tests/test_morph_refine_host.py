"""CPU: the design of two-identity morph refinement and its host-side surface.

For convex weights every quadratic term of the pair objective equals the same term against ONE blended target plus a constant:
    (1-a) LPIPS(x,Ta) + a LPIPS(x,Tb) = sum_taps mean_hw sum_c lin_c (u_x - u)^2 + a (1-a) LPIPS(Ta,Tb),   u = (1-a) u_a + a u_b
    (1-a) MSE(x,Ta)   + a MSE(x,Tb)   = MSE(x, (1-a) Ta + a Tb)                 + a (1-a) MSE(Ta,Tb)
which is what lets gradient mode run its single-target kernels once per step for a target pair.  Pinned here on the oracle in float64."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lpips_parts():
    from morphganformer_amd.lpips import WEIGHTS_DIR
    from oracle.loss_ref import backbone_random
    bb = {k: torch.as_tensor(v).double() for k, v in backbone_random("squeeze", 0).items()}
    lin = np.load(os.path.join(WEIGHTS_DIR, "lpips_lin_squeeze.npz"))
    lins = [torch.from_numpy(lin[f"lin{i}"]).double().reshape(-1) for i in range(7)]
    torch.manual_seed(5)
    x, ta, tb = (torch.rand(1, 3, 64, 64, dtype=torch.float64) * 2 - 1 for _ in range(3))
    return bb, lins, x, ta, tb


@pytest.mark.parametrize("alpha", [0.5, 0.3])
def test_pair_objective_collapses_to_a_blended_target_on_the_oracle(lpips_parts, alpha):
    from oracle.loss_ref import lpips_ref, mse_ref, normalize_tensor_ref, scaling_layer_ref, squeeze_features_ref
    bb, lins, x0, ta, tb = lpips_parts
    a = alpha
    unit = lambda img: [normalize_tensor_ref(t) for t in squeeze_features_ref(bb, scaling_layer_ref(img).double())]

    def explicit(x):
        return ((1 - a) * lpips_ref(bb, lins, x, ta).sum() + a * lpips_ref(bb, lins, x, tb).sum(),
                (1 - a) * mse_ref(x, ta) + a * mse_ref(x, tb))

    def blended(x):
        ua, ub = unit(ta), unit(tb)
        lp = sum((lin.reshape(1, -1, 1, 1) * (u - ((1 - a) * p + a * q)).square()).sum(1).mean((1, 2)).sum()
                 for lin, u, p, q in zip(lins, unit(x), ua, ub))
        return (lp + a * (1 - a) * lpips_ref(bb, lins, ta, tb).sum(),
                mse_ref(x, (1 - a) * ta + a * tb) + a * (1 - a) * mse_ref(ta, tb))

    xe, xb = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    for (ve, vb), name in zip(zip(explicit(xe), blended(xb)), ("lpips", "mse")):
        assert ve.dtype == torch.float64
        assert abs(float(ve.detach()) - float(vb.detach())) <= 1e-12, name
        (ge,) = torch.autograd.grad(ve, xe, retain_graph=True)
        (gb,) = torch.autograd.grad(vb, xb, retain_graph=True)
        assert float((ge - gb).abs().max()) <= 1e-12 * float(ge.abs().max()), name


def test_pair_kernel_is_declared_and_exported():
    from morphganformer_amd import _lib, build
    assert "mgf_embed_pair_loss_f32" in _lib.EXPORTED_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "mgf.h")).read()
    assert "int mgf_embed_pair_loss_f32(" in hdr
    assert "morph_pair.hip" in build.SOURCES


def test_pair_kernel_returns_errors_before_any_launch():
    """NULL or contradictory arguments are error returns (reachable without a GPU: they are checked before the launch)."""
    from morphganformer_amd import _lib, build
    build.build()
    L = _lib.lib()
    p = 4096            # a non-NULL stand-in: every call below must fail its checks before anything is dereferenced or launched
    call = lambda **kw: L.mgf_embed_pair_loss_f32(*[{**dict(loss=p, demb=None, trace=None, emb=p + 64, ta=p + 128, tb=p + 192, alpha=p + 256, n=1, width=8,
                                                          stride=0, gamma=1.0, delta=0.0, metric=0, acc=0, step=None, rows=0, stream=None), **kw}[k]
                                                    for k in ("loss", "demb", "trace", "emb", "ta", "tb", "alpha", "n", "width", "stride", "gamma", "delta",
                                                              "metric", "acc", "step", "rows", "stream")])
    for bad in (dict(loss=None), dict(emb=None), dict(ta=None), dict(tb=None), dict(alpha=None), dict(n=0), dict(width=0), dict(metric=2),
                dict(stride=4), dict(trace=p + 512), dict(trace=p + 512, step=p + 1024, rows=0), dict(demb=p + 64)):
        assert call(**bad) == -1, bad
        assert b"embed_pair_loss" in L.mgf_last_error()


def test_refine_morph_rejects_bad_arguments_before_touching_a_device():
    from morphganformer_amd import drivers
    w = np.zeros((1, 17, 32), np.float32)
    with pytest.raises(ValueError, match="differ in shape"):
        drivers.refine_morph(None, w, np.zeros((1, 16, 32), np.float32), None, None)
    with pytest.raises(ValueError, match="gradient"):
        drivers.refine_morph(None, w, w, None, None, mode="literal")
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        drivers.refine_morph(None, w, w, None, None, alphas=(0.5, 1.5))


def test_cli_morph_takes_the_refine_flags_and_parses_as_before_without_them():
    from morphganformer_amd import cli
    ap = cli.build_parser()
    base = ["morph", "--model", "net.pkl", "--w1", "a.mat", "--w2", "b.mat", "--out", "o/a+b"]
    a = ap.parse_args(base + ["--alphas", "0,0.5,1"])
    assert (a.cmd, a.w1, a.w2, a.alphas, a.out, a.ratio, a.truncation_psi, a.gpus) == ("morph", "a.mat", "b.mat", "0,0.5,1", "o/a+b", 1.0, 0.7, "0")
    assert a.refine is False and a.image_a is None and a.image_b is None
    r = ap.parse_args(base + ["--refine", "--image-a", "a.png", "--image-b", "b.png", "--id-balance", "0.5", "--id-metric", "cosine", "--step", "6",
                              "--biometric", "iresnet18", "--biometric-random", "--gamma", "0.1", "--pixel-term", "dssim", "--latent-space", "w+",
                              "--lpips-random-backbone", "--net", "vgg"])
    assert r.refine and (r.image_a, r.image_b) == ("a.png", "b.png") and r.id_balance == 0.5 and r.id_metric == "cosine" and r.step == 6
    assert (r.biometric, r.gamma, r.pixel_term, r.latent_space, r.net) == ("iresnet18", 0.1, "dssim", "w+", "vgg")
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--id-metric", "euclid"])


def test_gradient_engine_names_the_pair_parameters():
    """target_b and its companions are named parameters of GradientProjectionEngine, not swallowed by **ignored."""
    import inspect
    from morphganformer_amd.projection import GradientProjectionEngine
    params = inspect.signature(GradientProjectionEngine.__init__).parameters
    for name, default in (("target_b", None), ("morph_alpha", 0.5), ("id_balance", 0.0), ("id_metric", "mse"), ("lm_target_b", None)):
        assert name in params and params[name].default == default, name
