"""Pins tests/msssim_torch_ref.py, the float64 reference of the MS-SSIM kernels, without a library to compare with: closed forms, an
explicit-loop NumPy restatement that shares no code with it (no convolution call, the window as a double sum, the pooling written out), the
clamped branch, the level weights, and the host-side refusals that need no GPU."""
import math

import numpy as np
import pytest
import torch

from msssim_torch_ref import level_means, msssim_torch, msssim_torch_grad, msssim_weights as ref_weights

C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2


def _correlated(shape, seed):
    g = torch.Generator().manual_seed(seed)
    img = 0.7 * torch.randn(shape, generator=g)
    return img, (img + 0.3 * torch.randn(shape, generator=g)).clamp(-1, 1)


def test_identical_images_give_exactly_zero():
    for shape, levels in (((2, 3, 64, 64), 3), ((1, 2, 23, 44), 2), ((1, 3, 161, 176), 5)):
        img = 0.7 * torch.randn(shape, generator=torch.Generator().manual_seed(shape[2]))
        v = msssim_torch(img, img.clone(), levels)
        assert torch.equal(v, torch.zeros(shape[0], dtype=torch.float64)), (shape, v)


@pytest.mark.parametrize("levels", [1, 3, 5])
def test_constant_images_follow_the_closed_form(levels):
    """Constant images a, b: every variance and covariance vanishes, so every cs = 1 and the loss is 1 - l^{w_last} with the luminance term
    of the coarsest level.  A side that stays even down the pyramid keeps the pooled image constant (no zero padding enters)."""
    a, b = 0.3, -0.45
    side = 11 * 2 ** (levels - 1)
    img, tgt = torch.full((1, 2, side, side), a), torch.full((2, side, side), b)
    pa, pb = 127.5 * np.float64(np.float32(a)) + 127.5, 127.5 * np.float64(np.float32(b)) + 127.5
    want = 1 - ((2 * pa * pb + C1) / (pa * pa + pb * pb + C1)) ** ref_weights(levels)[-1]
    got = float(msssim_torch(img, tgt, levels)[0])
    assert abs(got - want) <= 1e-12, (got, want)


def _numpy_msssim(img, tgt, levels, weights):
    """The definition with explicit loops: img, tgt [c,h,w] float64 in [-1, 1] units -> loss."""
    g = np.array([math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)])
    g = g / g.sum()
    p, q = 127.5 * img + 127.5, 127.5 * tgt + 127.5
    ms_sum = 0.0
    for ch in range(p.shape[0]):
        x, y = p[ch], q[ch]
        ms, ok = 1.0, True
        for j in range(levels):
            h, w = x.shape
            acc = 0.0
            for r in range(h - 10):
                for s in range(w - 10):
                    ux = uy = exx = eyy = exy = 0.0
                    for u in range(11):
                        for t in range(11):
                            k, xv, yv = g[u] * g[t], x[r + u, s + t], y[r + u, s + t]
                            ux += k * xv; uy += k * yv; exx += k * xv * xv; eyy += k * yv * yv; exy += k * xv * yv
                    cs = (2 * (exy - ux * uy) + C2) / ((exx - ux * ux) + (eyy - uy * uy) + C2)
                    if j == levels - 1:
                        cs *= (2 * ux * uy + C1) / (ux * ux + uy * uy + C1)
                    acc += cs
            v = acc / ((h - 10) * (w - 10))
            ok = ok and v > 0
            if ok:
                ms *= v ** weights[j]
            if j < levels - 1:
                nx, ny = [], []
                for src, dst in ((x, nx), (y, ny)):
                    ph, pw = h % 2, w % 2
                    padded = np.zeros((h + 2 * ph, w + 2 * pw))              # an odd side: one zero on BOTH ends, counted in the divisor
                    padded[ph:ph + h, pw:pw + w] = src
                    out = np.zeros((padded.shape[0] // 2, padded.shape[1] // 2))
                    for r in range(out.shape[0]):
                        for s in range(out.shape[1]):
                            out[r, s] = (padded[2 * r, 2 * s] + padded[2 * r, 2 * s + 1] + padded[2 * r + 1, 2 * s] + padded[2 * r + 1, 2 * s + 1]) / 4
                    dst.append(out)
                x, y = nx[0], ny[0]
        ms_sum += ms if ok else 0.0
    return 1 - ms_sum / p.shape[0]


@pytest.mark.parametrize("shape,levels", [((1, 2, 23, 44), 2), ((1, 1, 11, 11), 1)])
def test_reference_equals_an_explicit_loop_restatement(shape, levels):
    img, tgt = _correlated(shape, 3)
    want = _numpy_msssim(img[0].double().numpy(), tgt[0].double().numpy(), levels, ref_weights(levels))
    got = float(msssim_torch(img, tgt[0], levels)[0])
    assert 0.0 < want < 0.5, want                                            # off the clamped branch: the comparison is not of zeros
    assert abs(got - want) <= 1e-12, (got, want)


def test_odd_side_pools_like_the_definition():
    """23 -> 12 rows, first output row half of the first input row (the zero pad is counted in the divisor)."""
    x = torch.arange(23 * 44, dtype=torch.float64).reshape(1, 1, 23, 44)
    y = torch.nn.functional.avg_pool2d(x, 2, 2, padding=[23 % 2, 44 % 2])
    assert tuple(y.shape[2:]) == (12, 22)
    assert torch.equal(y[0, 0, 0], (x[0, 0, 0, 0::2] + x[0, 0, 0, 1::2]) / 4)


def test_anticorrelated_images_sit_on_the_clamped_branch_with_zero_gradient():
    img, _ = _correlated((2, 3, 64, 64), 5)
    v, g = msssim_torch_grad(img, -img, 3)
    assert float(level_means(img, -img, 3).min()) < 0
    assert torch.equal(v, torch.ones(2, dtype=torch.float64)), v
    assert torch.isfinite(g).all() and torch.equal(g, torch.zeros_like(g))


def test_gradient_is_nonzero_and_finite_off_the_clamped_branch():
    img, tgt = _correlated((1, 3, 33, 21), 7)
    v, g = msssim_torch_grad(img, tgt, 2)
    assert float(level_means(img, tgt, 2).min()) > 0.5
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0 and 0 < float(v[0]) < 1


def test_level_weights():
    from morphganformer_amd.projection import MSSSIM_WEIGHTS, msssim_max_levels, msssim_weights
    assert msssim_weights(1) == [1.0]
    for levels in range(1, 6):
        w = msssim_weights(levels)
        assert len(w) == levels and abs(sum(w) - 1.0) <= 1e-15
        assert np.allclose(np.array(w) * sum(MSSSIM_WEIGHTS[:levels]), MSSSIM_WEIGHTS[:levels], rtol=1e-15)
        assert np.allclose(w, ref_weights(levels), rtol=1e-15, atol=0)
    assert abs(msssim_weights(5)[0] - 0.0448 / 1.0001) <= 1e-15
    assert [msssim_max_levels(*s) for s in ((1024, 1024), (256, 256), (161, 176), (160, 176), (64, 64), (11, 11), (10, 64))] == [5, 5, 5, 4, 3, 1, 0]


def test_host_side_refusals():
    from morphganformer_amd import cli
    from morphganformer_amd._lib import MgfError
    from morphganformer_amd.projection import ProjectionArgs, msssim_weights
    for bad in (0, 6, -1, 2.5):
        with pytest.raises(MgfError, match="msssim_levels"):
            ProjectionArgs(pixel_term="msssim", msssim_levels=bad)
        with pytest.raises(MgfError, match="msssim_levels"):
            msssim_weights(bad)
    assert ProjectionArgs(pixel_term="msssim").msssim_levels == 5
    assert ProjectionArgs(pixel_term="mse", msssim_levels=0).msssim_levels == 0          # the field is read with pixel_term="msssim" only
    ap = cli.build_parser()
    a = ap.parse_args(["project", "--model", "m.pkl", "--image", "a.png", "--mode", "gradient", "--pixel-term", "msssim", "--msssim-levels", "3"])
    assert (a.pixel_term, a.msssim_levels) == ("msssim", 3)
    a = ap.parse_args(["morph", "--model", "m.pkl", "--w1", "a.mat", "--w2", "b.mat", "--out", "o", "--refine", "--pixel-term", "msssim", "--msssim-levels", "4"])
    assert (a.pixel_term, a.msssim_levels, a.refine) == ("msssim", 4, True)
    assert ap.parse_args(["project", "--model", "m.pkl", "--image", "a.png"]).msssim_levels == 5
    with pytest.raises(SystemExit):
        ap.parse_args(["project", "--model", "m.pkl", "--image", "a.png", "--pixel-term", "ms-ssim"])
