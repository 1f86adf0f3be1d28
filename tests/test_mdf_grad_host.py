"""The MDF backward's host side, no GPU: the adjoint-weight helper, a float64 restatement of the backward in the forward's frames
(include/mgf.h, "MDF backward") against torch autograd through test_mdf_host.mdf_taps64 and against the reference's own gradient
(tests/golden/mdf_grad_tiny.npz, tools/make_mdf_grad_golden.py), and the CLI's choice of a differentiable loss in gradient mode."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from morphganformer_amd import mdf  # noqa: E402
from test_mdf_host import GOLDEN, mdf_taps64  # noqa: E402

GOLDEN_GRAD = os.path.join(ROOT, "tests", "golden", "mdf_grad_tiny.npz")


def ring(h, w, r, dev="cpu"):
    m = torch.zeros(h, w, dtype=torch.float64, device=dev)
    m[r:h - r, r:w - r] = 1.0
    return m


def dlrelu(a):
    return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, mdf.SLOPE))


def frames_grad64(sd, target, cand, scale=1.0):
    """scale * d loss / d cand of one discriminator (sum over its taps of the means), restated in frames: every map an h x w frame,
    valid on its ring, the backward of include/mgf.h with its ring zeroing.  float64 torch; target [1,3,h,w], cand [n,3,h,w]."""
    dev = cand.device
    L = [(torch.as_tensor(w, device=dev), torch.as_tensor(b, device=dev)) for w, b in mdf.fold_bn(sd)]
    h, w = cand.shape[-2:]

    def fwd(img):
        a = [F.leaky_relu(F.conv2d(img, L[0][0], L[0][1], padding=1), mdf.SLOPE)]
        for k in range(mdf.BODY_BLOCKS):
            a.append(F.leaky_relu(F.conv2d(a[-1], L[1 + k][0], L[1 + k][1], padding=1), mdf.SLOPE))
        return a, F.conv2d(a[-1], L[-1][0], L[-1][1], padding=1)

    (at, x3t), (a, x3) = fwd(target), fwd(cand)
    N = a[0].shape[1]
    c1, c2, c3 = N * (h - 2) * (w - 2), N * (h - 8) * (w - 8), (h - 10) * (w - 10)
    adj = lambda g, W: F.conv2d(g, torch.as_tensor(mdf.adjoint_weights(W.cpu().numpy()), device=dev), padding=1)
    g3 = scale * 2 / c3 * (x3 - x3t) * ring(h, w, 5, dev)
    d = (adj(g3, L[-1][0]) + scale * 2 / c2 * (a[3] - at[3])) * dlrelu(a[3]) * ring(h, w, 4, dev)
    for k in reversed(range(mdf.BODY_BLOCKS)):
        d = adj(d, L[1 + k][0]) * dlrelu(a[k]) * ring(h, w, k + 1, dev)
        if k == 0:
            d = d + scale * 2 / c1 * (a[0] - at[0]) * dlrelu(a[0]) * ring(h, w, 1, dev)
    return adj(d, L[0][0])


def autograd_grad64(sd, target, cand):
    y = cand.clone().requires_grad_()
    tx, ty = mdf_taps64(sd, target), mdf_taps64(sd, y)
    sum(((ty[k] - tx[k].detach()) ** 2).mean(dim=(1, 2, 3)).sum() for k in range(3)).backward()
    return y.grad


@pytest.mark.parametrize("c", [32, 64, 128])
def test_adjoint_weights_are_the_transpose(c):
    rng = np.random.default_rng(c)
    W = rng.standard_normal((c, c, 3, 3))
    h, w = 9, 11
    x = torch.from_numpy(rng.standard_normal((1, c, h, w)))
    g = torch.from_numpy(rng.standard_normal((1, c, h - 2, w - 2)))
    lhs = float((F.conv2d(x, torch.from_numpy(W)) * g).sum())
    gf = torch.zeros(1, c, h, w, dtype=torch.float64)
    gf[..., 1:-1, 1:-1] = g                                  # the frame of g, zero outside ring 1
    rhs = float((x * F.conv2d(gf, torch.from_numpy(mdf.adjoint_weights(W)), padding=1)).sum())
    assert abs(lhs - rhs) <= 1e-10 * abs(lhs)
    At = mdf.adjoint_weights(W)
    assert At.shape == (c, c, 3, 3) and np.array_equal(At[3, 5, 0, 2], W[5, 3, 2, 0])


@pytest.mark.parametrize("N,hw,n", [(32, (13, 12), 2), (64, (17, 23), 1)])
def test_frame_restatement_matches_autograd(N, hw, n):
    sd = mdf.random_discriminators(3, (N,))[0]
    g = torch.Generator().manual_seed(N)
    t = torch.tanh(torch.randn(1, 3, *hw, generator=g, dtype=torch.float64))
    y = (t + 0.3 * torch.randn(n, 3, *hw, generator=g, dtype=torch.float64)).clamp(-1, 1)
    ref = autograd_grad64(sd, t, y)
    got = frames_grad64(sd, t, y, scale=1.0)
    assert float((got - ref).abs().max()) <= 1e-10 * float(ref.abs().max())
    assert float(ref.abs().max()) > 0


@pytest.mark.parametrize("case", ["asc8", "asc5", "desc9"])
def test_frame_restatement_reproduces_reference_gradient(case):
    g, gg = np.load(GOLDEN), np.load(GOLDEN_GRAD)
    assert hashlib.sha256(g["target"].tobytes() + g["candidates"].tobytes()).hexdigest() == str(gg["inputs_digest"])
    seed, nd, scales, asc = (int(v) for v in g[f"{case}_cfg"])
    Ds = mdf.random_discriminators(seed, (32,) * 4 + (64,) * 4 + ((128,) if nd == 9 else ()))
    t, y = torch.from_numpy(g["target"]).double(), torch.from_numpy(g["candidates"]).double()
    got = sum(frames_grad64(Ds[i if asc else len(Ds) - 1 - i], t, y) for i in range(scales)) / y.shape[0]
    ref = torch.from_numpy(gg[f"{case}_grad"]).double()
    # the reference runs in float32: where a pre-activation sits within its rounding of 0 the LeakyReLU slope flips (1 vs 0.2) against
    # float64.  Observed: relative L2 1.5e-4 / 7.4e-7 / 1.5e-4 and max 1.8e-3 / 8.0e-7 / 2.1e-3 of max|g| for asc8 / asc5 / desc9
    assert float((got - ref).norm() / ref.norm()) <= 5e-4
    assert float((got - ref).abs().max()) <= 5e-3 * float(ref.abs().max())


def test_cli_builds_a_differentiable_loss_in_gradient_mode():
    from morphganformer_amd import cli
    base = ["project", "--model", "m.pkl", "--image", "a.png", "--mdf-random", "--mdf-scales", "3", "--mdf-descending"]
    grad = cli.mdf_options(cli.build_parser().parse_args(base + ["--mode", "gradient"]))
    lit = cli.mdf_options(cli.build_parser().parse_args(base))
    assert grad == {"num_scales": 3, "is_ascending": 0, "differentiable": True}
    assert lit == {"num_scales": 3, "is_ascending": 0, "differentiable": False}
