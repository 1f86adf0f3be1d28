"""float64 references of the LPIPS term's block mean (PerceptualLoss(pool_above=N)) for tests/test_lpips_pool_host.py,
tests/test_hip_lpips_pool.py and tests/test_hip_lpips_pool_loops.py:

    P x   [n, c, H/f, W/f] = x.reshape(n, c, H/f, f, W/f, f).mean((3, 5))                     block_mean_ref (differentiable torch)
    P^T y [n, c, H, W]     = y[.., Y, X] / f^2 on the f x f block of (Y, X), 0 on the pixels no y covers    block_mean_adjoint_ref

and the two error bounds the kernels are held to, from the arithmetic alone (u = 2^-24, the unit roundoff of float32):

    forward  a float32 sum of f^2 terms in ANY order commits f^2 - 1 roundings, the scaling by 1 / f^2 at most two more (the constant, the
             product): |out - exact| <= (f^2 + 1) u mean_block |x|
    adjoint  dy / f^2 is one or two roundings: |dx - exact| <= 2 u |dy| / f^2, plus u |result| for the addition when accumulating"""
import torch

U = 2.0 ** -24


def block_mean_ref(x, f):
    """P x in float64; x [n, c, H, W] of any float dtype (gradients flow back to it)."""
    n, c, H, W = x.shape
    return x.double().reshape(n, c, H // f, f, W // f, f).mean((3, 5))


def block_mean_adjoint_ref(y, f, h, w):
    """P^T y in float64 as [n, c, h, w]; y [n, c, gh, gw] may cover less than [h / f, w / f] (the rest of dx is 0)."""
    n, c, gh, gw = y.shape
    out = torch.zeros(n, c, h, w, dtype=torch.float64)
    out[:, :, :gh * f, :gw * f] = (y.double() / (f * f)).repeat_interleave(f, dim=2).repeat_interleave(f, dim=3)
    return out


def block_mean_bound(x, f):
    """(f^2 + 1) u mean_block |x| per output pixel, float64 [n, c, H/f, W/f]."""
    return (f * f + 1) * U * block_mean_ref(x.double().abs(), f)


def block_mean_adjoint_bound(y, f, h, w, result=None):
    """2 u |dy| / f^2 per dx pixel (0 where no dy reaches), plus u |result| when accumulating into a dx that ends at `result`."""
    b = 2 * U * block_mean_adjoint_ref(y.double().abs(), f, h, w)
    return b if result is None else b + U * result.double().abs()


def pool_factor_ref(size, pool_above):
    """The three expressions tests/test_cli_parser_host.py lists, as one."""
    return size // pool_above if (pool_above and size > pool_above) else 1
