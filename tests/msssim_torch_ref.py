"""The multi-scale SSIM loss of `mgf_msssim_f32` / `mgf_msssim_grad_f32` (the definition in include/mgf.h) restated in torch, float64,
differentiable.  A helper of the tests, not a test module.  No library with this function is installed, so tests/test_msssim_ref.py pins this
file independently: closed forms, and an explicit-loop NumPy restatement that shares no code with it.

The clamped branch (some level mean <= 0: ms = 0, gradient defined as zero) is written with torch.where on a safe base, so autograd returns
exact zeros there and never 0 * inf."""
import torch

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def msssim_weights(levels):
    w = torch.tensor(WEIGHTS[:levels], dtype=torch.float64)
    return (w / w.sum()).tolist()


def gauss_window():
    x = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-x * x / (2 * 1.5 ** 2))
    return g / g.sum()


def _blur(x, g):
    """Separable valid filter of [n,c,h,w]: rows (along w), then columns."""
    c = x.shape[1]
    x = torch.nn.functional.conv2d(x, g.reshape(1, 1, 1, 11).expand(c, 1, 1, 11), groups=c)
    return torch.nn.functional.conv2d(x, g.reshape(1, 1, 11, 1).expand(c, 1, 11, 1), groups=c)


def level_means(img, target, levels=5, data_range=255.0):
    """v [n,c,levels] float64: per level the mean over positions of cs, of ssim = l cs on the last."""
    p, q = 127.5 * img.double() + 127.5, 127.5 * target.double() + 127.5
    q = q.expand_as(p) if q.ndim == 4 else q[None].expand_as(p)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    g = gauss_window()
    v = []
    for j in range(levels):
        if min(p.shape[2:]) < 11:
            raise ValueError(f"msssim: level {j} is {p.shape[2]}x{p.shape[3]}, smaller than the 11x11 window")
        ux, uy, exx, eyy, exy = _blur(p, g), _blur(q, g), _blur(p * p, g), _blur(q * q, g), _blur(p * q, g)
        vx, vy, vxy = exx - ux * ux, eyy - uy * uy, exy - ux * uy
        cs = (2 * vxy + c2) / (vx + vy + c2)
        if j == levels - 1:
            cs = cs * (2 * ux * uy + c1) / (ux * ux + uy * uy + c1)
        v.append(cs.mean(dim=(2, 3)))
        if j < levels - 1:
            pad = [s % 2 for s in p.shape[2:]]
            p = torch.nn.functional.avg_pool2d(p, 2, 2, padding=pad)
            q = torch.nn.functional.avg_pool2d(q, 2, 2, padding=pad)
    return torch.stack(v, dim=2)


def msssim_torch(img, target, levels=5, weights=None, data_range=255.0):
    """img [n,c,h,w], target [c,h,w] or [n,c,h,w] (any float dtype) -> msssim_loss per sample [n], float64."""
    w = torch.tensor(msssim_weights(levels) if weights is None else list(weights), dtype=torch.float64)
    v = level_means(img, target, levels, data_range)
    ok = (v > 0).all(dim=2)
    safe = torch.where(ok[..., None], v, torch.ones_like(v))
    ms = torch.where(ok, (safe ** w).prod(dim=2), torch.zeros_like(ok, dtype=torch.float64))
    return 1 - ms.mean(dim=1)


def msssim_torch_grad(img, target, levels=5, weights=None, data_range=255.0):
    """(value [n] float64, d value[i] / d img[i] [n,c,h,w] float64) by autograd."""
    x = img.detach().double().clone().requires_grad_(True)
    v = msssim_torch(x, target, levels, weights, data_range)
    v.sum().backward()
    return v.detach(), x.grad
