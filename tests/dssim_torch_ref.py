"""The continuous DSSIM of gradient mode (`mgf_dssim_f32` / `mgf_dssim_grad_f32`) restated in torch, float64, differentiable: skimage's SSIM
(oracle.loss_ref.ssim_ref, unchanged: 7x7 uniform window, sample covariance, K1 0.01, K2 0.03, the positions whose window lies whole inside
the image, mean over positions and channels) applied to p = 127.5 img + 127.5 without the uint8 quantisation.  A helper of the tests, not a
test module; tests/test_dssim_gradient_ref.py pins it on oracle.loss_ref."""
import torch


def dssim_torch(img, target, data_range=255.0):
    """img [n,c,h,w], target [c,h,w] or [n,c,h,w] (any float dtype) -> dssim per sample [n], float64."""
    p, q = 127.5 * img.double() + 127.5, 127.5 * target.double() + 127.5
    q = q.expand_as(p) if q.ndim == 4 else q[None].expand_as(p)
    box = lambda x: torch.nn.functional.avg_pool2d(x, 7, 1)
    ux, uy, uxx, uyy, uxy = box(p), box(q), box(p * p), box(q * q), box(p * q)
    cov = 49.0 / 48.0
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return (1 - s.mean(dim=(1, 2, 3))) / 2


def dssim_torch_grad(img, target, data_range=255.0):
    """(value [n] float64, d value[i] / d img[i] [n,c,h,w] float64) by autograd."""
    x = img.detach().double().clone().requires_grad_(True)
    v = dssim_torch(x, target, data_range)
    v.sum().backward()
    return v.detach(), x.grad
