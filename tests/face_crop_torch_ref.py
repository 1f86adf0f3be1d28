"""The aligned face crop of `mgf_face_crop_f32` / `mgf_face_crop_bwd_f32` (the definition in include/mgf.h) restated in torch, float64,
differentiable.  A helper of the tests, not a test module; tests/test_face_crop_host.py pins it against closed forms.

M maps a crop pixel index (u, v) to a source pixel index (x, y) = M (u, v, 1).  A source index x is the normalised grid_sample coordinate
g = (2 x + 1) / W - 1 under align_corners=False, and padding_mode="zeros" is the zero border; the area filter is the mean of S x S such samples."""
import math

import torch

MAX_S = 16


def subsamples(matrix, filter="area"):
    """S of one [2,3] matrix: clamp(ceil(sqrt(|det M[:, :2]|)), 1, 16) for the area filter, 1 for the bilinear one."""
    if filter == "bilinear":
        return 1
    assert filter == "area", filter
    m = torch.as_tensor(matrix, dtype=torch.float64)
    det = abs(float(m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]))
    return int(min(max(math.ceil(math.sqrt(det)), 1), MAX_S))


def face_crop_torch(x, matrices, size=112, filter="area"):
    """x [n,3,H,W] (any float dtype), matrices [2,3], [1,2,3] or [n,2,3] -> [n,3,size,size] float64, differentiable in x."""
    x = x.double()
    n, _, h, w = x.shape
    ms = torch.as_tensor(matrices, dtype=torch.float64).reshape(-1, 2, 3)
    assert ms.shape[0] in (1, n), ms.shape
    idx = torch.arange(size, dtype=torch.float64)
    out = []
    for k in range(n):
        m = ms[k if ms.shape[0] > 1 else 0]
        s = subsamples(m, filter)
        acc = torch.zeros(1, x.shape[1], size, size, dtype=torch.float64)
        for j in range(s):
            v = (idx + (j + 0.5) / s - 0.5)[:, None].expand(size, size)
            for i in range(s):
                u = (idx + (i + 0.5) / s - 0.5)[None, :].expand(size, size)
                sx = m[0, 0] * u + m[0, 1] * v + m[0, 2]
                sy = m[1, 0] * u + m[1, 1] * v + m[1, 2]
                grid = torch.stack([(2 * sx + 1) / w - 1, (2 * sy + 1) / h - 1], dim=-1)[None]
                acc = acc + torch.nn.functional.grid_sample(x[k:k + 1], grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        out.append(acc / (s * s))
    return torch.cat(out, dim=0)


def face_crop_torch_adjoint(dy, matrices, h, w, filter="area"):
    """A^T dy [n,3,h,w] float64 for dy [n,3,size,size], by autograd (the operator is linear in x, so any x gives the adjoint)."""
    dy = dy.double()
    x = torch.zeros(dy.shape[0], dy.shape[1], h, w, dtype=torch.float64, requires_grad=True)
    (face_crop_torch(x, matrices, dy.shape[-1], filter) * dy).sum().backward()
    return x.grad


def similarity(scale, degrees, tx, ty):
    """[2,3] float64: crop index -> source index, a rotation by `degrees` scaled by `scale`, then a shift."""
    c, s = scale * math.cos(math.radians(degrees)), scale * math.sin(math.radians(degrees))
    return torch.tensor([[c, -s, tx], [s, c, ty]], dtype=torch.float64)
