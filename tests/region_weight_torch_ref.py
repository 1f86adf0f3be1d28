"""float64 reference of the region-weighted image-space terms, composed from the oracle's pieces -- the backbone
features of oracle/loss_ref.py and its normalize_tensor_ref -- for tests/test_hip_region_weight.py and tests/test_region_weight_host.py:

    MSE_W(x, t)   = sum_c sum_p W[p] (x[c,p] - t[c,p])^2 / (C sum_p W[p])
    LPIPS_W(x, t) = sum_l sum_p omega_l[p] m_l[p],   omega_l = W_l / sum W_l,   W_l = adaptive_avg_pool2d(W, tap l's grid)  (float64, cast
                    to float32 once),   m_l[p] = sum_c lin_l[c] (unit(f_l(x))[c,p] - unit(f_l(t))[c,p])^2

Everything is differentiable torch, so the same functions serve as the loss of oracle.loss_ref.projection_gradient_ref."""
import torch
import torch.nn.functional as F

from oracle.loss_ref import normalize_tensor_ref, scaling_layer_ref, sequential_features_ref, squeeze_features_ref


def tap_weights_ref(W, side):
    """omega of one tap: W [n or 1, H, W] float64 -> [n or 1, h, w] float64 holding the float32 values the kernels multiply by."""
    wl = F.adaptive_avg_pool2d(W.double()[:, None], side)[:, 0]
    wl = wl / wl.sum(dim=(1, 2), keepdim=True)
    return wl.float().double()


def tap_distance_map_ref(f0, f1, lin):
    """m[p] of one tap, [n, h, w] (what mgf_lpips_layer_map_f32 defines), in the dtype of its inputs."""
    d = (normalize_tensor_ref(f0) - normalize_tensor_ref(f1)).square()
    return (d * lin.reshape(1, -1, 1, 1)).sum(1)


def lpips_weighted_ref(bb, lins, img0, img1, W, net="squeeze", per_layer=False):
    """LPIPS_W per sample, float64 [n].  img0 [n,3,H,W], img1 [n or 1,3,H,W] (any float dtype; gradients flow back to them),
    W [H,W] or [n or 1,H,W] >= 0."""
    bb64 = {k: v.double() for k, v in bb.items()}
    feats = (lambda x: squeeze_features_ref(bb64, x)) if net == "squeeze" else (lambda x: sequential_features_ref(net, bb64, x))
    W = torch.as_tensor(W).double()
    W = W[None] if W.dim() == 2 else W.reshape(-1, *W.shape[-2:])
    t0 = feats(scaling_layer_ref(img0.double()))
    t1 = feats(scaling_layer_ref(img1.double()))
    vals = []
    for a, b, lin in zip(t0, t1, lins):
        m = tap_distance_map_ref(a, b.expand_as(a), lin.double())
        vals.append((tap_weights_ref(W, tuple(a.shape[2:])) * m).sum(dim=(1, 2)))
    total = vals[0]
    for v in vals[1:]:
        total = total + v
    return (total, vals) if per_layer else total


def mse_weighted_ref(x, t, W):
    """MSE_W per sample, float64 [n]."""
    W = torch.as_tensor(W).double()
    W = W[None] if W.dim() == 2 else W.reshape(-1, *W.shape[-2:])
    d = (x.double() - t.double()).square() * W[:, None]
    return d.sum(dim=(1, 2, 3)) / (x.shape[1] * W.sum(dim=(1, 2)))


def weights(kind, h, w, seed=0):
    """The three test weights at h x w as float64 [h, w]: random positive, a half plane with exact zeros, a feathered disc."""
    if kind == "random":
        g = torch.Generator().manual_seed(seed)
        return torch.rand(h, w, generator=g, dtype=torch.float64) + 0.05
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    if kind == "half":
        return (xx >= w // 2).double()
    if kind == "disc":
        r = ((yy - (h - 1) / 2) ** 2 + (xx - (w - 1) / 2) ** 2).sqrt()
        return ((0.35 * min(h, w) - r) / (0.1 * min(h, w)) + 0.5).clamp(0.0, 1.0)
    raise ValueError(kind)
