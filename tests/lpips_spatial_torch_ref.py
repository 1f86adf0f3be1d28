"""The spatial path of PNetLin.forward (lpips/networks_basic.py:20-24,75-76,85-87) restated in float64 on the oracle's building blocks:
every tap's lin-weighted squared difference of unit-normalised features, up-sampled bilinearly (torch.nn.Upsample with the reference's
scale factor 1. * H / h, align_corners=False) to the image size, and the taps summed.  Pinned by tests/golden/lpips_spatial.npz (the
reference's own PNetLin with spatial=True on injected tap tensors; tests/make_lpips_spatial_golden.py)."""
import torch

from oracle.loss_ref import (backbone_random, normalize_tensor_ref, scaling_layer_ref, sequential_features_ref, squeeze_features_ref)


def upsample_ref(m, H):
    """`upsample(in_tens, out_H=H)` (networks_basic.py:20-24): ONE scale factor, derived from the height, for both axes."""
    scale = 1. * H / m.shape[2]
    return torch.nn.Upsample(scale_factor=scale, mode="bilinear", align_corners=False)(m)


def tap_maps_ref(taps0, taps1, lins):
    """The un-up-sampled per-tap maps [n,1,h,w] in float64: `self.lins[kk].model(diffs[kk])` (dropout = identity in eval)."""
    maps = []
    for a, b, lin in zip(taps0, taps1, lins):
        a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
        d = (normalize_tensor_ref(a) - normalize_tensor_ref(b)).square()
        maps.append((d * torch.as_tensor(lin).double().reshape(1, -1, 1, 1)).sum(1, keepdim=True))
    return maps


def spatial_from_taps_ref(taps0, taps1, lins, H):
    """-> (val [n,1,H,H], up-sampled per-tap maps, un-up-sampled per-tap maps), float64; the per-tap list is un-aliased."""
    maps = tap_maps_ref(taps0, taps1, lins)
    ups = [upsample_ref(m, H) for m in maps]
    val = ups[0].clone()
    for u in ups[1:]:
        val = val + u
    return val, ups, maps


def lpips_spatial_ref(net, lins, img0, img1, seed=0):
    """The whole chain on the oracle's backbone (seeded random weights, as PerceptualLoss(backbone_seed=seed) uses), float64."""
    bb = {k: v.double() for k, v in backbone_random(net, seed).items()}
    feats = (lambda x: squeeze_features_ref(bb, x)) if net == "squeeze" else (lambda x: sequential_features_ref(net, bb, x))
    x0, x1 = torch.as_tensor(img0).double(), torch.as_tensor(img1).double()
    return spatial_from_taps_ref(feats(scaling_layer_ref(x0)), feats(scaling_layer_ref(x1)), lins, x0.shape[2])
