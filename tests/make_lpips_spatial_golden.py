"""Generator of tests/golden/lpips_spatial.npz (run by hand where the reference tree is present; not collected by pytest):

    python tests/make_lpips_spatial_golden.py

The REFERENCE's own PNetLin (lpips/networks_basic.py:26-92) with spatial=True, on the tap tensors already committed in
tests/golden/lpips_dist.npz standing where the backbone's output would be -- its `upsample` (:20-24), lin heads (vendored weights) and sum
(:85-87) run verbatim.  Stored: `{net}_spatial_val` [2,1,H,H], `{net}_spatial_res_i` (res[0] is the running total there: the reference's
in-place `val += res[l]` aliases it) and `{net}_H`.  Outputs only."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# image side per net: every tap side of the lpips_dist.npz tensors (squeeze 9/5/3/2, vgg 8/4/2, alex 7/3) up-samples to exactly H under
# torch's floor(h * (H / h)) rule; one side with a scalar tail, one multiple of 4, one odd
SIDES = {"squeeze": 18, "vgg": 16, "alex": 21}
CHNS = {"squeeze": 7, "vgg": 5, "alex": 5}


def main():
    from oracle.make_golden import _reference_pnetlin, import_reference_lpips
    _, nb = import_reference_lpips()
    g = np.load(os.path.join(ROOT, "tests", "golden", "lpips_dist.npz"))
    out = {}
    with torch.no_grad():
        for net, H in SIDES.items():
            L = CHNS[net]
            t0 = [g[f"{net}_tap0_{i}"] for i in range(L)]
            t1 = [g[f"{net}_tap1_{i}"] for i in range(L)]
            for t in t0:
                assert t.shape[2] == t.shape[3] and int(math.floor(float(t.shape[2]) * (1. * H / t.shape[2]))) == H, (net, t.shape, H)
            seq = iter([t0, t1])
            m = _reference_pnetlin(nb, net, lambda x: [torch.from_numpy(a) for a in next(seq)])
            m.spatial = True
            img = torch.zeros(2, 3, H, H)
            val, res = m.forward(img, img, retPerLayer=True)
            assert tuple(val.shape) == (2, 1, H, H), val.shape
            out[f"{net}_spatial_val"] = val.numpy().astype(np.float32)
            for i in range(L):
                assert tuple(res[i].shape) == (2, 1, H, H)
                out[f"{net}_spatial_res_{i}"] = res[i].numpy().astype(np.float32)
            out[f"{net}_H"] = np.int32(H)
    path = os.path.join(ROOT, "tests", "golden", "lpips_spatial.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
