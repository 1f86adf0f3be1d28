"""Recipe of tests/golden/mdf_grad_tiny.npz: the gradient of the reference's own MDFLoss (mdfloss.py over SinGAN/models.py's
WDiscriminator) with respect to the candidates, on the seeded weights of morphganformer_amd.mdf.random_discriminators, on the CPU in
float32 -- the same three cases, target and candidates as tests/golden/mdf_tiny.npz (tools/make_mdf_golden.py).

    python tools/make_mdf_grad_golden.py --reference <checkout of the reference project>

The reference is imported from the given checkout at run time; nothing of it is copied.  Per case the file holds y.grad of the
reference's batch-mean call (`loss = criterion(x, y); loss.backward()` with y.requires_grad_(), modules in eval mode) and the batch
mean itself, plus a digest of the candidates so that a change of the draw is noticed.
"""
import argparse
import hashlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from make_mdf_golden import CASES  # noqa: E402
from morphganformer_amd.mdf import random_discriminators  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mdf_grad_tiny.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from SinGAN.models import WDiscriminator
    from mdfloss import MDFLoss
    torch.manual_seed(0)
    rng = np.random.default_rng(11)                  # the draw of tools/make_mdf_golden.py
    target = np.tanh(rng.standard_normal((1, 3, 64, 64))).astype(np.float32)
    cands = np.clip(target + 0.3 * rng.standard_normal((3, 3, 64, 64)), -1, 1).astype(np.float32)
    out = {"inputs_digest": np.array(hashlib.sha256(target.tobytes() + cands.tobytes()).hexdigest())}
    for name, seed, nfc, scales, asc in CASES:
        Ds = []
        for sd in random_discriminators(seed, nfc):
            N = sd["head.conv.weight"].shape[0]
            opt = types.SimpleNamespace(nfc=N, min_nfc=N, nc_im=3, ker_size=3, padd_size=0, num_layer=5)
            D = WDiscriminator(opt)
            D.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
            for p in D.parameters():
                p.requires_grad_(False)
            Ds.append(D.eval())
        crit = MDFLoss.__new__(MDFLoss)
        torch.nn.Module.__init__(crit)
        crit.Ds, crit.num_discs = Ds, len(Ds)
        x = torch.from_numpy(target).expand(3, -1, -1, -1)
        y = torch.from_numpy(cands.copy()).requires_grad_()
        loss = crit(x, y, num_scales=scales, is_ascending=asc)
        loss.backward()
        out[f"{name}_grad"] = y.grad.numpy().astype(np.float32)
        out[f"{name}_mean"] = np.float32(float(loss.detach()))
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
