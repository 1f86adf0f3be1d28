"""Recipe of tests/golden/mdf_tiny.npz: the reference's own MDFLoss (mdfloss.py) and WDiscriminator (SinGAN/models.py) on the
seeded weights of morphganformer_amd.mdf.random_discriminators, on the CPU in float32.

    python tools/make_mdf_golden.py --reference <checkout of the reference project>

The reference is imported from the given checkout at run time; nothing of it is copied.  What the file holds: a 64x64 target in
[-1, 1], three candidates, and per case (8 discriminators ascending, 5 ascending, a 9-discriminator set descending) the per
candidate, discriminator position and tap mean squared differences, the per-candidate losses and the reference's batch mean, plus a
digest of the weights so that a change of the seeded draw is noticed.
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

from morphganformer_amd.mdf import random_discriminators  # noqa: E402

CASES = [("asc8", 0, (32,) * 4 + (64,) * 4, 8, 1), ("asc5", 0, (32,) * 4 + (64,) * 4, 5, 1),
         ("desc9", 1, (32,) * 4 + (64,) * 4 + (128,), 8, 0)]


def digest(Ds):
    h = hashlib.sha256()
    for sd in Ds:
        for k in sorted(sd):
            h.update(k.encode() + np.ascontiguousarray(sd[k], dtype=np.float32).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mdf_tiny.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from SinGAN.models import WDiscriminator
    from mdfloss import MDFLoss
    torch.manual_seed(0)
    rng = np.random.default_rng(11)
    target = np.tanh(rng.standard_normal((1, 3, 64, 64))).astype(np.float32)
    cands = np.clip(target + 0.3 * rng.standard_normal((3, 3, 64, 64)), -1, 1).astype(np.float32)
    out = {"target": target, "candidates": cands}
    for name, seed, nfc, scales, asc in CASES:
        sds = random_discriminators(seed, nfc)
        Ds = []
        for sd in sds:
            N = sd["head.conv.weight"].shape[0]
            opt = types.SimpleNamespace(nfc=N, min_nfc=N, nc_im=3, ker_size=3, padd_size=0, num_layer=5)
            D = WDiscriminator(opt)
            D.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
            Ds.append(D.eval())
        crit = MDFLoss.__new__(MDFLoss)
        torch.nn.Module.__init__(crit)
        crit.Ds, crit.num_discs = Ds, len(Ds)
        x, y = torch.from_numpy(target), torch.from_numpy(cands)
        with torch.no_grad():
            taps = np.zeros((3, scales, 3), np.float32)
            for i in range(scales):
                D = Ds[i if asc else len(Ds) - 1 - i]
                px = D(x, is_loss=True)
                for j in range(3):
                    py = D(y[j:j + 1], is_loss=True)
                    for t in range(3):
                        taps[j, i, t] = float(torch.mean((px[t] - py[t]) ** 2))
            per = np.array([float(crit(x, y[j:j + 1], num_scales=scales, is_ascending=asc)) for j in range(3)], np.float32)
            mean = float(crit(x.expand(3, -1, -1, -1), y, num_scales=scales, is_ascending=asc))
        out[f"{name}_taps"], out[f"{name}_loss"], out[f"{name}_mean"] = taps, per, np.float32(mean)
        out[f"{name}_digest"] = np.array(digest(sds))
        out[f"{name}_cfg"] = np.array([seed, len(nfc), scales, asc], np.int64)
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
