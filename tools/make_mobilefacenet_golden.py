"""Recipe of tests/golden/mobilefacenet.npz: the reference's own MobileFaceNet (backbones/mobilefacenet.py) on the seeded weights of
morphganformer_amd.mobilefacenet.random_state(0), on the CPU.

    python tools/make_mobilefacenet_golden.py --reference <checkout of the reference project>

The reference is imported from the given checkout at run time; nothing of it is copied.  What the file holds: a seeded input
x [2,3,112,112] in [-1,1]; the module's float32 embedding, the mean and rms of the outputs of layers.0 .. layers.7 and conv_sep, and
d sum(embedding * v) / dx by its autograd for the stored v; the same embedding and gradient from the module in float64; the module's
own float32-against-float64 distances r_emb (max-norm over max|embedding|), r_grad_l2 (relative L2) and r_grad_max (max-norm over
max|gradient|) -- the yardstick of the float32 gates of the tests; and the state dict's names and shapes.

To stay under the size limit of a committed file the input lies on the 8-bit grid of an image (k / 127.5 - 1) and the two gradients
share their leading bits: grad64_hi = float32(grad64), grad64_lo = float32(grad64 - grad64_hi) (together 48 bits of the float64
gradient, 4e-15 relative) and grad_delta = grad - grad64_hi, exact in float32 (asserted), which deflates well.
tests/mobilefacenet_torch_ref.py:fixture_gradients puts them together again.

A PReLU kink within float32 rounding of an activation makes two precisions take different slopes: when the module's own two
precisions disagree by more than 1e-4 in the gradient on an input, the next input seed is drawn (the seed used is stored).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from morphganformer_amd.mobilefacenet import random_state  # noqa: E402

R_MAX = 1e-4


def run(net, x, v):
    """(embedding, stage outputs, d sum(embedding * v) / dx) of the module in x's dtype."""
    stages = []
    hooks = [m.register_forward_hook(lambda mod, i, o: stages.append(o.detach())) for m in list(net.layers) + [net.conv_sep]]
    x = x.clone().requires_grad_(True)
    emb = net(x)
    (g,) = torch.autograd.grad((emb * v).sum(), x)
    for h in hooks:
        h.remove()
    return emb.detach(), stages, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mobilefacenet.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from backbones.mobilefacenet import MobileFaceNet
    torch.manual_seed(0)
    torch.set_num_threads(1)                                     # one summation order, whatever the machine
    sd = random_state(0)
    net = MobileFaceNet(False, 512).eval()
    have = {k: tuple(t.shape) for k, t in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    assert have == {k: v.shape for k, v in sd.items()}, "random_state(0) is not the module's state dict (strict up to num_batches_tracked)"
    missing, unexpected = net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    params = sum(p.numel() for p in net.parameters())
    net64 = MobileFaceNet(False, 512).eval().double()
    net64.load_state_dict({k: torch.from_numpy(v).double() for k, v in sd.items()}, strict=False)
    v = np.random.default_rng(5).standard_normal((2, 512)).astype(np.float32)
    for seed in range(7, 32):
        x = (np.random.default_rng(seed).integers(0, 256, (2, 3, 112, 112)) / 127.5 - 1.0).astype(np.float32)
        emb, stages, g = run(net, torch.from_numpy(x), torch.from_numpy(v))
        emb64, _, g64 = run(net64, torch.from_numpy(x).double(), torch.from_numpy(v).double())
        r_emb = float((emb.double() - emb64).abs().max() / emb64.abs().max())
        r_l2 = float((g.double() - g64).norm() / g64.norm())
        r_max = float((g.double() - g64).abs().max() / g64.abs().max())
        print(f"input seed {seed}: r_emb {r_emb:.3e} r_grad_l2 {r_l2:.3e} r_grad_max {r_max:.3e}")
        assert all(np.isfinite(r) for r in (r_emb, r_l2, r_max))
        if r_emb < R_MAX and r_l2 < R_MAX and r_max < R_MAX:
            break
    else:
        raise SystemExit("no input seed on which the module's float32 and float64 gradients agree to 1e-4")
    hi = g64.numpy().astype(np.float32)
    lo = (g64.numpy() - hi.astype(np.float64)).astype(np.float32)
    delta = g.numpy() - hi
    assert np.array_equal(hi + delta, g.numpy()), "grad - float32(grad64) is not exact in float32"
    assert np.abs(hi.astype(np.float64) + lo.astype(np.float64) - g64.numpy()).max() < 1e-14 * float(g64.abs().max())
    out = {"x": x, "v": v, "input_seed": np.int64(seed), "embedding": emb.numpy(), "embedding64": emb64.numpy(),
           "grad64_hi": hi, "grad64_lo": lo, "grad_delta": delta,
           "stage_mean": np.array([float(s.double().mean()) for s in stages]),
           "stage_rms": np.array([float(s.double().square().mean().sqrt()) for s in stages]),
           "r_emb": np.float64(r_emb), "r_grad_l2": np.float64(r_l2), "r_grad_max": np.float64(r_max), "parameters": np.int64(params),
           "names": np.array(sorted(have)), "shapes": np.array([" ".join(map(str, have[k])) for k in sorted(have)])}
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes;", params, "parameters")


if __name__ == "__main__":
    main()
