"""Timings of the MobileFaceNet embedder beside IResNet-18 / IResNet-50, one process, one MI355X, medians of three:

    python tools/mobilefacenet_bench.py [--out profiles/mobilefacenet_bench.txt] [--loop-steps 256]

  embed        embed_image of 32 candidates from 1024^2 images (the literal loop's call), ms
  fwd+bwd      embed_image + backward into a 1024^2 gradient image at ONE image (gradient mode's call), ms
  depthwise    every depthwise launch of the network at 32 candidates on its own: us and achieved bytes/s against input + output
  loop         the literal loop, Wing + embedder + LPIPS(squeeze) + MSE at 32 candidates per generator forward on the 1024^2 generator,
               iters/s, with the embedder `mobilefacenet` and `iresnet18` (the same loop: compare the latter with the parent commit's figure)

Reported, not gated: nothing in the suite depends on these numbers."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from morphganformer_amd import _lib  # noqa: E402
from morphganformer_amd.iresnet import BiometricLoss  # noqa: E402

NAMES = ("mobilefacenet", "iresnet18", "iresnet50")


def timed(fn, iters, reps=3):
    """median over `reps` of the mean milliseconds of `iters` calls (one warm-up call first)."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), out


def embedders(say):
    img32 = torch.rand(32, 3, 1024, 1024, device="cuda") * 2 - 1
    img1 = img32[:1].contiguous()
    dimg = torch.zeros_like(img1)
    demb = torch.randn(1, 512, device="cuda")
    for name in NAMES:
        e = BiometricLoss(name, n=32).embedder
        ms, runs = timed(lambda: e.embed_image(img32), 10)
        say(f"embed   32 x 1024^2  {name:14s} {ms:8.3f} ms   ({' / '.join(f'{r:.3f}' for r in runs)})")
        e1 = e.clone_for(1)

        def step():
            e1.embed_image(img1)
            e1.backward(demb, dimg)
        ms, runs = timed(step, 10)
        say(f"fwd+bwd  1 x 1024^2  {name:14s} {ms:8.3f} ms   ({' / '.join(f'{r:.3f}' for r in runs)})")


def depthwise_launches(say, n=32):
    from morphganformer_amd.mobilefacenet import block_table
    L = _lib.lib()
    shapes, res = [("layers.1", 64, 56, 3, 1, 1)], 56
    for p, cin, cout, g, stride, residual, stage in block_table():
        shapes.append((p + ".layers.1", g, res, 3, stride, 1))
        res = (res + 2 - 3) // stride + 1
    shapes.append(("features.layers.0", 512, 7, 7, 1, 0))
    seen = set()
    for name, c, r, k, s, p in shapes:
        if (c, r, k, s) in seen:
            continue
        seen.add((c, r, k, s))
        o = (r + 2 * p - k) // s + 1
        x, y = torch.randn(n, c, r, r, device="cuda"), torch.empty(n, c, o, o, device="cuda")
        w, sc, sh, sl = (torch.rand(c, k * k, device="cuda"), torch.rand(c, device="cuda"), torch.rand(c, device="cuda"),
                         torch.rand(c, device="cuda") * 0.3 + 0.1)
        dx = torch.empty_like(x)
        byt = 4.0 * (x.numel() + y.numel())
        fwd = lambda: _lib.check(L.mgf_dwconv_f32(y.data_ptr(), x.data_ptr(), w.data_ptr(), sc.data_ptr(), sh.data_ptr(), sl.data_ptr(), n, c, r, r,
                                                  k, k, s, p, _lib.stream_ptr()))
        bwd = lambda: _lib.check(L.mgf_dwconv_bwd_data_f32(dx.data_ptr(), y.data_ptr(), w.data_ptr(), sc.data_ptr(), y.data_ptr(), sl.data_ptr(),
                                                           x.data_ptr(), sl.data_ptr(), n, c, r, r, k, k, s, p, _lib.stream_ptr()))
        f, _ = timed(fwd, 50)
        b, _ = timed(bwd, 50)
        # (the masked backward also reads the two stored activations: 2 x input + 2 x output bytes)
        say(f"depthwise n={n} c={c:3d} {r:2d}^2 k{k} s{s} ({name}): forward {f * 1e3:7.1f} us {byt / f / 1e9:7.3f} TB/s of in+out;  "
            f"masked data gradient {b * 1e3:7.1f} us {byt / b / 1e9:7.3f} TB/s of in+out")


def loop(say, steps, batch=32):
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine, latent_stats, synthetic_landmarks
    from morphganformer_amd.synth_weights import FULL1024, make_state_dict, synthetic_latents
    cfg = FULL1024
    G = Generator(make_state_dict(cfg, seed=0), cfg, "cuda", max_batch=1)
    G.fuse_torgb = True
    target = G(torch.from_numpy(synthetic_latents(cfg, 1, seed=1000)).cuda(), None, noise_mode="const")[0].clamp(-1, 1).clone()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    latent_mean, latent_std = latent_stats(G, 10000, "cuda", gen)
    lm_t, lm_s = synthetic_landmarks(steps * 4, cfg.img_resolution, seed=7)
    for name in ("mobilefacenet", "iresnet18"):
        percept = PerceptualLoss(model="net-lin", net="squeeze", use_gpu=True, device="cuda", allow_random_backbone=True)
        eng = ProjectionEngine(G, target, latent_mean, latent_std, ProjectionArgs(step=steps * 4, min_loss_init=1e30), percept=percept, use_mse=True,
                               lm_target=lm_t, lm_steps=lm_s, noise_mode="random", seed=100, use_graph=True, batch=batch,
                               biometric=BiometricLoss(name, n=batch), gamma=1e-6)
        eng.run(batch * 2)
        torch.cuda.synchronize()
        rates = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.run(steps)
            b.record()
            torch.cuda.synchronize()
            rates.append(steps / (a.elapsed_time(b) * 1e-3))
        say(f"literal loop 1024^2, Wing + {name} + LPIPS(squeeze) + MSE, {batch} candidates: {statistics.median(rates):7.1f} iters/s   "
            f"({' / '.join(f'{r:.1f}' for r in rates)})")
        del eng, percept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mobilefacenet_bench.txt"))
    ap.add_argument("--loop-steps", type=int, default=256, help="timed loop steps per repetition (0 = skip the loop leg)")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/mobilefacenet_bench.py on {torch.cuda.get_device_name(0)}; medians of three (the three in brackets)")
    embedders(say)
    depthwise_launches(say)
    if a.loop_steps:
        loop(say, a.loop_steps)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
