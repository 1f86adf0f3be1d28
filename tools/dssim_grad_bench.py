"""Cost of the DSSIM pixel term in gradient mode at 1024^2, one target, LPIPS(squeeze) + pixel term, hipGraph replay:
    python tools/dssim_grad_bench.py [--steps 60] [--reps 3]      -> alternates pixel_term="mse" and "dssim", `reps` times each, one JSON line per
                                                                    run and a summary line; then the fused kernel alone (hip events)
    python tools/dssim_grad_bench.py --kernel-only                -> the kernel loop alone (for `rocprofv3 --kernel-trace --stats -- python ...`)"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import build                                                                  # noqa: E402
from morphganformer_amd import _lib                                                     # noqa: E402
from morphganformer_amd.lpips import PerceptualLoss                                     # noqa: E402
from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs     # noqa: E402
from morphganformer_amd.synth_weights import GeneratorConfig                            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--kernel-only", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)


def kernel_us(launches=200):
    """mgf_dssim_grad_f32 (fused kernel + finish kernel) on [1, 3, 1024, 1024], microseconds per call between two events."""
    L = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(0)
    img, tgt = torch.randn(1, 3, 1024, 1024, device=dev, generator=g) * 0.5, torch.rand(3, 1024, 1024, device=dev, generator=g) * 2 - 1
    dimg, out = torch.empty_like(img), torch.empty(1, device=dev)
    scratch = torch.empty(int(L.mgf_dssim_scratch_bytes(1, 3, 1024, 1024)) // 8, dtype=torch.float64, device=dev)
    call = lambda: _lib.check(L.mgf_dssim_grad_f32(dimg.data_ptr(), out.data_ptr(), img.data_ptr(), tgt.data_ptr(), 1, 3, 1024, 1024, 0, 255.0, 1.0,
                                                   0, 0, scratch.data_ptr(), _lib.stream_ptr()), "dssim_grad")
    for _ in range(10):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


if a.kernel_only:
    print(json.dumps({"dssim_grad_call_us": round(kernel_us(), 2)}), flush=True)
    sys.exit(0)

cfg = GeneratorConfig(img_resolution=1024)
sd, G, percept, eng, target, latent_mean, latent_std, lms = build(cfg, dev, 0, 64, False, 1)
del eng, percept
total = (a.reps + 1) * a.steps + 8
rates = {"mse": [], "dssim": []}
engines = {term: GradientProjectionEngine(G, target, latent_mean, latent_std, ProjectionArgs(step=total, pixel_term=term),
                                          percept=PerceptualLoss(net="squeeze", device=dev, allow_random_backbone=True), use_mse=True,
                                          noise_mode="random", seed=5, use_graph=True) for term in rates}
for e in engines.values():
    e.run(4)
torch.cuda.synchronize()
for rep in range(a.reps):
    for term, e in engines.items():
        t0 = time.perf_counter()
        e.run(a.steps)
        torch.cuda.synchronize()
        rates[term].append(a.steps / (time.perf_counter() - t0))
        print(json.dumps({"pixel_term": term, "rep": rep, "iters_per_s": round(rates[term][-1], 2)}), flush=True)
mean = {k: sum(v) / len(v) for k, v in rates.items()}
print(json.dumps({"summary": "gradient mode 1024^2, one target, LPIPS(squeeze) + pixel term", "mse_iters_per_s": round(mean["mse"], 2),
                  "dssim_iters_per_s": round(mean["dssim"], 2), "dssim_over_mse": round(mean["dssim"] / mean["mse"], 4),
                  "dssim_grad_call_us": round(kernel_us(), 2)}), flush=True)
