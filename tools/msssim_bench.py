"""Cost of the MS-SSIM pixel term in gradient mode at 1024^2, one target, LPIPS(squeeze) + pixel term, hipGraph replay:
    python tools/msssim_bench.py [--steps 60] [--reps 3] [--out profiles/msssim_bench.jsonl]
        -> alternates pixel_term="mse", "dssim" and "msssim" on one box, `reps` times each, one JSON line per run and a summary line; then the entry
           points alone between hip events: mgf_msssim_f32 (pyramid + statistics + finish), mgf_msssim_grad_f32 (the same + the gradient pass; the
           difference is the gradient pass) and mgf_dssim_grad_f32 beside them.  Every line is printed and appended to --out.
    python tools/msssim_bench.py --kernel-only                -> the entry-point loops alone (for `rocprofv3 --kernel-trace --stats -- python ...`)"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import build                                                                  # noqa: E402
from morphganformer_amd import _lib                                                     # noqa: E402
from morphganformer_amd.lpips import PerceptualLoss                                     # noqa: E402
from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, msssim_weights     # noqa: E402
from morphganformer_amd.synth_weights import GeneratorConfig                            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--levels", type=int, default=5)
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msssim_bench.jsonl"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
out_file = open(a.out, "w")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out_file.write(line + "\n")
    out_file.flush()


def time_calls(call, launches=200):
    for _ in range(10):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        call()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / launches, 2)


def kernels_us():
    """The entry points on [1, 3, 1024, 1024] (correlated images: off the clamped branch, every level's gradient pass runs), microseconds per call."""
    L, st = _lib.lib(), _lib.stream_ptr()
    g = torch.Generator(device=dev).manual_seed(0)
    img = torch.randn(1, 3, 1024, 1024, device=dev, generator=g) * 0.5
    tgt = (img[0] + 0.2 * torch.randn(3, 1024, 1024, device=dev, generator=g)).clamp(-1, 1).contiguous()
    dimg, out = torch.empty_like(img), torch.empty(1, device=dev)
    nbytes = int(L.mgf_msssim_scratch_bytes(1, 3, 1024, 1024, a.levels))
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    dscratch = torch.empty(int(L.mgf_dssim_scratch_bytes(1, 3, 1024, 1024)) // 8, dtype=torch.float64, device=dev)
    w = msssim_weights(a.levels)
    wts = (ctypes.c_double * len(w))(*w)
    wp = ctypes.addressof(wts)
    value = lambda: _lib.check(L.mgf_msssim_f32(out.data_ptr(), img.data_ptr(), tgt.data_ptr(), 1, 3, 1024, 1024, 0, wp, a.levels, 255.0, 1.0, 0,
                                                scratch.data_ptr(), st), "msssim")
    grad = lambda: _lib.check(L.mgf_msssim_grad_f32(dimg.data_ptr(), out.data_ptr(), img.data_ptr(), tgt.data_ptr(), 1, 3, 1024, 1024, 0, wp, a.levels,
                                                    255.0, 1.0, 0, 0, scratch.data_ptr(), st), "msssim_grad")
    dssim = lambda: _lib.check(L.mgf_dssim_grad_f32(dimg.data_ptr(), out.data_ptr(), img.data_ptr(), tgt.data_ptr(), 1, 3, 1024, 1024, 0, 255.0, 1.0,
                                                    0, 0, dscratch.data_ptr(), st), "dssim_grad")
    rec = {"levels": a.levels, "msssim_scratch_bytes": nbytes, "msssim_value_call_us": time_calls(value), "msssim_grad_call_us": time_calls(grad),
           "dssim_grad_call_us": time_calls(dssim)}
    rec["msssim_gradient_pass_us"] = round(rec["msssim_grad_call_us"] - rec["msssim_value_call_us"], 2)
    rec["msssim_loss"] = round(float(out), 6)
    return rec


if a.kernel_only:
    emit(kernels_us())
    sys.exit(0)

cfg = GeneratorConfig(img_resolution=1024)
sd, G, percept, eng, target, latent_mean, latent_std, lms = build(cfg, dev, 0, 64, False, 1)
del eng, percept
total = (a.reps + 1) * a.steps + 8
rates = {"mse": [], "dssim": [], "msssim": []}
engines = {term: GradientProjectionEngine(G, target, latent_mean, latent_std, ProjectionArgs(step=total, pixel_term=term, msssim_levels=a.levels),
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
        emit({"pixel_term": term, "rep": rep, "iters_per_s": round(rates[term][-1], 2)})
mean = {k: sum(v) / len(v) for k, v in rates.items()}
step_us = {k: 1e6 / v for k, v in mean.items()}
summary = {"summary": "gradient mode 1024^2, one target, LPIPS(squeeze) + pixel term", "levels": a.levels}
summary.update({f"{k}_iters_per_s": round(v, 2) for k, v in mean.items()})
summary.update({"dssim_over_mse": round(mean["dssim"] / mean["mse"], 4), "msssim_over_mse": round(mean["msssim"] / mean["mse"], 4),
                "msssim_over_dssim": round(mean["msssim"] / mean["dssim"], 4), "dssim_step_share_us": round(step_us["dssim"] - step_us["mse"], 1),
                "msssim_step_share_us": round(step_us["msssim"] - step_us["mse"], 1)})
emit(summary)
emit(kernels_us())
