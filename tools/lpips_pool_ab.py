"""What PerceptualLoss(pool_above=N) is worth at 1024^2, LPIPS + Wing + MSE, hipGraph replay, on one box:
    python tools/lpips_pool_ab.py [--pool-above 256] [--nets squeeze,vgg] [--reps 3] [--run head] [--out profiles/lpips_pool_ab.jsonl]
        -> per backbone the literal loop (32 candidates, pipelined) and one-target gradient mode, alternating pool_above = 0 and
           pool_above = N `reps` times each; one JSON line per timed window and a summary line per loop; then the two entry points of
           csrc/block_pool.hip alone between hip events.  Every line is printed and appended to --out.
    MGF_PACKAGE_ROOT=<a checkout of the parent commit> python tools/lpips_pool_ab.py --run parent ...
        -> the same windows on a tree without the option (pool_above = 0 only): the A/B that pool_above = 0 costs nothing.
    python tools/lpips_pool_ab.py --kernel-only
        -> the entry-point loops alone (for `rocprofv3 --kernel-trace --stats -- python ...`)
Bytes of the kernels are computed from the shapes: the forward reads planes h w floats and writes 1 / f^2 of that; the adjoint with
accumulate reads and writes dx and reads dy."""
import argparse
import inspect
import json
import os
import sys
import time

import torch

ROOT = os.environ.get("MGF_PACKAGE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import build                                                                  # noqa: E402
from morphganformer_amd import _lib                                                     # noqa: E402
from morphganformer_amd.lpips import PerceptualLoss                                     # noqa: E402
from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, ProjectionEngine     # noqa: E402
from morphganformer_amd.synth_weights import GeneratorConfig                            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pool-above", type=int, default=256)
ap.add_argument("--nets", default="squeeze,vgg")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--batch", type=int, default=32, help="candidates of the literal loop")
ap.add_argument("--literal-steps", type=int, default=640, help="loop steps per timed window of the literal loop")
ap.add_argument("--gradient-steps", type=int, default=40, help="loop steps per timed window of gradient mode")
ap.add_argument("--res", type=int, default=1024)
ap.add_argument("--run", default="head", help="the run's name in every line (parent, head)")
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lpips_pool_ab.jsonl"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
HAS_OPTION = "pool_above" in inspect.signature(PerceptualLoss.__init__).parameters
SETTINGS = [0, a.pool_above] if HAS_OPTION else [0]


def emit(rec):
    line = json.dumps({"run": a.run, **rec})
    print(line, flush=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


def time_calls(call, launches=200):
    for _ in range(10):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def kernels():
    """mgf_block_mean_f32 on 32 images and mgf_block_mean_adjoint_f32 (accumulate, as grad_into calls it) on one, f = res // pool_above:
    microseconds per call between hip events (launch gaps included: the kernels' own time is the kernel trace's)."""
    L, st = _lib.lib(), _lib.stream_ptr()
    r, f = a.res, a.res // a.pool_above
    x = torch.randn(a.batch, 3, r, r, device=dev)
    out = torch.empty(a.batch, 3, r // f, r // f, device=dev)
    dimg = torch.zeros(1, 3, r, r, device=dev)
    g = torch.randn(1, 3, r // f, r // f, device=dev)[:, :, :r // f - 1, :r // f - 1]       # a view that stops short, like the backbone's
    fwd = lambda: _lib.check(L.mgf_block_mean_f32(out.data_ptr(), x.data_ptr(), a.batch * 3, r, r, f, st), "block_mean")
    adj = lambda: _lib.check(L.mgf_block_mean_adjoint_f32(dimg.data_ptr(), g.data_ptr(), 3, r, r, f, g.shape[2], g.shape[3], g.stride(2), g.stride(1),
                                                          1, st), "block_mean_adjoint")
    fwd_bytes = 4 * a.batch * 3 * r * r * (1 + 1 / (f * f))
    adj_bytes = 4 * 3 * (2 * r * r + g.shape[2] * g.shape[3])
    fwd_us, adj_us = time_calls(fwd), time_calls(adj)
    return {"kernels": f"{r}x{r}, f = {f}", "block_mean_images": a.batch, "block_mean_bytes": int(fwd_bytes), "block_mean_call_us": round(fwd_us, 2),
            "block_mean_call_TB_per_s": round(fwd_bytes / fwd_us * 1e-6, 3), "adjoint_images": 1, "adjoint_bytes": int(adj_bytes),
            "adjoint_call_us": round(adj_us, 2), "adjoint_call_TB_per_s": round(adj_bytes / adj_us * 1e-6, 3)}


def percept(net, pool_above):
    kw = {"pool_above": pool_above} if HAS_OPTION else {}
    return PerceptualLoss(net=net, device=dev, allow_random_backbone=True, **kw)


def alternate(name, net, engines, steps):
    """Timed windows of `steps` loop steps, the settings in turn, `reps` times; every window ends in a device synchronise."""
    rates = {k: [] for k in engines}
    for e in engines.values():
        e.run(steps // 4)                                  # graph capture and first replays, untimed
    torch.cuda.synchronize()
    for rep in range(a.reps):
        for k, e in engines.items():
            t0 = time.perf_counter()
            e.run(steps)
            torch.cuda.synchronize()
            rates[k].append(steps / (time.perf_counter() - t0))
            emit({"loop": name, "net": net, "pool_above": k, "rep": rep, "window_steps": steps, "iters_per_s": round(rates[k][-1], 2)})
    rec = {"summary": name, "net": net, "res": a.res, "window_steps": steps, "reps": a.reps}
    for k, v in rates.items():
        rec[f"pool_above_{k}_iters_per_s"] = round(sum(v) / len(v), 2)
        rec[f"pool_above_{k}_spread"] = round((max(v) - min(v)) / (sum(v) / len(v)), 4)
    if len(rates) == 2:
        lo, hi = (sum(rates[k]) / len(rates[k]) for k in SETTINGS)
        rec["speedup"] = round(hi / lo, 3)
    emit(rec)


if a.kernel_only:
    if not HAS_OPTION:
        raise SystemExit("lpips_pool_ab: this tree has no block-mean kernels")
    emit(kernels())
    sys.exit(0)

cfg = GeneratorConfig(img_resolution=a.res)
lit_total = (a.reps + 1) * a.literal_steps + 2 * a.batch
grad_total = (a.reps + 1) * a.gradient_steps + 8
sd, G, p0, e0, target, latent_mean, latent_std, (lm_t, lm_s) = build(cfg, dev, 0, max(lit_total, grad_total), False, 1)
del e0, p0
for net in a.nets.split(","):
    lit = {k: ProjectionEngine(G, target, latent_mean, latent_std, ProjectionArgs(step=lit_total), percept=percept(net, k), use_mse=True, lm_target=lm_t,
                               lm_steps=lm_s, noise_mode="random", seed=100, use_graph=True, batch=a.batch, pipeline=True) for k in SETTINGS}
    alternate(f"literal, {a.batch} candidates, LPIPS + Wing + MSE", net, lit, a.literal_steps)
    del lit
    torch.cuda.empty_cache()
    grad = {k: GradientProjectionEngine(G, target, latent_mean, latent_std, ProjectionArgs(step=grad_total), percept=percept(net, k), use_mse=True,
                                        lm_target=lm_t, lm_steps=lm_s, noise_mode="random", seed=5, use_graph=True) for k in SETTINGS}
    alternate("gradient, one target, LPIPS + Wing + MSE", net, grad, a.gradient_steps)
    del grad
    torch.cuda.empty_cache()
if HAS_OPTION:
    emit(kernels())
