"""Throughput of the MDF literal loop (1024_example_mdfloss.py / projection_example_v1_mdfloss.py): ProjectionEngine(mdf=MDFLoss) on
seeded synthetic generator and discriminator weights, no LPIPS / MSE term, min_loss 1000, graph replay, injected noise.

    python tools/mdf_bench.py [--res 1024] [--batch 16 32] [--steps 96] [--reps 3] [--pool-above 0] [--out FILE]
    python tools/mdf_bench.py --gradient [--res 1024] [--steps 64] [--reps 3] [--out FILE]

Prints one JSON line per configuration: iterations/s (median of --reps runs, one warm-up sequence each), and the body launches'
executed fraction of the FP32 matrix peak (Winograd F(2x2,3x3) executes 4/9 of the direct form's multiplies; peak 157.3 TFLOP/s),
from the library's own per-launch profile (mgf_conv_profile_begin/end) of one launch sequence.  MGF_MDF_BODY=taps puts the body
layers on the direct tap-list kernel instead (the A/B reference).  --profile-one runs a single launch sequence (for a
`rocprofv3 --kernel-trace --stats` capture around this script).

--gradient: the gradient-mode leg instead -- GradientProjectionEngine(mdf=MDFLoss(differentiable=True)) at one target, MDF alone, the 8
random_discriminators, graph replay: iterations/s, and each MDF launch of one forward + backward call in the library's per-launch
profile (the body adjoints next to the forward body launch of the same layer; the tail and head backward against their HBM bound).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MATRIX_PEAK = 157.3e12


def build(res, batch, steps, pool_above):
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine
    from morphganformer_amd.synth_weights import FULL1024, SMALL256, make_state_dict, synthetic_latents
    cfg = FULL1024 if res == 1024 else SMALL256
    G = Generator(make_state_dict(cfg, seed=0), cfg, "cuda", max_batch=1)
    tgt = G(torch.from_numpy(synthetic_latents(cfg, 1, 1000)).cuda(), None, noise_mode="const")[0].clamp(-1, 1).clone()
    if pool_above and res > pool_above:
        f = res // pool_above
        tgt = tgt.reshape(1, 3, pool_above, f, pool_above, f).mean(dim=(3, 5)).contiguous()
    rng = np.random.default_rng(0)
    eps = torch.from_numpy(rng.standard_normal((steps, 1, cfg.k, cfg.z_dim)).astype(np.float32)).cuda()
    args = ProjectionArgs(step=steps, min_loss_init=1000.0, pool_above=pool_above)
    return ProjectionEngine(G, tgt, torch.zeros(cfg.k, cfg.z_dim, device="cuda"), 1.0, args, percept=None, use_mse=False, eps=eps,
                            noise_mode="const", batch=batch, mdf=MDFLoss(random_discriminators(0)))


def body_fraction(crit, batch, res):
    """Executed fraction of the FP32 matrix peak over the body launches of one MDFLoss call on `batch` candidates (the library's
    per-launch profile: HIP events around each launch, eager)."""
    from morphganformer_amd import conv as cv
    img = torch.rand(batch, 3, res, res, device="cuda") * 2 - 1
    out = torch.zeros(batch, device="cuda")
    crit.distance_into(out, img)
    torch.cuda.synchronize()
    cv.profile_begin()
    crit.distance_into(out, img)
    torch.cuda.synchronize()
    recs = cv.profile_end()                          # (kernel, direct-form flops, seconds, ksplit, bytes)
    body = [r for r in recs if "mdf_" not in r[0]]
    if not body:
        return None
    t = sum(r[2] for r in body)
    direct = sum(r[1] for r in body)
    wino = all("wino3" in r[0] for r in body)
    executed = direct * (4.0 / 9.0 if wino else 1.0)
    return {"body_launches": len(body), "body_kernels": sorted(set(r[0] for r in body)), "body_ms": 1e3 * t,
            "body_direct_tflops": direct / t / 1e12, "body_executed_fraction_of_peak": executed / t / FP32_MATRIX_PEAK,
            "mdf_ms": 1e3 * sum(r[2] for r in recs)}


def build_gradient(res, steps):
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    from morphganformer_amd.synth_weights import FULL1024, SMALL256, make_state_dict, synthetic_latents
    cfg = FULL1024 if res == 1024 else SMALL256
    G = Generator(make_state_dict(cfg, seed=0), cfg, "cuda", max_batch=1)
    tgt = G(torch.from_numpy(synthetic_latents(cfg, 1, 1000)).cuda(), None, noise_mode="const")[0].clamp(-1, 1).clone()
    rng = np.random.default_rng(0)
    eps = torch.from_numpy(rng.standard_normal((steps, 1, cfg.k, cfg.z_dim)).astype(np.float32)).cuda()
    args = ProjectionArgs(step=steps, min_loss_init=1000.0)
    return GradientProjectionEngine(G, tgt, torch.zeros(cfg.k, cfg.z_dim, device="cuda"), 1.0, args, percept=None, use_mse=False, eps=eps,
                                    noise_mode="const", mdf=MDFLoss(random_discriminators(0), differentiable=True))


def gradient_launches(crit, res, hbm_tbs=8.0):
    """Per-launch profile of one forward + backward MDF call on one candidate: [(kernel, ms, fraction of the HBM bound)]."""
    from morphganformer_amd import conv as cv
    img = torch.rand(1, 3, res, res, device="cuda") * 2 - 1
    out, dimg = torch.zeros(1, device="cuda"), torch.empty_like(img)
    crit.distance_into(out, img, dimg=dimg)
    torch.cuda.synchronize()
    cv.profile_begin()
    crit.distance_into(out, img, dimg=dimg)
    torch.cuda.synchronize()
    recs = cv.profile_end()                          # (kernel, direct-form flops, seconds, ksplit, bytes)
    return [{"kernel": r[0], "ms": 1e3 * r[2], "hbm_bound_fraction": (r[4] / (hbm_tbs * 1e12)) / r[2] if r[4] else None} for r in recs]


def main_gradient(a):
    eng = build_gradient(a.res, a.steps)
    eng.run(2)                                      # capture + warm-up
    torch.cuda.synchronize()
    if a.profile_one:
        eng.run(a.steps - 2)
        torch.cuda.synchronize()
        return
    rates = []
    for _ in range(a.reps):
        eng.rewind()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run()
        torch.cuda.synchronize()
        rates.append(a.steps / (time.perf_counter() - t0))
    rec = {"leg": "gradient", "res": a.res, "targets": 1, "steps": a.steps, "discriminators": len(eng.mdf.nets),
           "iters_per_s_median": float(np.median(rates)), "iters_per_s": rates, "launches": gradient_launches(eng.mdf, a.res)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024, choices=[256, 1024])
    ap.add_argument("--batch", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--steps", type=int, default=96)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pool-above", type=int, default=0)
    ap.add_argument("--profile-one", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--gradient", action="store_true")
    a = ap.parse_args()
    if a.gradient:
        return main_gradient(a)
    lines = []
    for batch in a.batch:
        eng = build(a.res, batch, a.steps, a.pool_above)
        eng.run(batch)                              # capture + one warm-up sequence
        torch.cuda.synchronize()
        if a.profile_one:
            eng.rewind()
            eng.run(batch)
            torch.cuda.synchronize()
            continue
        rates = []
        for _ in range(a.reps):
            eng.rewind()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.run()
            torch.cuda.synchronize()
            rates.append(a.steps / (time.perf_counter() - t0))
        rec = {"res": a.res, "pool_above": a.pool_above, "batch": batch, "steps": a.steps, "body": os.environ.get("MGF_MDF_BODY", "winograd"),
               "iters_per_s_median": float(np.median(rates)), "iters_per_s": rates}
        r = a.res // (a.res // a.pool_above) if (a.pool_above and a.res > a.pool_above) else a.res
        rec.update(body_fraction(eng.mdf, batch, r) or {})
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del eng
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
