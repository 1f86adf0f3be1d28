"""Cost of noise-map optimisation in gradient mode at 1024^2, one target, LPIPS(squeeze) + MSE, hipGraph replay:
    python tools/noise_opt_bench.py [--steps 60] [--reps 3] [--out profiles/noise_opt_bench.jsonl]
    python tools/noise_opt_bench.py --lockstep 8 [--out profiles/noise_sets_bench.jsonl]      (+ the lockstep leg, see the end)
alternates optimize_noise off and on, `reps` times each on one device (one JSON line per run), then times the added launches by group
between two events -- the channel sums of all noise layers (mgf_noise_grad_f32), the regulariser over all maps (one set call), keep + Adam +
normalisation (one set call each) -- and ends with a summary line.  The on-engine also runs its backward pass without the fused style / activation / blur-gradient pass (the noise
layers' pre-activation gradient has to reach memory): that difference is part of the step-time figure, not of the three groups.

--lockstep B adds, alternated on the same device, `reps` times each: (i) B lockstep targets without noise optimisation, (ii) B lockstep
targets with maps of their own (noise_per_target=True), (iii) the one-target optimize_noise engine run B times in a row; per-target rates of
all three, the step-time difference (ii) - (i), the kernel nodes of the captured graphs of (i) and (ii), and the set calls timed by group."""
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
ap.add_argument("--out", default=None)
ap.add_argument("--lockstep", type=int, default=0, help="also measure B lockstep targets with and without per-target noise maps")
a = ap.parse_args()
dev = torch.device("cuda", 0)
lines = []


def emit(rec):
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)


def timed_us(fn, reps=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


cfg = GeneratorConfig(img_resolution=1024)
sd, G, percept, eng, target, latent_mean, latent_std, lms = build(cfg, dev, 0, 64, False, 1)
del eng, percept
total = (a.reps + 1) * a.steps * max(1, a.lockstep + 1) + 8
rates = {False: [], True: []}
engines = {on: GradientProjectionEngine(G, target, latent_mean, latent_std, ProjectionArgs(step=total),
                                        percept=PerceptualLoss(net="squeeze", device=dev, allow_random_backbone=True), use_mse=True,
                                        noise_mode="random", seed=5, use_graph=True, optimize_noise=on) for on in rates}
for e in engines.values():
    e.run(4)
torch.cuda.synchronize()
for rep in range(a.reps):
    for on, e in engines.items():
        t0 = time.perf_counter()
        e.run(a.steps)
        torch.cuda.synchronize()
        rates[on].append(a.steps / (time.perf_counter() - t0))
        emit({"optimize_noise": on, "rep": rep, "iters_per_s": round(rates[on][-1], 2)})

# the added launches by group, eager, on the on-engine's own buffers (the loop state is not advanced: the step counter is not touched)
e = engines[True]
L = _lib.lib()
layers = [lp for lp in G.plan.layers if lp.noise_strength is not None]
dpre = torch.randn(max(lp.cout * lp.res * lp.res for lp in layers), device=dev)


def channel_sums():
    for lp in layers:
        _lib.check(L.mgf_noise_grad_f32(e.dnoises[lp.name].data_ptr(), dpre.data_ptr(), lp.noise_strength.data_ptr(), lp.cout, lp.res * lp.res, 0,
                                        _lib.stream_ptr()), "noise_grad")


keep = [t.clone() for t in e._state()] + [e.p_loss.clone(), e.noise_grad.clone()]
us = {"noise_grad_all_layers_us": timed_us(channel_sums), "regulariser_all_maps_us": timed_us(lambda: e._noise_regularize(True)),
      "adam_and_normalise_us": timed_us(e._noise_update)}
for dst, src in zip(list(e._state()) + [e.p_loss, e.noise_grad], keep):
    dst.copy_(src)
mean = {k: sum(v) / len(v) for k, v in rates.items()}
emit({"summary": "gradient mode 1024^2, one target, LPIPS(squeeze) + MSE, optimize_noise off / on", "off_iters_per_s": round(mean[False], 2),
      "on_iters_per_s": round(mean[True], 2), "on_over_off": round(mean[True] / mean[False], 4),
      "off_ms_per_step": round(1e3 / mean[False], 3), "on_ms_per_step": round(1e3 / mean[True], 3),
      "noise_floats": int(e.noise_flat.numel()), "dpre_bytes_read": int(sum(4 * lp.cout * lp.res * lp.res for lp in layers)),
      **{k: round(v, 1) for k, v in us.items()}})


def lockstep_leg(B):
    from bench import graph_kernel_nodes
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import synthetic_latents
    GB = Generator(sd, cfg, dev, max_batch=B)
    zt = torch.from_numpy(synthetic_latents(cfg, B, seed=2000)).to(dev)
    tg = torch.cat([GB(zt[j:j + 1], None, noise_mode="const")[0].clamp(-1, 1) for j in range(B)]).contiguous()
    steps_total = (a.reps + 1) * a.steps + 8
    group = {}
    for on in (False, True):
        group[on] = GradientProjectionEngine(GB, tg, latent_mean, latent_std, ProjectionArgs(step=steps_total),
                                             percept=PerceptualLoss(net="squeeze", device=dev, allow_random_backbone=True), use_mse=True,
                                             noise_mode="random", seed=6, use_graph=True, optimize_noise=on, noise_per_target=on)
        group[on].graph_debug = True                     # (only so that the launches per step can be counted afterwards)
        group[on].run(4)
    one = engines[True]
    torch.cuda.synchronize()
    legs = {"lockstep_off": (group[False], a.steps, B), "lockstep_per_target_maps": (group[True], a.steps, B), "one_target_in_a_row": (one, B * a.steps, 1)}
    per_target = {k: [] for k in legs}
    for rep in range(a.reps):
        for name, (e, steps, targets) in legs.items():
            t0 = time.perf_counter()
            e.run(steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            per_target[name].append(steps / dt)
            emit({"leg": name, "targets": targets, "rep": rep, "steps_per_s": round(steps / dt, 2), "target_iters_per_s": round(targets * steps / dt, 2)})
    e = group[True]
    keep = [t.clone() for t in e._state()] + [e.p_loss.clone(), e.noise_grad.clone()]
    dpre_b = torch.randn(B * max(lp.cout * lp.res * lp.res for lp in layers), device=dev)

    def channel_sums_sets():
        for lp in layers:
            _lib.check(L.mgf_noise_sets_grad_f32(e.dnoises[lp.name].data_ptr(), e.noise_total, dpre_b.data_ptr(), lp.noise_strength.data_ptr(), B, lp.cout,
                                                 lp.res * lp.res, 0, _lib.stream_ptr()), "noise_sets_grad")

    us = {"noise_sets_grad_all_layers_us": timed_us(channel_sums_sets), "pack_us": timed_us(e._noise_pack),
          "regulariser_sets_us": timed_us(lambda: e._noise_regularize(True)), "keep_adam_and_normalise_sets_us": timed_us(e._noise_update)}
    for dst, src in zip(list(e._state()) + [e.p_loss, e.noise_grad], keep):
        dst.copy_(src)
    m = {k: sum(v) / len(v) for k, v in per_target.items()}
    off, on, single = m["lockstep_off"] * B, m["lockstep_per_target_maps"] * B, m["one_target_in_a_row"]
    emit({"summary": f"gradient mode 1024^2, LPIPS(squeeze) + MSE, {B} lockstep targets: no noise optimisation / per-target maps / the one-target "
                     "optimize_noise engine, target after target", "targets": B,
          "lockstep_off_target_iters_per_s": round(off, 2), "lockstep_maps_target_iters_per_s": round(on, 2),
          "one_target_engine_iters_per_s": round(single, 2), "lockstep_maps_over_one_target_engine": round(on / single, 3),
          "lockstep_off_ms_per_step": round(1e3 / m["lockstep_off"], 3), "lockstep_maps_ms_per_step": round(1e3 / m["lockstep_per_target_maps"], 3),
          "maps_minus_off_ms_per_step": round(1e3 / m["lockstep_per_target_maps"] - 1e3 / m["lockstep_off"], 3),
          "graph_kernel_nodes_off": graph_kernel_nodes(group[False].graph), "graph_kernel_nodes_maps": graph_kernel_nodes(group[True].graph),
          "hbm_gib_peak": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 1), **{k: round(v, 1) for k, v in us.items()}})


if a.lockstep > 1:
    lockstep_leg(a.lockstep)
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
