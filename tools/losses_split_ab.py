"""Bit equality of two builds over every export of csrc/losses.hip, maxpool.hip, loop_step.hip and dssim.hip, plus mgf_msssim_* and the MDF
value (their float64 block sums share mgf_block_tree_sum_256): small shapes across each kernel's seams, every output hashed
(profiles/losses_split_ab.jsonl).

    MGF_PACKAGE_ROOT=<a checkout of the parent commit, built> python tools/losses_split_ab.py --run parent --out FILE.jsonl
    python tools/losses_split_ab.py --run head --out FILE.jsonl
    python tools/losses_split_ab.py --compare FILE.jsonl          (appends a summary line; exit status 1 if any hash differs)
"""
import argparse
import contextlib
import ctypes
import json
import os
import sys

ROOT = os.environ.get("MGF_PACKAGE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

POOL_WIDTHS = [3, 63, 64, 65, 128, 129, 192, 256, 257, 320, 384, 448, 449, 512, 513, 641]
DSSIM_SIDES = [7, 16, 17, 38, 39]


def workload():
    import numpy as np
    import torch
    from morphganformer_amd import _lib
    from lpips_refactor_ab import alone, sha, spatial

    L, st, res = _lib.lib(), _lib.stream_ptr(), {}
    gen = torch.Generator().manual_seed(20)
    randn = lambda *s, dt=torch.float32: torch.randn(*s, generator=gen, dtype=dt).cuda()
    rand = lambda *s, dt=torch.float32: torch.rand(*s, generator=gen, dtype=dt).cuda()
    nans = lambda *s, dt=torch.float32: torch.full(s, float("nan"), dtype=dt, device="cuda")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    p = lambda t: 0 if t is None else t.data_ptr()

    # ---- maxpool.hip
    for h in (5, 6):
        for w in POOL_WIDTHS:
            x = torch.relu(randn(2, h, w)) - (5.0 if (h, w) == (6, 641) else 0.0)
            oh, ow = -(-(h - 3) // 2) + 1, -(-(w - 3) // 2) + 1
            oh, ow = oh - ((oh - 1) * 2 >= h), ow - ((ow - 1) * 2 >= w)
            dy, args = randn(2, oh, ow), (2, h, w, oh, ow, st)
            y, yi, taps, dx, dxi = nans(2, oh, ow), nans(2, oh, ow), torch.full((2, oh, ow), 255, dtype=torch.uint8, device="cuda"), nans(2, h, w), nans(2, h, w)
            _lib.check(L.mgf_maxpool3x3s2_ceil_f32(p(y), p(x), *args))
            _lib.check(L.mgf_maxpool3x3s2_ceil_idx_f32(p(yi), p(taps), p(x), *args))
            _lib.check(L.mgf_maxpool3x3s2_ceil_bwd_f32(p(dx), p(dy), p(x), *args))
            _lib.check(L.mgf_maxpool3x3s2_ceil_bwd_idx_f32(p(dxi), p(dy), p(taps), *args))
            res[f"pool/ceil/{h}x{w}"] = [sha(t) for t in (y, yi, taps, dx, dxi)]
            if w in (65, 257):
                for k in (2, 3):
                    fh, fw = (h - k) // 2 + 1, (w - k) // 2 + 1
                    fy, fdy, fdx = nans(2, fh, fw), randn(2, fh, fw), nans(2, h, w)
                    _lib.check(L.mgf_maxpool_s2_floor_f32(p(fy), p(x), 2, h, w, k, st))
                    _lib.check(L.mgf_maxpool_s2_floor_bwd_f32(p(fdx), p(fdy), p(x), 2, h, w, k, st))
                    res[f"pool/floor{k}/{h}x{w}"] = [sha(fy), sha(fdx)]

    # ---- dssim.hip, msssim.hip
    for h in DSSIM_SIDES:
        for w in DSSIM_SIDES:
            n, c = 2, 3
            img, tgt = rand(n, c, h, w) * 2 - 1, rand(n, c, h, w) * 2 - 1
            scratch = torch.empty(int(L.mgf_dssim_scratch_bytes(n, c, h, w)) // 8, dtype=torch.float64, device="cuda")
            out = []
            for stride in (0, c * h * w):
                u8, val, gval, dimg = torch.ones(n, device="cuda"), torch.ones(n, device="cuda"), torch.ones(n, device="cuda"), torch.ones_like(img)
                _lib.check(L.mgf_dssim_u8_f32(p(u8), p(img), p(tgt), n, c, h, w, stride, 255.0, 0.5, 1, p(scratch), st))
                _lib.check(L.mgf_dssim_f32(p(val), p(img), p(tgt), n, c, h, w, stride, 255.0, 1.0, 0, p(scratch), st))
                _lib.check(L.mgf_dssim_grad_f32(p(dimg), p(gval), p(img), p(tgt), n, c, h, w, stride, 255.0, 0.25, 1, 1, p(scratch), st))
                out += [sha(t) for t in (u8, val, gval, dimg)]
            res[f"dssim/{h}x{w}"] = out
    from morphganformer_amd.pixel_term import msssim_weights
    for (h, w, levels) in ((64, 64, 3), (38, 39, 2), (11, 17, 1)):
        n, c = 2, 3
        img, tgt = rand(n, c, h, w) * 2 - 1, rand(n, c, h, w) * 2 - 1
        wts = msssim_weights(levels)
        wbuf = (ctypes.c_double * levels)(*wts)
        scratch = torch.empty(int(L.mgf_msssim_scratch_bytes(n, c, h, w, levels)) // 8, dtype=torch.float64, device="cuda")
        val, gval, dimg = nans(n), nans(n), nans(n, c, h, w)
        _lib.check(L.mgf_msssim_f32(p(val), p(img), p(tgt), n, c, h, w, c * h * w, ctypes.addressof(wbuf), levels, 255.0, 1.0, 0, p(scratch), st))
        _lib.check(L.mgf_msssim_grad_f32(p(dimg), p(gval), p(img), p(tgt), n, c, h, w, 0, ctypes.addressof(wbuf), levels, 255.0, 0.5, 0, 0, p(scratch), st))
        res[f"msssim/{h}x{w}/{levels}"] = [sha(val), sha(gval), sha(dimg)]

    # ---- mdf.hip: the value and, with the backward built, the same value beside the gradient
    from morphganformer_amd.mdf import MDFLoss, random_discriminators
    for diff in (False, True):
        crit = MDFLoss(random_discriminators(1), num_scales=3, differentiable=diff)
        crit.set_target(rand(1, 3, 64, 64) * 2 - 1)
        cand, out = rand(3, 3, 64, 64) * 2 - 1, torch.zeros(3, device="cuda")
        dimg = torch.zeros_like(cand) if diff else None
        crit.distance_into(out, cand, dimg=dimg)
        res[f"mdf/differentiable={diff}"] = [sha(out)] + ([sha(dimg)] if diff else [])

    # ---- losses.hip: MSE family, Wing / AWing by direct calls; the LPIPS entries through PerceptualLoss
    red = int(L.mgf_reduce_scratch_floats())
    for numel, n in ((4, 3), (2052, 3), (2048 * 1024 + 2048, 2), (26001, 1), (7, 1)):
        a, b, scratch = randn(n, numel), randn(n, numel), torch.empty(n * red, device="cuda")
        out = []
        for stride in ((0, numel) if numel % 4 == 0 else (0,)):         # a target stride is a multiple of 4
            o = torch.ones(n, device="cuda")
            _lib.check(L.mgf_mse_f32(p(o), p(a), p(b), n, numel, stride, 0.25, 1, p(scratch), st))
            out.append(sha(o))
        res[f"mse/{numel}x{n}"] = out
    for hw, n in ((64, 2), (63, 2), (63, 1), (4100, 3)):
        c = 3
        a, b, wm, scratch = randn(n, c, hw), randn(n, c, hw), rand(n, hw) + 0.05, torch.empty(n * red, device="cuda")
        out = []
        for ws in (0, hw):
            o, d = torch.ones(n, device="cuda"), torch.ones(n, c, hw, device="cuda")
            _lib.check(L.mgf_mse_weighted_f32(p(o), p(a), p(b), p(wm), n, c, hw, c * hw, ws, 0.5, 1, p(scratch), st))
            _lib.check(L.mgf_mse_weighted_grad_f32(p(d), p(a), p(b), p(wm), n, c, hw, 0, ws, 0.5, 1, st))
            out += [sha(o), sha(d)]
        res[f"mse_weighted/{hw}x{n}"] = out
    for numel in (1, 63, 136, 257):
        target, step = rand(numel, dt=torch.float64) * 48 + 8, i32([1])
        pred = target[None] + rand(8, numel, dt=torch.float64) * 32 - 16
        heat_t, heat_p = rand(numel, dt=torch.float64), rand(8, numel, dt=torch.float64)
        wv, av = nans(4, dt=torch.float64), nans(4, dt=torch.float64)
        _lib.check(L.mgf_wing_loss_f64(p(wv), p(pred), p(target), 4, numel, 10.0, 2.0, p(step), 3, st))
        _lib.check(L.mgf_adaptive_wing_loss_f64(p(av), p(heat_p), p(heat_t), 4, numel, 14.0, 0.5, 1.0, 2.1, 0, -1, st))
        res[f"wing/{numel}"] = [sha(wv), sha(av)]
    null = lambda: contextlib.nullcontext()
    for name, run in [alone("squeeze", 65, 1), alone("squeeze", 65, 3), alone("vgg", 48, 3), alone("alex", 96, 1), spatial("squeeze", 2)]:
        res["lpips/" + name] = run(null)["eager"]

    # ---- loop_step.hip (the shapes of tests/test_hip_loop_step.py)
    for numel in (1, 255, 257, 544):
        steps_total, batch = 3, 5
        mean, eps, sigma = randn(numel), randn(steps_total, 18, numel), rand(steps_total) + 0.1
        out = []
        for s in (0, 2, steps_total):
            rows, rows18, rows3 = nans(batch, numel), nans(batch, numel), nans(batch, numel)
            _lib.check(L.mgf_latent_perturb(p(rows), p(mean), p(eps), p(sigma), p(i32([s])), batch, steps_total, numel, st))
            _lib.check(L.mgf_latent_perturb_mean(p(rows18), p(mean), p(eps), p(sigma), p(i32([s])), batch, steps_total, numel, 18, st))
            _lib.check(L.mgf_latent_perturb_mean(p(rows3), p(mean), p(eps), p(sigma), p(i32([s])), batch, steps_total, numel, 3, st))
            out += [sha(rows), sha(rows18), sha(rows3)]
        res[f"perturb/{numel}"] = out
    for numel, batch in ((1, 1), (1, 64), (544, 1), (544, 64), (33, 4)):
        steps_total, cap = (6 if batch == 1 else 70), 4
        state = dict(min_loss=torch.tensor([100.0], dtype=torch.float64, device="cuda"), best_latent=nans(numel), best_step=i32([-1]),
                     losses=nans(steps_total, dt=torch.float64), step=i32([0]), take=i32([-7] * batch), count=i32([0]), tsteps=i32([-9] * cap),
                     tlosses=nans(cap, dt=torch.float64))
        valid = (rand(steps_total) > 0.25).to(torch.int32)
        out = []
        for launch in range(-(-steps_total // batch) + 1):
            drift = 1.0 - 0.2 * launch
            lat, pl, wl, ml = randn(batch, numel), rand(batch) * drift, rand(batch, dt=torch.float64) * 30 * drift, rand(batch) * 0.5 * drift
            _lib.check(L.mgf_select_best(p(state["min_loss"]), p(state["best_latent"]), p(state["best_step"]), p(state["losses"]), p(lat), numel, p(pl),
                                         p(wl), p(ml), 0.01, 1.0, p(state["step"]), p(valid), batch, steps_total, p(state["take"]), p(state["count"]), cap,
                                         p(state["tsteps"]), p(state["tlosses"]), st))
            out.append([sha(t) for t in state.values()])
        res[f"select/{numel}x{batch}"] = out
    for numel in (7, 1024, 4 * (512 * 256 + 300)):
        imgs, trail = randn(5, numel), nans(4, numel)
        _lib.check(L.mgf_keep_improvements(p(trail), p(imgs), numel, p(i32([2, -1, -1, -1, 3])), 5, st))
        res[f"keep/{numel}"] = sha(trail)
    for (n, h, w) in ((1, 17, 19), (2, 16, 20), (1, 64, 64), (2, 1, 4)):
        img = randn(n, 3, h, w)
        u8, gray = torch.zeros(h, w, 3, dtype=torch.uint8, device="cuda"), torch.zeros(n, h, w, dtype=torch.uint8, device="cuda")
        scratch = torch.empty(n * int(L.mgf_reference_gray_scratch_floats()), device="cuda")
        _lib.check(L.mgf_to_uint8_hwc(p(u8), p(img), 3, h, w, st))
        _lib.check(L.mgf_reference_gray_u8(p(gray), p(img), n, h, w, p(scratch), st))
        res[f"images/{n}x{h}x{w}"] = [sha(u8), sha(gray)]
    torch.cuda.synchronize()
    return res


def compare(path):
    runs = [json.loads(line) for line in open(path) if line.strip()]
    runs = [r for r in runs if "hashes" in r]
    base, differ = runs[0], []
    for r in runs[1:]:
        differ += [f"{r['run']}: {k}" for k in sorted(set(base["hashes"]) | set(r["hashes"])) if base["hashes"].get(k) != r["hashes"].get(k)]
    line = {"summary": "hashes", "runs": [r["run"] for r in runs], "entries": len(base["hashes"]), "differ": differ}
    with open(path, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))
    return 1 if differ or len(runs) < 2 else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run")
    ap.add_argument("--out")
    ap.add_argument("--compare")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare))
    line = json.dumps({"run": a.run, "package_root": "parent" if os.environ.get("MGF_PACKAGE_ROOT") else "tree", "hashes": workload()})
    with open(a.out, "a") as f:
        f.write(line + "\n")
    print(a.run, "done:", len(json.loads(line)["hashes"]), "entries")
