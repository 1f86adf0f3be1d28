"""Cost of the aligned face crop of the ArcFace biometric term (csrc/face_crop.hip) at the size the drivers run: one 1024^2 image, the typical face
(scale 7.3, 4 degrees: S = 8, 64 bilinear samples per crop pixel).

    python tools/face_crop_bench.py [--res 1024] [--scale 7.3] [--iters 200] [--reps 5] [--embedder iresnet50] [--out FILE]

Prints (and with --out writes) one JSON object:
  kernels   mgf_face_crop_f32 + mgf_face_crop_bwd_f32 (accumulating) next to the pair they replace, mgf_resize_bilinear_f32 +
            mgf_resize_bilinear_bwd_f32 (the scatter alone, as in the accumulating case), in the same process, alternating blocks of --iters launches between
            device events; median microseconds per call over --reps blocks, and the spread.  The resize kernels run 4-6 us a call: back-to-back launches
            that short may be bounded by the host's launch rate, so read their figures as upper bounds.
  floor     the traffic each crop kernel cannot avoid -- forward: the source read once (12.6 MB at 1024^2); adjoint: the image gradient read, modified
            and written (25.2 MB) -- over the measured time: achieved bytes/s of that floor.
  step      one gradient-mode step of the embedder's term (BiometricLoss.distance_into + grad_into on seeded weights) with and without a crop:
            the pair's share of the embedder's own forward + backward."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    """Microseconds per call of `fn` over `iters` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def alternate(fns, iters, reps):
    """{name: [us per call] * reps}: the candidates take turns, block after block (other work shares the machine)."""
    for fn in fns.values():                      # warm-up: code objects, caches
        timed(fn, max(10, iters // 10))
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(timed(fn, iters))
    return out


def summary(samples):
    return {"us_median": float(np.median(samples)), "us_min": float(min(samples)), "us_max": float(max(samples))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=7.3)
    ap.add_argument("--degrees", type=float, default=4.0)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--embedder", default="iresnet50")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from morphganformer_amd import _lib
    from morphganformer_amd.biometric import BiometricLoss
    L, st, r = _lib.lib(), _lib.stream_ptr(), a.res
    c, s = a.scale * math.cos(math.radians(a.degrees)), a.scale * math.sin(math.radians(a.degrees))
    M = np.array([[c, -s, 0.127 * r], [s, c, 0.059 * r]], dtype=np.float64)
    mats = torch.from_numpy(M[None]).cuda()
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(1, 3, r, r, device="cuda", generator=gen) * 2 - 1
    y, dy, dx = torch.empty(1, 3, 112, 112, device="cuda"), torch.randn(1, 3, 112, 112, device="cuda", generator=gen), torch.zeros_like(x)

    def crop_fwd():
        _lib.check(L.mgf_face_crop_f32(y.data_ptr(), x.data_ptr(), mats.data_ptr(), 1, r, r, 112, 1, 0, st), "face_crop")

    def crop_bwd():
        _lib.check(L.mgf_face_crop_bwd_f32(dx.data_ptr(), dy.data_ptr(), mats.data_ptr(), 1, r, r, 112, 1, 0, 1, st), "face_crop_bwd")

    def resize_fwd():
        _lib.check(L.mgf_resize_bilinear_f32(y.data_ptr(), x.data_ptr(), 3, r, r, 112, 112, st), "resize_bilinear")

    def resize_bwd():                            # what ArcFaceEmbedder._image_grad runs when it accumulates: the scatter alone
        _lib.check(L.mgf_resize_bilinear_bwd_f32(dx.data_ptr(), dy.data_ptr(), 3, r, r, 112, 112, st), "resize_bilinear_bwd")

    t = alternate({"face_crop": crop_fwd, "face_crop_bwd": crop_bwd, "resize_bilinear": resize_fwd, "resize_bilinear_bwd": resize_bwd}, a.iters, a.reps)
    kernels = {k: summary(v) for k, v in t.items()}
    src_bytes = 3 * r * r * 4
    floor = {"face_crop": {"bytes": src_bytes, "achieved_tb_per_s": src_bytes / (kernels["face_crop"]["us_median"] * 1e-6) / 1e12},
             "face_crop_bwd": {"bytes": 2 * src_bytes, "achieved_tb_per_s": 2 * src_bytes / (kernels["face_crop_bwd"]["us_median"] * 1e-6) / 1e12}}

    bio = BiometricLoss(a.embedder, n=1)
    bio.embedder.keep_activations = True
    out, dimg = torch.zeros(1, device="cuda"), torch.zeros_like(x)

    def step():
        bio.distance_into(out, x)
        bio.grad_into(dimg, accumulate=True)

    steps = {}
    for name, crop in (("resize", None), ("crop", M), ("resize_again", None)):
        bio.set_crop(crop)
        bio.set_target(x)
        step_iters = max(10, a.iters // 10)
        timed(step, 5)
        steps[name] = summary([timed(step, step_iters) for _ in range(a.reps)])
    pair = kernels["face_crop"]["us_median"] + kernels["face_crop_bwd"]["us_median"]
    old = kernels["resize_bilinear"]["us_median"] + kernels["resize_bilinear_bwd"]["us_median"]
    rec = {"res": r, "scale": a.scale, "degrees": a.degrees, "subsamples": int(min(max(math.ceil(a.scale), 1), 16)), "iters": a.iters, "reps": a.reps,
           "kernels": kernels, "crop_pair_us": pair, "resize_pair_us": old, "traffic_floor": floor, "embedder": a.embedder, "term_step": steps,
           "crop_pair_share_of_term_step": pair / steps["crop"]["us_median"]}
    line = json.dumps(rec, indent=1)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
