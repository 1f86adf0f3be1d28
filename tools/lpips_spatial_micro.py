"""Spatial LPIPS maps at 1024^2 (GPU): python tools/lpips_spatial_micro.py [--out FILE] [--size 1024] [--batches 1,8]

Per batch size, LPIPS(squeeze, seeded random backbone): device-event times of
  (a) distance_into                    the scalar distance, fused stem
  (b) distance_into(keep_taps=True)    the scalar distance on the un-fused path -- the path spatial mode rides on
  (c) distance_map_into                the [n,1,H,H] map
and of the two kernels under (c) on (c)'s own operands: the seven mgf_lpips_layer_map_f32 launches and the one mgf_lpips_upsample_sum_f32 launch,
the latter with its achieved store bandwidth (n H^2 floats written; the tap maps it reads are 9 % of that and stay in L2) beside the 5.0 TB/s a copy
reaches on this chip.  Every figure: the median of `--repeats` windows of `--iters` calls after a warm-up, with the windows' min and max."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from morphganformer_amd import _lib  # noqa: E402
from morphganformer_amd.lpips import PerceptualLoss  # noqa: E402

COPY_TBS = 5.0


def timed(fn, iters, repeats, warmup=3):
    """us per call: (median, min, max) over `repeats` event-timed windows of `iters` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / iters * 1e3)
    return statistics.median(us), min(us), max(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_spatial_micro: no GPU (this tool measures; it has no CPU mode)")
    H = a.size
    lines = [f"spatial LPIPS(squeeze) at {H}x{H}: us per call, median [min .. max] of {a.repeats} windows of {a.iters} calls ({torch.cuda.get_device_name(0)})"]
    P = PerceptualLoss(model="net-lin", net="squeeze", spatial=True, use_gpu=True, allow_random_backbone=True)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    target = torch.rand(1, 3, H, H, device="cuda", generator=gen) * 2 - 1
    P.set_target(target)
    L, st = _lib.lib(), _lib.stream_ptr()
    for n in [int(v) for v in a.batches.split(",")]:
        pred = torch.rand(n, 3, H, H, device="cuda", generator=gen) * 2 - 1
        val, out = torch.empty(n, device="cuda"), torch.empty(n, 1, H, H, device="cuda")
        rows = [("(a) distance_into, fused stem", lambda: P.distance_into(val, pred)),
                ("(b) distance_into(keep_taps=True)", lambda: P.distance_into(val, pred, keep_taps=True)),
                ("(c) distance_map_into", lambda: P.distance_map_into(out, pred))]
        res = {}
        for name, fn in rows:
            res[name[:3]] = timed(fn, a.iters, a.repeats)
            lines.append("n {:2d}  {:36s} {:9.1f} [{:9.1f} .. {:9.1f}]".format(n, name, *res[name[:3]]))
        # the two kernels alone, on the operands (c) just left in the workspace
        f = P._features(n, H, H)
        taps = [f.buf[idx] for idx in (1, 4, 7, 9, 10, 11, 12)]
        maps = P._map_ws[(n, H)]

        def layer_maps():
            for t, b, lin, m in zip(taps, P._map_taps, P.lins, maps):
                _, c, hh, ww = t.shape
                _lib.check(L.mgf_lpips_layer_map_f32(m.data_ptr(), t.data_ptr(), b.data_ptr(), lin.data_ptr(), n, c, hh * ww, 0, st), "lpips_layer_map")

        km = timed(layer_maps, a.iters, a.repeats)
        ku = timed(lambda: P._upsample_sum(out, maps), a.iters, a.repeats)
        tap_bytes = 4 * sum(t.numel() for t in taps) + 4 * sum(b.numel() for b in P._map_taps)
        lines.append("n {:2d}  {:36s} {:9.1f} [{:9.1f} .. {:9.1f}]  {:.2f} TB/s over the taps read ({:.1f} MB)".format(
            n, "    7 x mgf_lpips_layer_map_f32", *km, tap_bytes / km[0] / 1e6, tap_bytes / 1e6))
        wr = 4 * n * H * H
        lines.append("n {:2d}  {:36s} {:9.1f} [{:9.1f} .. {:9.1f}]  {:.2f} TB/s stored ({:.1f} MB; a copy reaches {:.1f} TB/s = {:.1f} us); maps read: {:.2f} MB".format(
            n, "    1 x mgf_lpips_upsample_sum_f32", *ku, wr / ku[0] / 1e6, wr / 1e6, COPY_TBS, wr / COPY_TBS / 1e6, 4 * sum(m.numel() for m in maps) / 1e6))
        lines.append("n {:2d}  (c) - (b) = {:.1f} us; writing n H^2 floats at the copy rate = {:.1f} us".format(n, res["(c)"][0] - res["(b)"][0], wr / COPY_TBS / 1e6))
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
