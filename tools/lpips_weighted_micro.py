"""Region-weighted LPIPS tap kernels against the un-weighted entry points on the SqueezeNet tap shapes at 1024^2 (GPU), alternated on the
same buffers:   python tools/lpips_weighted_micro.py [n] [repeats] [--json FILE]

Forward: mgf_lpips_layer_defer_f32 vs mgf_lpips_layer_defer_weighted_f32 (both with stats, as gradient mode calls them).
Backward: mgf_lpips_layer_bwd_relu_stats_f32 vs mgf_lpips_layer_bwd_relu_stats_weighted_f32 (reading the forward's stats).
A weighted kernel reads one more float per pixel beside the 2 c floats of the two taps: 1 / (2 c) more bytes.  Per shape the script prints
the medians, the un-weighted repeats' spread ((max - min) / median) and the weighted / un-weighted ratio next to the margin 1 + 1 / (2 c) + spread."""
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from morphganformer_amd import _lib  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(argv[0]) if argv else 32
repeats = int(argv[1]) if len(argv) > 1 else 7
json_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
L, st = _lib.lib(), _lib.stream_ptr()
red = int(L.mgf_reduce_scratch_floats())
scratch = torch.empty(n * red, device="cuda")
INNER = 20


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / INNER * 1e3


rows = []
for c, side in ((128, 255), (256, 127), (384, 63), (512, 63)):
    hw = side * side
    torch.manual_seed(c)
    a = torch.relu(torch.randn(n, c, hw, device="cuda"))
    b = torch.nn.functional.normalize(torch.rand(1, c, hw, device="cuda"), dim=1)
    lin = torch.rand(c, device="cuda")
    w = torch.rand(1, hw, device="cuda")
    w /= w.sum()
    stats = torch.empty(n, 3, hw, device="cuda")
    dz, dy = torch.empty_like(a), torch.randn_like(a)
    got = C.c_int32(0)
    P = lambda t: t.data_ptr()
    fns = {
        ("fwd", "plain"): lambda: _lib.check(L.mgf_lpips_layer_defer_f32(P(scratch), P(stats), P(a), P(b), P(lin), n, c, hw, 0, C.byref(got), st)),
        ("fwd", "weighted"): lambda: _lib.check(L.mgf_lpips_layer_defer_weighted_f32(P(scratch), P(stats), P(a), P(b), P(lin), P(w), n, c, hw, 0, 0,
                                                                                    C.byref(got), st)),
        ("bwd", "plain"): lambda: _lib.check(L.mgf_lpips_layer_bwd_relu_stats_f32(P(dz), None, P(dy), P(a), P(b), P(lin), P(stats), n, c, c, hw, 0, 1.0,
                                                                                 st)),
        ("bwd", "weighted"): lambda: _lib.check(L.mgf_lpips_layer_bwd_relu_stats_weighted_f32(P(dz), None, P(dy), P(a), P(b), P(lin), P(stats), P(w), n, c,
                                                                                             c, hw, 0, 0, 1.0, st)),
    }
    for f in fns.values():          # warm up every kernel of the timed window
        f()
        f()
    torch.cuda.synchronize()
    for direction in ("fwd", "bwd"):
        t = {"plain": [], "weighted": []}
        for _ in range(repeats):    # alternated: plain, weighted, plain, weighted ...
            for kind in ("plain", "weighted"):
                t[kind].append(timed(fns[(direction, kind)]))
        mp, mw = statistics.median(t["plain"]), statistics.median(t["weighted"])
        spread = (max(t["plain"]) - min(t["plain"])) / mp
        margin = 1.0 + 1.0 / (2 * c) + spread
        row = dict(direction=direction, n=n, c=c, side=side, plain_us=mp, weighted_us=mw, ratio=mw / mp, plain_spread=spread, extra_bytes=1.0 / (2 * c),
                   margin=margin, within=mw / mp <= margin, plain_all=t["plain"], weighted_all=t["weighted"])
        rows.append(row)
        print(f"{direction} c {c:3d} {side}x{side} n {n}: plain {mp:7.1f} us  weighted {mw:7.1f} us  ratio {mw / mp:.4f}  "
              f"margin {margin:.4f} (bytes +{1.0 / (2 * c):.4f}, plain spread {spread:.4f})  {'ok' if row['within'] else 'OVER'}", flush=True)
if json_path:
    with open(json_path, "w") as f:
        json.dump(rows, f, indent=1)
