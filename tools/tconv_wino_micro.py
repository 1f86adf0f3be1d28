"""Per-layer time of the stride-2 transposed conv: polyphase Winograd launch (csrc/wino_tconv.hip) vs the tap-list launch, border kernel
included in both, on the generator's up-sampling shapes at n samples: python tools/tconv_wino_micro.py [n] [reps]"""
import os, sys, math, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from morphganformer_amd import conv as cv
n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
cv.TCONV_WINO_MIN_WGS = 1
for cin, cout, res in ((512, 512, 16), (512, 512, 32), (512, 256, 64), (256, 128, 128), (128, 64, 256), (64, 32, 512)):
    torch.manual_seed(res)
    x = torch.randn(n, cin, res, res, device="cuda")
    wt = torch.randn(cout, cin, 3, 3, device="cuda") / math.sqrt(9 * cin)
    pc, u = cv.pack_weights(wt), cv.tconv_winograd_weights(wt)
    s, d = torch.rand(n, cin, device="cuda") + 0.5, torch.rand(n, cout, device="cuda") + 0.5
    out = torch.empty(n, cout, 2 * res + 1, cv.tconv_pitch(res), device="cuda")
    times = {}
    for name, wk in (("taps", None), ("wino", u)):
        fn = lambda: cv.tconv3x3s2_forward(x, pc, in_scale=s, out_scale=d, out=out, wt=wk)
        fn(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        times[name] = e0.elapsed_time(e1) / reps * 1e3
        times[name + "_out"] = out[:, :, :, :2 * res + 1].clone()
    a, b = times["taps_out"].double(), times["wino_out"].double()
    rel = float((a - b).abs().max() / a.abs().max())
    del times["taps_out"], times["wino_out"]
    print(f"{cin:3d}->{cout:3d} at {res:3d}^2 n {n}: tap-list + border {times['taps']:7.1f} us   Winograd + border {times['wino']:7.1f} us"
          f"   ({times['wino'] - times['taps']:+7.1f})   max rel diff {rel:.2e}", flush=True)
