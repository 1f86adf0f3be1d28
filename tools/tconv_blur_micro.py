"""Per-layer time of the up-sampling half of the two top blocks at n samples: today's three launches (tap-list transposed conv + border
kernel + streaming blur with the epilogue) against the fused launch (csrc/tconv_blur.hip), alternated, HIP-event time per launch group on
seeded data: python tools/tconv_blur_micro.py [n] [reps] > profiles/tconv_blur_micro.txt"""
import os, sys, math, statistics, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from morphganformer_amd import _lib, conv as cv
n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
cv.TCONV_BLUR_MIN_WGS, cv.TCONV_BLUR_MAX_CIN = 0, 1 << 30          # both layers take the fused launch here: this run decides what is wired
f1 = torch.tensor([1.0, 3.0, 3.0, 1.0], device="cuda") / 8
f2 = torch.outer(f1, f1).contiguous()
for cin, cout, res in ((128, 64, 256), (64, 32, 512)):
    torch.manual_seed(res)
    x = torch.randn(n, cin, res, res, device="cuda")
    wt = torch.randn(cout, cin, 3, 3, device="cuda") / math.sqrt(9 * cin)
    pc = cv.pack_weights(wt)
    s, d = torch.rand(n, cin, device="cuda") + 0.5, torch.rand(n, cout, device="cuda") + 0.5
    noise, strength, bias = torch.randn(1, 4 * res * res, device="cuda"), torch.tensor(0.3, device="cuda"), torch.randn(cout, device="cuda")
    ep = _lib.make_epilogue(bias=bias, noise=noise, noise_strength=strength, noise_n=1, act="lrelu", alpha=0.2, gain=math.sqrt(2.0))
    t = torch.empty(n, cout, 2 * res + 1, cv.tconv_pitch(res), device="cuda")
    y = {k: torch.empty(n, cout, 2 * res, 2 * res, device="cuda") for k in ("three", "fused")}
    assert cv.tconv_blur_ok(n, cin, res, res, cout, y["fused"], f1, ep)

    def three():
        tt = cv.tconv3x3s2_forward(x, pc, in_scale=s, out_scale=d, out=t)
        cv.upfirdn_into(y["three"], tt, f2, up=1, pad=(1, 1, 1, 1), gain=4.0, epilogue=ep, separable=True)

    def fused():
        cv.tconv3x3s2_blur_forward(x, pc, f1, 4.0, in_scale=s, out_scale=d, epilogue=ep, out=y["fused"])
    times = {"three": [], "fused": []}
    for fn in (three, fused, three, fused):                       # warm-up
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in (("three", three), ("fused", fused)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    cv.profile_begin(); three(); fused(); recs = cv.profile_end()
    a, b = y["three"].double(), y["fused"].double()
    rel = float((a - b).abs().max() / a.abs().max())
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"{cin:3d}->{cout:3d} at {res:3d}^2 n {n}, {reps} alternated launches each: three launches median {med['three']:7.1f} us "
          f"(min {min(times['three']):7.1f}, max {max(times['three']):7.1f})   fused median {med['fused']:7.1f} us "
          f"(min {min(times['fused']):7.1f}, max {max(times['fused']):7.1f})   ({med['fused'] - med['three']:+7.1f} us)   max rel diff {rel:.2e}", flush=True)
    for k, fl, sec, _, by in recs:
        print(f"    {k:48s} {sec * 1e6:8.1f} us  {fl / sec / 1e12:6.1f} TFLOP/s  {by / sec / 1e12:5.2f} TB/s", flush=True)
