"""Per-step cost of two-identity morph refinement against the single-target gradient engine with the same terms:
    python tools/morph_refine_bench.py [--window 200] [--reps 3] [--out profiles/morph_refine_step.txt]
1024^2, k = 17, LPIPS(squeeze) + MSE + IResNet-50 (seeded weights), hipGraph replay; the engines are alternated on one device, `reps` windows
each; then the lockstep 11-alpha sweep (one engine, 11 pairs) is timed beside them."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from morphganformer_amd.engine import Generator                                         # noqa: E402
from morphganformer_amd.iresnet import BiometricLoss, IResNetEmbedder                   # noqa: E402
from morphganformer_amd.lpips import PerceptualLoss                                     # noqa: E402
from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs     # noqa: E402
from morphganformer_amd.synth_weights import FULL1024, make_state_dict                  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=int, default=200)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
out = open(a.out, "w") if a.out else None


def log(*parts):
    s = " ".join(str(x) for x in parts)
    print(s, flush=True)
    if out is not None:
        out.write(s + "\n")
        out.flush()


cfg = FULL1024
sd = make_state_dict(cfg, seed=0)
dev = "cuda"
WIN, REP, WARM = a.window, a.reps, 10
total = WARM + WIN * REP + 8
G = Generator(sd, cfg, dev, max_batch=1)
gen = torch.Generator(device=dev)
gen.manual_seed(1)
z = torch.randn(2, cfg.k, cfg.z_dim, device=dev, generator=gen)
ta = G(z[0:1], None, noise_mode="const")[0].clamp(-1, 1).clone()
tb = G(z[1:2], None, noise_mode="const")[0].clamp(-1, 1).clone()
start = torch.randn(cfg.k, cfg.z_dim, device=dev, generator=gen)
args = ProjectionArgs(step=total)
mk = lambda Gx, t, lm, n, **kw: GradientProjectionEngine(Gx, t, lm, 1.0, args, percept=PerceptualLoss(net="squeeze", allow_random_backbone=True),
                                                          biometric=BiometricLoss(IResNetEmbedder(None, depth=50, n=n, device=dev)), gamma=1e-6,
                                                          noise_mode="random", seed=5, use_graph=True, **kw)
log(f"morph refinement, per-step cost: {cfg.img_resolution}^2, k = {cfg.k}, LPIPS(squeeze) + MSE + IResNet-50 (seeded), hipGraph replay, "
    f"{WIN} steps per window, {REP} windows each, alternated")
engines = {"single target": mk(G, ta, start, 1), "pair mse, id_balance 0": mk(G, ta, start, 1, target_b=tb, morph_alpha=0.5),
           "pair cosine, id_balance 0.5": mk(G, ta, start, 1, target_b=tb, morph_alpha=0.5, id_balance=0.5, id_metric="cosine")}
for e in engines.values():
    e.run(WARM)
torch.cuda.synchronize()
times = {k: [] for k in engines}
for r in range(REP):
    for name, e in engines.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.run(WIN)
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) / WIN * 1e3)
base = float(np.median(times["single target"]))
for name, t in times.items():
    med = float(np.median(t))
    log(f"  {name:30s} ms/step " + "  ".join(f"{v:.4f}" for v in t) + f"   median {med:.4f}   spread {(max(t) - min(t)) / med * 100:.2f} %   vs single {100 * (med / base - 1):+.2f} %")
for name, e in engines.items():
    l = e.losses.cpu().numpy()
    log(f"  {name:30s} losses finite: {bool(np.isfinite(l[:WARM + WIN * REP]).all())}  first {l[0]:.6f}  best {float(e.min_loss):.6f}")
del engines, e
torch.cuda.empty_cache()
B = 11
alphas = [i / 10 for i in range(B)]
GB = Generator(sd, cfg, dev, max_batch=B)
rep = lambda t: t.expand(B, -1, -1, -1).contiguous()
sweep = mk(GB, rep(ta), start, B, target_b=rep(tb), morph_alpha=alphas, id_balance=0.5, id_metric="cosine")
sweep.run(WARM)
torch.cuda.synchronize()
ts = []
for r in range(REP):
    t0 = time.perf_counter()
    sweep.run(40)
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) / 40 * 1e3)
med = float(np.median(ts))
log(f"  lockstep 11-alpha sweep (cosine, id_balance 0.5): ms/step " + "  ".join(f"{v:.3f}" for v in ts) + f"   median {med:.3f} = {med / B:.3f} ms per pair and step "
    f"({base * B / med:.2f} x the rate of 11 single-pair engines run one after the other)")
if out is not None:
    out.close()
