"""Recipe of tests/golden/noise_opt_reg.npz: the reference driver's own `noise_regularize` on seeded maps.

    python tools/make_noise_opt_golden.py --reference <checkout of the reference project>

The driver script cannot be imported (it starts a projection at import time and needs its detector libraries), so the one function is taken
out of its syntax tree at run time and evaluated with torch alone; nothing of it is copied.  Per side s in (4, 8, 32) the file holds the
map `x{s}` [1, 1, s, s] (float64, numpy PCG64 seed 20 + s: white for 4 and 8, box-smoothed and renormalised for 32 so that the means are
not ~0) and `reg{s}`, the function's value on [x] in float64, and `reg_all`, its value on the list of the three maps.
"""
import argparse
import ast
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = "1024_example_wing_loss_perceptual_sqz_MSE.py"
SIDES = (4, 8, 32)


def make_map(s):
    rng = np.random.Generator(np.random.PCG64(20 + s))
    x = rng.standard_normal((s, s))
    if s > 8:
        x = sum(np.roll(np.roll(x, i, 0), j, 1) for i in range(3) for j in range(3))
        x = (x - x.mean()) / x.std(ddof=1)
    return x.reshape(1, 1, s, s)


def reference_function(checkout, name):
    with open(os.path.join(checkout, SCRIPT)) as f:
        tree = ast.parse(f.read())
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[node], type_ignores=[]), SCRIPT, "exec"), ns)
    return ns[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "noise_opt_reg.npz"))
    a = ap.parse_args()
    fn = reference_function(a.reference, "noise_regularize")
    out, maps = {}, []
    for s in SIDES:
        x = make_map(s)
        maps.append(torch.from_numpy(x))
        out[f"x{s}"] = x
        out[f"reg{s}"] = np.float64(float(fn([torch.from_numpy(x)])))
    out["reg_all"] = np.float64(float(fn(maps)))
    np.savez_compressed(a.out, **out)
    print(a.out, {k: float(v) for k, v in out.items() if k.startswith("reg")})


if __name__ == "__main__":
    main()
