"""The literal loop's step bookkeeping as a plain sequential model (a helper of tests/test_loop_step_host.py and tests/test_hip_loop_step.py,
not a test module).

include/mgf.h ("Literal projection step bookkeeping") restated one candidate at a time in numpy and python floats: mgf_latent_perturb,
mgf_select_best and mgf_keep_improvements.  Nothing here imports the package: the model is what the kernels are held against, bit for bit.
A python float is an IEEE float64 and every python operator rounds once, so `a + b * c` below is two roundings, never a fused multiply-add;
numpy's float32 operators round once each as well."""
from fractions import Fraction

import numpy as np

F32, F64, I32 = np.float32, np.float64, np.int32
STEP_FILL = -7                    # what an unused trail_steps entry holds (the device tests prefill their buffer with the same value)


def bits(a):
    """The raw bits of a float32 / float64 / integer array, as integers."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(a, b):
    """Bit equality with NaN positions compared separately (any NaN equals any NaN, everything else bit for bit: -0.0 is not +0.0)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def perturb(latent_in, eps, sigma, step, batch, steps_total):
    """latent_n[j] = f32(latent_in + f32(eps[s] * sigma[s])), s = min(step + j, steps_total - 1): two float32 roundings.
    latent_in [numel], eps [steps_total, numel], sigma [steps_total], all float32 -> [batch, numel] float32."""
    latent_in, eps, sigma = np.asarray(latent_in), np.asarray(eps), np.asarray(sigma)
    assert latent_in.dtype == F32 and eps.dtype == F32 and sigma.dtype == F32
    out = np.empty((batch, latent_in.size), F32)
    for j in range(batch):
        s = min(step + j, steps_total - 1)
        prod = (eps[s].reshape(-1) * sigma[s]).astype(F32)
        out[j] = (latent_in.reshape(-1) + prod).astype(F32)
    return out


def _fused(acc, a, b):
    """fma(a, b, acc) in float64: the exact value of a * b + acc, rounded once (to nearest even, by python's exact integer division)."""
    vals = (float(acc), float(a), float(b))
    if any(v != v or v in (float("inf"), float("-inf")) for v in vals):
        return float(a) * float(b) + float(acc)
    return float(Fraction(vals[1]) * Fraction(vals[2]) + Fraction(vals[0]))


def total(p, w, mse, lamda, beta, fused=False):
    """float64(p) + (lamda * w) + float64(float32(beta) * float32(mse)): every operation its own rounding, left to right from 0.0; a term
    that is None is skipped.  fused=True is what the model must NOT be: the wing product added by one fused multiply-add."""
    t = 0.0
    if p is not None:
        t = t + float(F32(p))
    if w is not None:
        t = _fused(t, float(lamda), float(w)) if fused else t + float(lamda) * float(w)
    if mse is not None:
        with np.errstate(all="ignore"):
            t = t + float(F32(F32(beta) * F32(mse)))
    return t


def fma_differs(p, lamda, w):
    """Would `p + lamda * w` as one fused multiply-add have other bits than the product rounded to float64 and then added?"""
    two = float(F32(p)) + float(lamda) * float(w)
    one = _fused(float(F32(p)), lamda, w)
    return bool(bits(F64(two)) != bits(F64(one)))


class LoopState:
    """Everything mgf_select_best keeps on the device.  Buffers that a call has not reached keep their fill: NaN, -1, STEP_FILL."""

    def __init__(self, numel, steps_total, trail_capacity, min_loss=100.0):
        self.min_loss = float(min_loss)
        self.best_latent = np.full(numel, np.nan, F32)
        self.best_step = -1
        self.losses_out = np.full(steps_total, np.nan, F64)
        self.step = 0
        self.take_slot = None                                  # the last launch's, [batch] int32
        self.trail_count = 0
        self.trail_steps = np.full(trail_capacity, STEP_FILL, I32)
        self.trail_losses = np.full(trail_capacity, np.nan, F64)
        self.improved = []                                     # (step, launch) of every improvement: bookkeeping of the model, not of the device


def select(state, latent_n, p, w, mse, valid, batch, steps_total, lamda, beta, trail=True):
    """One mgf_select_best launch on `state`.  latent_n [batch, numel]; p / w / mse indexed by candidate j (None = slot absent); valid
    indexed by STEP (None = all valid).  trail=False is take_slot == NULL: no trail bookkeeping at all.  Returns the totals it formed."""
    s0 = state.step
    capacity = len(state.trail_steps)
    take_slot = np.full(batch, -1, I32)
    last_full_j = -1
    totals = []
    for j in range(batch):
        s = s0 + j
        if s >= steps_total:
            take_slot[j] = -1
            continue
        ok = True if valid is None else bool(valid[s] != 0)
        t = total(None if p is None else p[j], None if w is None else w[j], None if mse is None else mse[j], lamda, beta)
        totals.append(t)
        state.losses_out[s] = t if ok else np.nan
        if not (ok and t < state.min_loss):                    # strict; a NaN total compares false
            continue
        state.min_loss = t
        state.best_step = s
        state.best_latent = np.array(latent_n[j], F32).reshape(-1).copy()
        state.improved.append(s)
        if trail:
            slot = min(state.trail_count, capacity - 1)
            if slot == capacity - 1:
                if last_full_j >= 0:
                    take_slot[last_full_j] = -1                 # the later candidate's image is the one the last slot keeps
                last_full_j = j
            state.trail_steps[slot] = s
            state.trail_losses[slot] = t
            state.trail_count += 1
            take_slot[j] = slot
    state.take_slot = take_slot if trail else None
    state.step = min(s0 + batch, steps_total)
    return totals


def keep(trail_imgs, imgs, take_slot):
    """trail_imgs[take_slot[j]] = imgs[j] for every j with take_slot[j] >= 0, on a copy."""
    out = np.array(trail_imgs, copy=True)
    for j, slot in enumerate(take_slot):
        if slot >= 0:
            out[slot] = imgs[j]
    return out


# ---- the scripted scenario of tests/test_hip_loop_step.py: 23 steps in launches of 5 (the last: 3 real candidates, 2 past the end), a trail of 4
SCENARIO = dict(steps_total=23, batch=5, numel=257, trail_capacity=4, lamda=0.01, beta=1.0, min_loss=100.0)
# what each step is to be: "imp" an improvement, "worse", "tie" (the operands of the running minimum's step again), "nan" (a NaN perceptual
# term), "inv" (valid = 0 with a total below every other).  A trailing "*": p + lamda * w rounds differently when fused, and so does the total.
SCRIPT = ["imp", "worse*", "imp*", "tie", "nan",               # two improvements, the tie and the NaN in one launch
          "inv", "worse*", "worse", "worse", "worse",          # nothing taken: the best total of the run is not valid
          "imp*", "imp", "worse*", "imp*", "imp",              # slots 2, 3, 3, 3: the trail overflows by two, take_slot = 2 -1 -1 -1 3
          "worse*", "imp", "inv", "worse*", "imp",
          "worse*", "imp*", "worse"]


def scripted_scenario():
    """(p float32 [23], w float64 [23], mse float32 [23], valid int32 [23], latents float32 [23, 257]) drawn from a literal seed so that
    every step is what SCRIPT says.  The draws are float32-valued, like the loop's own loss slots."""
    rng = np.random.default_rng(20240607)
    n, lamda, beta = SCENARIO["steps_total"], SCENARIO["lamda"], SCENARIO["beta"]
    assert len(SCRIPT) == n
    p, w, mse, valid = np.zeros(n, F32), np.zeros(n, F64), np.zeros(n, F32), np.ones(n, I32)
    running, best_at, level = SCENARIO["min_loss"], -1, 1.6
    for s, what in enumerate(SCRIPT):
        kind, want = what.rstrip("*"), what.endswith("*")
        if kind == "tie":
            p[s], w[s], mse[s] = p[best_at], w[best_at], mse[best_at]
            continue
        for _ in range(100000):
            if kind == "inv":
                ps, ws, goal = F32(rng.uniform(0.01, 0.03)), F64(F32(rng.uniform(0.5, 2.0))), 0.06
            else:
                ps, ws = F32(rng.uniform(0.05, 0.9)), F64(F32(rng.uniform(0.5, 30.0)))
                goal = level - rng.uniform(0.02, 0.08) if kind == "imp" else (min(running, level) + rng.uniform(0.05, 0.5))
            ms = F32(goal - float(ps) - lamda * float(ws))
            if not ms > 0:
                continue
            t = total(ps, ws, ms, lamda, beta)
            differs = fma_differs(ps, lamda, ws) and total(ps, ws, ms, lamda, beta, fused=True) != t
            if differs != want:
                continue
            if (kind in ("imp", "inv") and t < running) or (kind in ("worse", "nan") and t > running + 0.01):
                break
        else:
            raise AssertionError(f"no draw for step {s} ({what})")
        p[s], w[s], mse[s] = ps, ws, ms
        if kind == "nan":
            p[s] = np.nan
        if kind == "inv":
            valid[s] = 0
        if kind == "imp":
            running, best_at, level = t, s, t
    latents = rng.standard_normal((n, SCENARIO["numel"])).astype(F32)
    return p, w, mse, valid, latents


def run_scenario(upto=None):
    """The model over the scripted scenario: [(state after launch k, totals of launch k)], a deep copy per launch."""
    import copy
    p, w, mse, valid, latents = scripted_scenario()
    c = SCENARIO
    st = LoopState(c["numel"], c["steps_total"], c["trail_capacity"], c["min_loss"])
    out = []
    launches = -(-c["steps_total"] // c["batch"])
    for k in range(launches if upto is None else upto):
        s0 = st.step
        cand = candidate_rows(latents, s0, c["batch"])
        totals = select(st, cand, pad(p, s0, c["batch"]), pad(w, s0, c["batch"]), pad(mse, s0, c["batch"]), valid, c["batch"],
                        c["steps_total"], c["lamda"], c["beta"])
        out.append((copy.deepcopy(st), totals))
    return out


def pad(x, s0, batch):
    """The slots of a launch that starts at step s0: x[s0 : s0 + batch], the candidates past the end NaN."""
    out = np.full(batch, np.nan, x.dtype)
    real = x[s0:s0 + batch]
    out[:len(real)] = real
    return out


def candidate_rows(latents, s0, batch):
    out = np.full((batch, latents.shape[1]), np.nan, F32)
    real = latents[s0:s0 + batch]
    out[:len(real)] = real
    return out
