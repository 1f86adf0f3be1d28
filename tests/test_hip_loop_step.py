"""The literal loop's step kernels, called directly through the C ABI and held against the sequential model of tests/loop_step_model.py:
mgf_latent_perturb, mgf_select_best and mgf_keep_improvements bit for bit, and the loss slots mgf_select_best reads (mgf_wing_loss_f64,
mgf_adaptive_wing_loss_f64, mgf_mse_f32, mgf_mse_grad_f32) against float64 with their row tables, strides, accumulate and scale.

Every operand and output is a guarded allocation (tests/guarded_buffers.py): NaN (or a fill pattern) before the call and behind the end, so a
wrong stride reads NaN or writes into the guard.  The inputs come from literal numpy seeds, not from torch's seed: the properties of the
scripted scenario (tests/test_loop_step_host.py asserts them on the CPU) hold under any soak offset."""
import numpy as np
import pytest
import torch

import loop_step_model as M
from guarded_buffers import Guarded
from loop_step_model import F32, F64, I32, SCENARIO

pytestmark = pytest.mark.gpu

F32T, F64T, I32T = torch.float32, torch.float64, torch.int32


def _api():
    from morphganformer_amd import _lib
    return _lib, _lib.lib(), _lib.stream_ptr()


def gin(data, dtype, span=1, offset=0):
    """A guarded operand holding `data` (numpy, any shape)."""
    arr = np.atleast_1d(np.asarray(data))
    return Guarded(arr.shape, torch.from_numpy(np.ascontiguousarray(arr)), span=span, offset=offset, dtype=dtype)


def gptr(g):
    return 0 if g is None else g.ptr()


# ---------------------------------------------------------------------------------------------------------------- mgf_latent_perturb

def _perturb(latent_in, eps, sigma, step, batch, steps_total):
    _lib, L, st = _api()
    numel = latent_in.size
    d_in, d_eps, d_sigma, d_step = gin(latent_in, F32T), gin(eps, F32T), gin(sigma, F32T), gin([step], I32T)
    out = Guarded((batch, numel))
    _lib.check(L.mgf_latent_perturb(out.ptr(), d_in.ptr(), d_eps.ptr(), d_sigma.ptr(), d_step.ptr(), batch, steps_total, numel, st), "latent_perturb")
    torch.cuda.synchronize()
    assert out.guard_intact() and int(d_step.numpy()[0]) == step          # the kernel reads the counter, mgf_select_best advances it
    return out.numpy()


def test_perturb_reproduces_the_reference_run(golden):
    g = golden("loop_tiny.npz")
    steps = g["eps"].shape[0]
    eps, mean, sigma = g["eps"].reshape(steps, -1), g["latent_mean"].reshape(-1), g["sigmas"].astype(F32)
    want = g["latents_n"].reshape(steps, -1)
    for s0 in range(0, steps, 7):                                          # the last launch: 1 real step, 6 clamped to step 49
        rows = _perturb(mean, eps, sigma, s0, 7, steps)
        idx = np.minimum(np.arange(s0, s0 + 7), steps - 1)
        assert M.same_bits(rows, want[idx]), s0
        assert M.same_bits(rows, M.perturb(mean, eps, sigma, s0, 7, steps)), s0
    assert s0 == 49


@pytest.mark.parametrize("numel", [1, 255, 257, 544])
def test_perturb_rows_past_the_end_repeat_the_last_step(numel):
    rng = np.random.default_rng(numel)
    steps_total, batch = 3, 5
    mean, eps = rng.standard_normal(numel).astype(F32), rng.standard_normal((steps_total, numel)).astype(F32)
    sigma = rng.uniform(0.1, 1.5, steps_total).astype(F32)
    for step in (0, 2, steps_total):                                       # a counter already at steps_total: every row is the last step's
        rows = _perturb(mean, eps, sigma, step, batch, steps_total)
        assert M.same_bits(rows, M.perturb(mean, eps, sigma, step, batch, steps_total)), step
        last = (mean + (eps[steps_total - 1] * sigma[steps_total - 1]).astype(F32)).astype(F32)
        for j in range(batch):
            if step + j >= steps_total - 1:
                assert M.same_bits(rows[j], last), (step, j)


# ---------------------------------------------------------------------------------------------------------------- mgf_select_best

class DeviceLoop:
    """The device state of mgf_select_best in guarded buffers, one launch at a time."""

    def __init__(self, numel, steps_total, batch, capacity, min_loss=100.0, valid=None, trail=True):
        self.numel, self.steps_total, self.batch, self.capacity, self.trail = numel, steps_total, batch, capacity, trail
        self.min_loss, self.best_step, self.step = gin([min_loss], F64T), gin([-1], I32T), gin([0], I32T)
        self.best_latent, self.losses_out = Guarded((numel,)), Guarded((steps_total,), dtype=F64T)
        self.take_slot = Guarded((batch,), dtype=I32T) if trail else None
        self.trail_count = gin([0], I32T) if trail else None
        self.trail_steps = gin(np.full(capacity, M.STEP_FILL, I32), I32T) if trail else None
        self.trail_losses = Guarded((capacity,), dtype=F64T) if trail else None
        self.valid = None if valid is None else gin(valid, I32T)
        self.latent_n, self.p, self.w, self.mse = Guarded((batch, numel)), Guarded((batch,)), Guarded((batch,), dtype=F64T), Guarded((batch,))

    def buffers(self):
        names = ["min_loss", "best_step", "step", "best_latent", "losses_out", "take_slot", "trail_count", "trail_steps", "trail_losses", "valid",
                 "latent_n", "p", "w", "mse"]
        return {k: getattr(self, k) for k in names if getattr(self, k) is not None}

    def launch(self, cand, p, w, mse, lamda, beta):
        _lib, L, st = _api()
        for buf, data in ((self.latent_n, cand), (self.p, p), (self.w, w), (self.mse, mse)):
            if data is not None:
                buf.t.copy_(torch.from_numpy(np.ascontiguousarray(data)).view(buf.t.shape))
        if self.trail:
            self.take_slot.t.fill_(self.take_slot.fill)
        rc = L.mgf_select_best(self.min_loss.ptr(), self.best_latent.ptr(), self.best_step.ptr(), self.losses_out.ptr(), self.latent_n.ptr(),
                               self.numel, self.p.ptr() if p is not None else 0, self.w.ptr() if w is not None else 0,
                               self.mse.ptr() if mse is not None else 0, lamda, beta, self.step.ptr(), gptr(self.valid), self.batch,
                               self.steps_total, gptr(self.take_slot), gptr(self.trail_count), self.capacity if self.trail else 0,
                               gptr(self.trail_steps), gptr(self.trail_losses), st)
        _lib.check(rc, "select_best")
        torch.cuda.synchronize()

    def snapshot(self):
        return {k: b.numpy().copy() for k, b in self.buffers().items()}

    def problems(self, state, tag):
        """Every field in which the device differs from the model's state, as text."""
        bad = []
        snap = self.snapshot()
        want = dict(min_loss=np.array([state.min_loss], F64), best_step=np.array([state.best_step], I32), step=np.array([state.step], I32),
                    best_latent=state.best_latent, losses_out=state.losses_out)
        if self.trail:
            want.update(take_slot=state.take_slot, trail_count=np.array([state.trail_count], I32), trail_steps=state.trail_steps,
                        trail_losses=state.trail_losses)
        for k, ref in want.items():
            got = snap[k]
            if not M.same_bits(got, np.asarray(ref, got.dtype).reshape(got.shape)):
                ref = np.asarray(ref, got.dtype).reshape(got.shape)
                where = [int(i) for i in np.flatnonzero([not M.same_bits(got[i:i + 1], ref[i:i + 1]) for i in range(len(got))])]
                show = lambda x: [float(v).hex() if x.dtype.kind == "f" else int(v) for v in x[where[:4]]]
                bad.append(f"{tag}: {k} differs at {where[:12]}: got {show(got)}, model {show(ref)}")
        bad += [f"{tag}: the guard behind {k} was written" for k, b in self.buffers().items() if not b.guard_intact()]
        return bad


def _run_select(numel, steps_total, batch, capacity, lamda, beta, p, w, mse, valid, latents, min_loss=100.0, trail=True, extra=1):
    """All launches of a run (and `extra` more with the counter at steps_total), the whole device state against the model after each one."""
    dev = DeviceLoop(numel, steps_total, batch, capacity, min_loss, valid, trail)
    st = M.LoopState(numel, steps_total, max(capacity, 1), min_loss)
    bad = []
    launches = -(-steps_total // batch)
    for k in range(launches + extra):
        s0 = st.step
        slots = [None if x is None else M.pad(x, s0, batch) for x in (p, w, mse)]
        cand = M.candidate_rows(latents, s0, batch)
        before = dev.snapshot()
        M.select(st, cand, slots[0], slots[1], slots[2], valid, batch, steps_total, lamda, beta, trail=trail)
        dev.launch(cand, slots[0], slots[1], slots[2], lamda, beta)
        bad += dev.problems(st, f"launch {k}")
        if k >= launches:                                               # the counter stood at steps_total: nothing but take_slot may change
            after = dev.snapshot()
            for name in after:
                if name == "take_slot":
                    assert list(after[name]) == [-1] * batch, after[name]
                elif name not in ("latent_n", "p", "w", "mse"):          # (the operands are this launch's own: NaN rows past the end)
                    assert M.same_bits(after[name], before[name]), (k, name)
    assert int(dev.step.numpy()[0]) == steps_total
    return bad, st, dev


def test_select_scripted_scenario():
    """23 steps in launches of 5 with a trail of 4: two improvements in one launch, an exact tie, a NaN total, an invalid step with the best
    total, a launch that overflows the trail by two, candidates past the end -- and eleven rows whose total has other bits when the wing product is
    added by a fused multiply-add.  After every launch the whole device state equals the model's, bit for bit; a sixth launch changes nothing."""
    c = SCENARIO
    p, w, mse, valid, latents = M.scripted_scenario()
    bad, st, dev = _run_select(c["numel"], c["steps_total"], c["batch"], c["trail_capacity"], c["lamda"], c["beta"], p, w, mse, valid, latents,
                               c["min_loss"])
    assert not bad, "\n".join(bad)
    assert st.best_step == 21 and st.trail_count == 9 and list(st.trail_steps) == [0, 2, 10, 21]
    assert M.same_bits(dev.best_latent.numpy(), latents[21])


def _random_run(seed, numel, steps_total, fall=0.6):
    """Float32-valued loss slots with a downward drift (several improvements), a quarter of the steps invalid."""
    rng = np.random.default_rng(seed)
    drift = 1.0 - fall * np.arange(steps_total) / steps_total
    p = (rng.uniform(0.05, 0.9, steps_total) * drift).astype(F32)
    w = (rng.uniform(0.5, 30.0, steps_total) * drift).astype(F32).astype(F64)
    mse = (rng.uniform(0.0, 0.5, steps_total) * drift).astype(F32)
    valid = (rng.random(steps_total) > 0.25).astype(I32)
    valid[:2] = 1
    return p, w, mse, valid, rng.standard_normal((steps_total, numel)).astype(F32)


@pytest.mark.parametrize("use", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)])
def test_select_every_subset_of_loss_slots(use):
    p, w, mse, valid, latents = _random_run(300 + 4 * use[0] + 2 * use[1] + use[2], 33, 11)
    bad, st, _ = _run_select(33, 11, 4, 3, 0.01, 1.0, p if use[0] else None, w if use[1] else None, mse if use[2] else None, valid, latents)
    assert not bad, "\n".join(bad)
    assert st.trail_count >= 3                                          # the trail of 3 fills


@pytest.mark.parametrize("case", ["valid_null", "no_trail", "capacity_1", "lbp_form"])
def test_select_optional_arguments_and_weights(case):
    p, w, mse, valid, latents = _random_run(7, 33, 13)
    kw = dict(numel=33, steps_total=13, batch=4, capacity=3, lamda=0.01, beta=1.0, p=p, w=w, mse=mse, valid=valid, latents=latents)
    if case == "valid_null":
        kw.update(valid=None)
    elif case == "no_trail":                                            # take_slot NULL, every trail argument NULL
        kw.update(trail=False, capacity=0)
    elif case == "capacity_1":                                          # every improvement lands in slot 0; only the last of a launch keeps it
        kw.update(capacity=1)
    else:                                                               # lamda = 1.0 is how the LBP driver adds its float64 distance
        kw.update(lamda=1.0, beta=0.5)
    bad, st, _ = _run_select(**kw)
    assert not bad, "\n".join(bad)
    assert len(st.improved) >= 3
    if case == "capacity_1":
        assert st.trail_count == len(st.improved) and st.trail_steps[0] == st.improved[-1]


@pytest.mark.parametrize("numel,batch", [(1, 1), (1, 64), (544, 1), (544, 64)])
def test_select_sizes(numel, batch):
    steps_total = 6 if batch == 1 else 70                               # 64 + 6 real candidates, 58 past the end
    p, w, mse, valid, latents = _random_run(1000 + numel + batch, numel, steps_total)
    bad, st, _ = _run_select(numel, steps_total, batch, 4, 0.01, 1.0, p, w, mse, valid, latents)
    assert not bad, "\n".join(bad)
    assert len(st.improved) >= 2


def test_select_refuses_a_take_slot_without_a_trail_count():
    _lib, L, st = _api()
    dev = DeviceLoop(4, 3, 2, 2)
    before = dev.snapshot()
    rc = L.mgf_select_best(dev.min_loss.ptr(), dev.best_latent.ptr(), dev.best_step.ptr(), dev.losses_out.ptr(), dev.latent_n.ptr(), 4, dev.p.ptr(),
                           0, 0, 0.01, 1.0, dev.step.ptr(), 0, 2, 3, dev.take_slot.ptr(), 0, 2, dev.trail_steps.ptr(), dev.trail_losses.ptr(), st)
    assert rc == _lib.MGF_EINVAL and "select_best" in L.mgf_last_error().decode()
    torch.cuda.synchronize()
    after = dev.snapshot()
    assert all(M.same_bits(after[k], before[k]) for k in after)


def _fma_rows(n, seed):
    """n rows whose total has other bits with a fused wing product (tests/loop_step_model.fma_differs says so for the sum, the totals confirm it)."""
    rng = np.random.default_rng(seed)
    rows = []
    while len(rows) < n:
        ps, ws, ms = F32(rng.uniform(0.05, 0.9)), F64(F32(rng.uniform(0.5, 30.0))), F32(rng.uniform(0.01, 0.5))
        if M.fma_differs(ps, 0.01, ws) and M.total(ps, ws, ms, 0.01, 1.0, fused=True) != M.total(ps, ws, ms, 0.01, 1.0):
            rows.append((ps, ws, ms))
    return (np.array([r[0] for r in rows], F32), np.array([r[1] for r in rows], F64), np.array([r[2] for r in rows], F32))


def test_joint_losses_row_totals_have_select_bests_bits():
    """csrc/demorph.hip promises that mgf_joint_losses_f32's row_totals[b] is mgf_select_best's expression for row b: on eight rows that a fused
    multiply-add would round differently, both have the model's bits."""
    _lib, L, st = _api()
    n = 8
    p, w, mse = _fma_rows(n, 3)
    assert all(M.fma_differs(p[b], 0.01, w[b]) for b in range(n))
    want = np.array([M.total(p[b], w[b], mse[b], 0.01, 1.0) for b in range(n)], F64)
    dp, dw, dm, step = gin(p, F32T), gin(w, F64T), gin(mse, F32T), gin([0], I32T)
    pj, wj, mj, rows = Guarded((1,)), Guarded((1,), dtype=F64T), Guarded((1,)), Guarded((n,), dtype=F64T)
    _lib.check(L.mgf_joint_losses_f32(pj.ptr(), wj.ptr(), mj.ptr(), rows.ptr(), dp.ptr(), dw.ptr(), dm.ptr(), 0, 0.01, 1.0, step.ptr(), 0, n, 1, st),
               "joint_losses")
    torch.cuda.synchronize()
    assert rows.guard_intact() and pj.guard_intact() and wj.guard_intact() and mj.guard_intact()
    latents = np.random.default_rng(4).standard_normal((n, 5)).astype(F32)
    bad, state, dev = _run_select(5, n, n, 2, 0.01, 1.0, p, w, mse, None, latents, extra=0)
    assert not bad, "\n".join(bad)
    assert M.same_bits(dev.losses_out.numpy(), want)
    assert M.same_bits(rows.numpy(), dev.losses_out.numpy()), (rows.numpy(), dev.losses_out.numpy())


# ---------------------------------------------------------------------------------------------------------------- mgf_keep_improvements

def _overflow_take_slot():
    take = M.run_scenario(upto=3)[-1][0].take_slot
    assert list(take) == [2, -1, -1, -1, 3]                              # the launch that overflows the trail: two slots named, three candidates not kept
    return take


@pytest.mark.parametrize("numel", [7, 1024, 4 * (512 * 256 + 300)])     # scalar path; 16-byte path; past the 512-block cap: a thread's second stride
def test_keep_improvements_matches_the_model(numel):
    _lib, L, st = _api()
    take = _overflow_take_slot()
    batch, capacity = len(take), SCENARIO["trail_capacity"]
    imgs_np = np.random.default_rng(numel).standard_normal((batch, numel)).astype(F32)
    imgs, slots, trail = gin(imgs_np, F32T), gin(take, I32T), Guarded((capacity, numel))
    _lib.check(L.mgf_keep_improvements(trail.ptr(), imgs.ptr(), numel, slots.ptr(), batch, st), "keep_improvements")
    torch.cuda.synchronize()
    want = M.keep(np.full((capacity, numel), np.nan, F32), imgs_np, take)
    got = trail.numpy()
    assert M.same_bits(got, want)
    assert np.isnan(got[0]).all() and np.isnan(got[1]).all() and M.same_bits(got[2], imgs_np[0]) and M.same_bits(got[3], imgs_np[4])
    assert trail.guard_intact() and M.same_bits(imgs.numpy(), imgs_np) and list(slots.numpy()) == list(take)


def test_keep_improvements_refusals():
    _lib, L, st = _api()
    take = gin(_overflow_take_slot(), I32T)
    imgs, trail = Guarded((5, 8)), Guarded((4, 8))
    off_imgs, off_trail = Guarded((5, 8), offset=1), Guarded((4, 8), offset=1)          # 4 bytes past a 16-byte boundary
    assert off_imgs.ptr() % 16 == 4 and imgs.ptr() % 16 == 0
    for t, i in ((off_trail, imgs), (trail, off_imgs)):
        assert L.mgf_keep_improvements(t.ptr(), i.ptr(), 8, take.ptr(), 5, st) == _lib.MGF_EINVAL
        assert "keep_improvements" in L.mgf_last_error().decode()
    assert L.mgf_keep_improvements(trail.ptr(), imgs.ptr(), 8, take.ptr(), 65536, st) == _lib.MGF_EINVAL
    assert "keep_improvements" in L.mgf_last_error().decode()
    torch.cuda.synchronize()
    assert not trail.written() and bool(torch.isnan(off_trail.buf).all())


# ---------------------------------------------------------------------------------------------------------------- the loss slots against float64

WING_CASES = [("rows 0..3", None, 5, 6, [0, 1, 2, 3]), ("pred_step 1", 1, 5, 6, [1, 2, 3, 4]), ("clamped to row 5", 4, 5, 6, [4, 5, 5, 5]),
              ("max_row -1", 4, -1, 8, [4, 5, 6, 7])]


@pytest.mark.parametrize("numel", [1, 63, 136, 257])
@pytest.mark.parametrize("kind", ["wing", "awing"])
def test_wing_losses_row_table_vs_float64(kind, numel):
    """n = 4 candidates read rows (*pred_step + j, clamped to max_row) of a [rows, numel] table; 1e-12 relative against the float64 oracle per row.
    Every row of the table has its own reference value, so a candidate that read another row cannot pass."""
    from oracle.loss_ref import adaptive_wing_loss_ref, wing_loss_ref
    _lib, L, st = _api()
    rng = np.random.default_rng(numel + (0 if kind == "wing" else 5000))
    if kind == "wing":                                                   # landmark coordinates: both sides of |d| = omega = 10
        target = rng.uniform(8.0, 56.0, numel)
        pred = target[None] + rng.uniform(-16.0, 16.0, (8, numel))
        ref = lambda row: float(wing_loss_ref(torch.from_numpy(row), torch.from_numpy(target)))
    else:                                                                # heat maps in [0, 1]: both sides of |d| = theta = 0.5
        target = rng.uniform(0.0, 1.0, numel)
        pred = rng.uniform(0.0, 1.0, (8, numel))
        ref = lambda row: float(adaptive_wing_loss_ref(torch.from_numpy(row), torch.from_numpy(target)))
    refs = np.array([ref(pred[r]) for r in range(8)])
    assert len(set(refs.tolist())) == 8 and np.all(np.isfinite(refs)) and np.all(refs > 0)
    d_target = gin(target, F64T)
    for name, pred_step, max_row, rows, read in WING_CASES:
        table = gin(pred[:rows], F64T, span=2)                           # an unclamped row lands in NaN, inside the allocation
        d_step = None if pred_step is None else gin([pred_step], I32T)
        out = Guarded((4,), dtype=F64T)
        if kind == "wing":
            rc = L.mgf_wing_loss_f64(out.ptr(), table.ptr(), d_target.ptr(), 4, numel, 10.0, 2.0, gptr(d_step), max_row, st)
        else:
            rc = L.mgf_adaptive_wing_loss_f64(out.ptr(), table.ptr(), d_target.ptr(), 4, numel, 14.0, 0.5, 1.0, 2.1, gptr(d_step), max_row, st)
        _lib.check(rc, kind)
        torch.cuda.synchronize()
        got, want = out.numpy(), refs[read]
        print(kind, numel, name, "max relative error", float(np.max(np.abs(got - want) / want)))
        assert out.written() and out.guard_intact(), name
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (name, got, want)


def _mse_additions(numel):
    """The additions on the longest path of mgf_mse_f32's two-stage sum: thread 0 of block 0 adds 4 terms per 16-byte quad it takes (and one
    scalar tail element), 6 wave steps, 3 to join the four waves; the finish block the same over the per-block partials."""
    grid = min(-(-numel // 2048), 1024)
    quads = numel // 4
    per_thread = 4 * -(-quads // (grid * 256)) + (1 if numel % 4 else 0)
    return per_thread + 9 + -(-grid // 256) + 9, grid


@pytest.mark.parametrize("numel,n", [(4, 3), (2052, 3), (2048 * 1024 + 2048, 2), (26001, 1)])
def test_mse_strides_accumulate_and_scale_vs_float64(numel, n):
    """float64 mean((a - b)^2) * scale (+ the previous out).  Every summand is non-negative, so the float32 sum is within (d + 3) 2^-24
    relative of it (3: the difference, the square and the term's own rounding; d: the additions on the longest path); gated at twice that."""
    _lib, L, st = _api()
    rng = np.random.default_rng(numel)
    d, grid = _mse_additions(numel)
    assert (numel, grid, d) in [(4, 1, 23), (2052, 2, 27), (2048 * 1024 + 2048, 1024, 34), (26001, 13, 28)]      # the rule above, worked by hand
    bound = 2 * (d + 3) * 2.0 ** -24
    a = rng.standard_normal((n, numel)).astype(F32)
    b = rng.standard_normal((n, numel)).astype(F32)
    prev = rng.uniform(0.5, 2.0, n).astype(F32)
    scale = 0.25
    da, db = gin(a, F32T), gin(b, F32T)
    scratch = torch.empty(n * int(L.mgf_reduce_scratch_floats()), device="cuda")
    for stride in ((0, numel) if n > 1 else (0,)):
        for accumulate in (0, 1):
            out = gin(prev, F32T)
            _lib.check(L.mgf_mse_f32(out.ptr(), da.ptr(), db.ptr(), n, numel, stride, scale, accumulate, scratch.data_ptr(), st), "mse")
            torch.cuda.synchronize()
            bb = b if stride else np.broadcast_to(b[0], b.shape)
            want = scale * np.mean((a.astype(F64) - bb.astype(F64)) ** 2, axis=1) + (prev.astype(F64) if accumulate else 0.0)
            got = out.numpy().astype(F64)
            err = float(np.max(np.abs(got - want) / want))
            print("mse", numel, n, "stride", stride, "accumulate", accumulate, "relative error", err, "bound", bound)
            assert out.guard_intact() and err <= bound, (stride, accumulate, err, bound)
            assert len(set(want.tolist())) == n


def test_mse_refusals():
    _lib, L, st = _api()
    a, b, out = Guarded((2, 8)), Guarded((2, 8)), Guarded((2,))
    scratch = torch.empty(2 * int(L.mgf_reduce_scratch_floats()), device="cuda")
    assert L.mgf_mse_f32(out.ptr(), a.ptr(), b.ptr(), 2, 6, 0, 1.0, 0, scratch.data_ptr(), st) == _lib.MGF_EINVAL     # the second sample of a would not be 16-byte aligned
    assert "mse" in L.mgf_last_error().decode()
    assert L.mgf_mse_f32(out.ptr(), a.ptr(), b.ptr(), 2, 8, 2, 1.0, 0, scratch.data_ptr(), st) == _lib.MGF_EINVAL
    assert "mse" in L.mgf_last_error().decode()
    torch.cuda.synchronize()
    assert not out.written()


@pytest.mark.parametrize("numel", [4, 2052])
def test_mse_grad_strides_and_accumulate_vs_float64(numel):
    """d (+)= 2 scale (a - b) / numel against float64: three roundings (difference, product, sum) and the float32 coefficient, so 4 float32
    ulps of |prev| + |g| per element."""
    _lib, L, st = _api()
    rng = np.random.default_rng(numel + 1)
    n, scale = 3, 0.25
    a = rng.standard_normal((n, numel)).astype(F32)
    b = rng.standard_normal((n, numel)).astype(F32)
    prev = rng.standard_normal((n, numel)).astype(F32)
    da, db = gin(a, F32T), gin(b, F32T)
    for stride in (0, numel):
        for accumulate in (0, 1):
            d = gin(prev, F32T) if accumulate else Guarded((n, numel))
            _lib.check(L.mgf_mse_grad_f32(d.ptr(), da.ptr(), db.ptr(), n, numel, stride, scale, accumulate, st), "mse_grad")
            torch.cuda.synchronize()
            bb = b if stride else np.broadcast_to(b[0], b.shape)
            g = 2.0 * scale * (a.astype(F64) - bb.astype(F64)) / numel
            p64 = prev.astype(F64) if accumulate else np.zeros_like(g)
            bound = 4.0 * np.spacing((np.abs(p64) + np.abs(g)).astype(F32)).astype(F64)
            err = np.abs(d.numpy().astype(F64) - (p64 + g))
            print("mse_grad", numel, "stride", stride, "accumulate", accumulate, "worst error / bound", float(np.max(err / bound)))
            assert d.written() and d.guard_intact() and np.all(err <= bound), (stride, accumulate, float(np.max(err / bound)))
