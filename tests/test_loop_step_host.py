"""The sequential model of the literal loop's step kernels (tests/loop_step_model.py) held against the reference run, against itself under
other launch sizes, and the scripted scenario of tests/test_hip_loop_step.py against the properties its device test relies on -- all on the
CPU, so that the device test cannot pass because its scenario happens to contain nothing."""
import copy

import numpy as np
import pytest

import loop_step_model as M
from loop_step_model import F32, F64, I32, SCENARIO, SCRIPT


@pytest.fixture(scope="module")
def tiny(golden):
    g = golden("loop_tiny.npz")
    steps = g["eps"].shape[0]
    return dict(steps=steps, eps=g["eps"].reshape(steps, -1), mean=g["latent_mean"].reshape(-1), sigma=g["sigmas"].astype(F32),
                latents_n=g["latents_n"].reshape(steps, -1), losses=g["losses"], best_step=int(g["best_step"]), best_loss=float(g["best_loss"]),
                best_latent=g["best_latent"].reshape(-1))


def _run_tiny(tiny, batch, capacity):
    """The reference run's 50 totals through the model in launches of `batch` (the totals ride in the wing slot with lamda = 1: 0.0 + 1.0 * x is x)."""
    steps = tiny["steps"]
    st = M.LoopState(tiny["mean"].size, steps, capacity)
    imgs = np.full((capacity, tiny["mean"].size), np.nan, F32)
    while st.step < steps:
        s0 = st.step
        M.select(st, M.candidate_rows(tiny["latents_n"], s0, batch), None, M.pad(tiny["losses"], s0, batch), None, None, batch, steps, 1.0, 1.0)
        imgs = M.keep(imgs, M.candidate_rows(tiny["latents_n"], s0, batch), st.take_slot)
    return st, imgs


def test_perturb_reproduces_the_reference_latents(tiny):
    for batch in (1, 7, 50):
        for s0 in range(0, tiny["steps"], batch):
            rows = M.perturb(tiny["mean"], tiny["eps"], tiny["sigma"], s0, batch, tiny["steps"])
            want = tiny["latents_n"][np.minimum(np.arange(s0, s0 + batch), tiny["steps"] - 1)]
            assert M.same_bits(rows, want), (batch, s0)


def test_fixture_sigmas_are_float32_values(golden):
    g = golden("loop_tiny.npz")
    assert np.array_equal(g["sigmas"].astype(F32).astype(F64), g["sigmas"])


def test_select_ends_where_the_reference_run_ended(tiny):
    st, _ = _run_tiny(tiny, 1, 50)
    assert st.best_step == tiny["best_step"] and st.min_loss == tiny["best_loss"]
    assert M.same_bits(st.best_latent, tiny["best_latent"]) and M.same_bits(st.best_latent, tiny["latents_n"][st.best_step])
    assert M.same_bits(st.losses_out, tiny["losses"]) and st.step == 50


def test_model_is_invariant_to_the_launch_size(tiny):
    base, base_imgs = _run_tiny(tiny, 1, 50)
    assert 2 <= base.trail_count <= 50                     # the capacity holds every improvement: no slot is overwritten
    for batch in (4, 7, 50, 64):
        st, imgs = _run_tiny(tiny, batch, 50)
        assert (st.min_loss, st.best_step, st.step, st.trail_count) == (base.min_loss, base.best_step, base.step, base.trail_count), batch
        assert st.improved == base.improved, batch
        for name in ("best_latent", "losses_out", "trail_steps", "trail_losses"):
            assert M.same_bits(getattr(st, name), getattr(base, name)), (batch, name)
        assert M.same_bits(imgs, base_imgs), batch
    for k, s in enumerate(base.improved):
        assert base.trail_steps[k] == s and M.same_bits(base_imgs[k], tiny["latents_n"][s])


def test_total_is_three_separate_roundings():
    # 0.01 * 3.0 is inexact; so is the sum
    assert M.total(F32(0.5), 3.0, F32(0.25), 0.01, 1.0) == (0.5 + 0.01 * 3.0) + 0.25
    assert M.total(None, 3.0, None, 0.01, 1.0) == 0.01 * 3.0 and M.total(F32(0.5), None, None, 0.01, 1.0) == 0.5
    # the pixel term's product is float32
    assert M.total(None, None, F32(0.3), 0.01, 0.7) == float(F32(0.7) * F32(0.3)) != float(F32(0.7)) * float(F32(0.3))
    # a case worked by hand: p = 1, lamda = 1 + 2^-30, w = 1 + 2^-30: the product is 1 + 2^-29 + 2^-60, rounded 1 + 2^-29, the sum 2 + 2^-29
    # both ways (no difference); p = -1: two roundings give 2^-29, the fused form keeps the 2^-60
    x = 1.0 + 2.0 ** -30
    assert not M.fma_differs(F32(1.0), x, x)
    assert M.fma_differs(F32(-1.0), x, x) and M.total(F32(-1.0), x, None, x, 1.0) == 2.0 ** -29
    assert M.total(F32(-1.0), x, None, x, 1.0, fused=True) == 2.0 ** -29 + 2.0 ** -60


def test_fma_differs_rate_on_loss_sized_operands():
    """With lamda = 0.01, float32-valued p in [0.05, 0.9) and w in [0.5, 30) a fused multiply-add changes the last bit for roughly one draw
    in eight: the defect the device test looks for is not rare."""
    rng = np.random.default_rng(11)
    hits = sum(M.fma_differs(F32(rng.uniform(0.05, 0.9)), 0.01, F64(F32(rng.uniform(0.5, 30.0)))) for _ in range(4000))
    assert 0.08 * 4000 < hits < 0.20 * 4000, hits


def test_select_tie_nan_and_overflow_rules():
    st = M.LoopState(3, 8, 2, min_loss=1.0)
    lat = np.arange(24, dtype=F32).reshape(8, 3)
    w = np.array([1.0, 0.5, 0.5, np.nan, 0.25, 0.125, 0.0625, 2.0])
    valid = np.array([1, 1, 1, 1, 0, 1, 1, 1], I32)
    M.select(st, lat[:6], None, w[:6], None, valid, 6, 8, 1.0, 1.0)
    # 1.0 ties with the initial minimum (not taken), 0.5 taken (slot 0), 0.5 ties, NaN never wins, 0.25 is invalid, 0.125 taken (slot 1 = last)
    assert list(st.take_slot) == [-1, 0, -1, -1, -1, 1] and st.trail_count == 2 and st.best_step == 5 and st.min_loss == 0.125
    assert np.isnan(st.losses_out[3]) and np.isnan(st.losses_out[4]) and st.losses_out[5] == 0.125 and np.isnan(st.losses_out[6])
    assert st.step == 6
    M.select(st, M.candidate_rows(lat, 6, 6), None, M.pad(w, 6, 6), None, valid, 6, 8, 1.0, 1.0)
    assert list(st.take_slot) == [1, -1, -1, -1, -1, -1] and st.trail_count == 3 and list(st.trail_steps) == [1, 6] and st.step == 8
    assert list(st.trail_losses) == [0.5, 0.0625] and M.same_bits(st.best_latent, lat[6])
    before = copy.deepcopy(st)
    M.select(st, M.candidate_rows(lat, 8, 6), None, M.pad(w, 8, 6), None, valid, 6, 8, 1.0, 1.0)
    assert list(st.take_slot) == [-1] * 6 and st.step == 8 and st.trail_count == 3 and M.same_bits(st.losses_out, before.losses_out)
    # two candidates of ONE launch in the last slot: the earlier one's take_slot goes back to -1, the entry is the later one's
    st = M.LoopState(3, 4, 2, min_loss=1.0)
    M.select(st, lat[:4], None, np.array([0.5, 0.4, 0.3, 0.2]), None, None, 4, 4, 1.0, 1.0)
    assert list(st.take_slot) == [0, -1, -1, 1] and list(st.trail_steps) == [0, 3] and list(st.trail_losses) == [0.5, 0.2] and st.trail_count == 4
    assert M.same_bits(M.keep(np.full((2, 3), np.nan, F32), lat[:4], st.take_slot), lat[[0, 3]])


# ---- the scripted scenario

@pytest.fixture(scope="module")
def scenario():
    p, w, mse, valid, latents = M.scripted_scenario()
    return dict(p=p, w=w, mse=mse, valid=valid, latents=latents, runs=M.run_scenario())


def test_scenario_is_built_from_literals_only():
    a, b = M.scripted_scenario(), M.scripted_scenario()
    assert all(M.same_bits(x, y) for x, y in zip(a, b))
    import inspect
    src = inspect.getsource(M)
    assert "torch" not in src and "morphganformer" not in src and "default_rng(20240607)" in src   # no torch seed for the soak offset to move, no kernels


def test_scenario_has_what_the_device_test_relies_on(scenario):
    c, runs = SCENARIO, scenario["runs"]
    p, w, mse, valid = scenario["p"], scenario["w"], scenario["mse"], scenario["valid"]
    assert len(runs) == 5 and (c["steps_total"], c["batch"], c["numel"], c["trail_capacity"], c["lamda"], c["beta"]) == (23, 5, 257, 4, 0.01, 1.0)
    totals = [t for _, ts in runs for t in ts]
    assert len(totals) == 23 and [len(ts) for _, ts in runs] == [5, 5, 5, 5, 3]
    final = runs[-1][0]
    improved = final.improved
    assert improved == [s for s, what in enumerate(SCRIPT) if what.startswith("imp")]
    # the running minimum before each step
    before, m = [], c["min_loss"]
    for s, t in enumerate(totals):
        before.append(m)
        if s in improved:
            m = t
    # an exact tie with the running minimum, valid, and not taken
    ties = [s for s, t in enumerate(totals) if valid[s] and t == before[s]]
    assert ties == [3] and 3 not in improved and M.same_bits(F64(totals[3]), F64(totals[2]))
    # a NaN total
    nans = [s for s, t in enumerate(totals) if t != t]
    assert nans == [4] and valid[4] == 1
    # an invalid step whose total would have been the best of the whole run
    inv = [s for s in range(23) if valid[s] == 0]
    assert inv == [5, 17] and all(totals[s] < min(t for k, t in enumerate(totals) if valid[k] and t == t) for s in inv)
    assert all(np.isnan(final.losses_out[s]) for s in inv + nans) and final.best_step == improved[-1] == 21
    # a launch with at least 2 improvements; a launch that overflows the trail by at least 2
    per_launch = [[s for s in improved if s // 5 == k] for k in range(5)]
    assert max(len(x) for x in per_launch) >= 2 and len(per_launch[0]) == 2
    count_before = {s: improved.index(s) for s in improved}
    overflow = [sum(1 for s in x if count_before[s] >= c["trail_capacity"]) for x in per_launch]
    assert overflow[2] >= 2, overflow
    assert list(runs[2][0].take_slot) == [2, -1, -1, -1, 3] and runs[2][0].trail_count == 6
    assert list(runs[2][0].trail_steps) == [0, 2, 10, 14] and list(final.take_slot) == [-1, 3, -1, -1, -1]      # the last two are past the end
    assert final.trail_count == len(improved) == 9 and list(final.trail_steps) == [0, 2, 10, 21] and final.step == 23
    # at least 8 rows on which a fused multiply-add gives other bits -- in the product sum AND in the finished total --, one of them an improvement
    differ = [s for s in range(23) if p[s] == p[s] and M.fma_differs(p[s], c["lamda"], w[s])
              and M.total(p[s], w[s], mse[s], c["lamda"], c["beta"], fused=True) != totals[s]]
    assert len(differ) >= 8 and set(differ) & set(improved), differ
    assert differ == [s for s, what in enumerate(SCRIPT) if what.endswith("*") or s == 3]
    assert any(valid[s] for s in differ if s in improved)


def test_scenario_totals_follow_the_header_expression(scenario):
    p, w, mse = scenario["p"], scenario["w"], scenario["mse"]
    assert p.dtype == F32 and w.dtype == F64 and mse.dtype == F32
    for s, t in enumerate(t for _, ts in scenario["runs"] for t in ts):
        if s != 4:
            assert t == (float(p[s]) + 0.01 * float(w[s])) + float(F32(1.0) * mse[s]), s
