"""Per-target noise maps for lockstep targets: the set entries of csrc/noise_opt.hip and csrc/adam.hip (mgf_noise_sets_*, mgf_adam_sets_f32) on their own,
then GradientProjectionEngine(optimize_noise=True) with one target (a set of one, against the per-map loops of
tests/noise_per_map_engine.py, bit for bit) and with two different targets and noise_per_target=True (each against its own autograd + Adam
run on the CPU), then the drivers.

A set kernel and its per-map counterpart share their body, their partial counts and their fold order, so per (set, map) the bits are the
per-map entry's: asserted with torch.equal against n_sets x n_maps per-map calls.  The float64 gates are those of
tests/test_hip_noise_opt.py (4 x torch's own float32-vs-float64 distance, floor 4 * 2^-23; both distances are printed as OBS lines)."""
import functools

import numpy as np
import pytest
import torch

import test_hip_noise_opt as base
from guarded_buffers import NAN, Guarded
from noise_per_map_engine import PerMapNoiseEngine
from noise_opt_torch_ref import projection_noise_ref
from noise_sets_torch_ref import BIG_SIDES, SIDES, gapped_table, make_sets, map_of, normalize_sets, regularize_sets
from test_hip_noise_opt import ADAM_EPS, LR, REG_WEIGHT, SKIPPED, STEPS, dist, gate, make_map

pytestmark = pytest.mark.gpu

EINVAL = -1
UNREAD = 99                   # a step slot between the sets' own (step_stride 2): read by mistake it says "past the end", and set 0 would not move
PER_MAP_CALLS = ["mgf_noise_grad_f32", "mgf_noise_regularize_f32", "mgf_noise_regularize_grad_f32", "mgf_noise_normalize_f32",
                 "mgf_adam_elementwise_f32"]
SET_CALLS = ["mgf_noise_sets_regularize_grad_f32", "mgf_noise_sets_normalize_f32", "mgf_noise_sets_grad_f32", "mgf_noise_sets_pack_f32",
             "mgf_adam_sets_f32"]


def _L():
    from morphganformer_amd import _lib
    return _lib, _lib.lib(), _lib.stream_ptr()


def _scratch(L, sides_c, n, n_sets, fill):
    nbytes = int(L.mgf_noise_sets_scratch_bytes(sides_c, n, n_sets))
    assert nbytes > 0
    return torch.full((nbytes // 8,), fill, dtype=torch.float64, device="cuda")


@functools.lru_cache(maxsize=None)
def _reg_case(which, n_sets):
    """Inputs and the torch references of one regulariser case, computed once and read-only afterwards."""
    sides = SIDES if which == "small" else BIG_SIDES
    offsets, extent, stride = gapped_table(sides)
    x = make_sets(make_map, sides, offsets, stride, n_sets, 900 + n_sets)
    v64, g64 = regularize_sets(x, sides, offsets, torch.float64)
    v32, g32 = regularize_sets(x, sides, offsets, torch.float32)
    return dict(sides=sides, offsets=offsets, stride=stride, x=x, v64=v64, g64=g64, v32=v32, g32=g32)


# ---------------------------------------------------------------------------------------------- regulariser sets
@pytest.mark.parametrize("which,n_sets", [("small", 1), ("small", 3), ("big", 2)])
@pytest.mark.parametrize("acc", [0, 1])
def test_regulariser_sets(which, n_sets, acc):
    """Sides [4, 8, 8, 16, 64]: one-level maps at and below the break, two maps of one side, multi-level maps; offsets with gaps, a
    set_stride larger than the extent, 1 and 3 sets of different data.  Sides [1024, 8], 2 sets: 256 partials per level (the cap) and
    grid-stride loops.  (a) float64 gate per set and map, (b) the bits of n_sets x n_maps per-map calls in table order, with and without
    both accumulate flags, (c) gaps and guard bands untouched, (d) a second call on other scratch gives the same bits."""
    _lib, L, st = _L()
    c = _reg_case(which, n_sets)
    sides, offsets, stride = c["sides"], c["offsets"], c["stride"]
    sides_c, offs_c, n = _lib.map_table(sides, offsets)
    scale, vstride, v0 = 3.0, 3, 0.75
    xg = Guarded((n_sets, stride), c["x"])                         # NaN in the gaps: a read outside a map poisons the result
    prior = make_sets(make_map, sides, offsets, stride, n_sets, 77) * 0.01

    def outputs():
        dx = Guarded((n_sets, stride), prior if acc else None)
        val = Guarded((n_sets, vstride))
        if acc:
            val.t[:, 0] = v0
        return dx, val

    dx, val = outputs()
    sc = _scratch(L, sides_c, n, n_sets, NAN)                      # NaN scratch: nothing is read before it is written
    _lib.check(L.mgf_noise_sets_regularize_grad_f32(dx.ptr(), val.ptr(), vstride, xg.ptr(), offs_c, sides_c, n, n_sets, stride, scale, acc, acc,
                                                    sc.data_ptr(), st))
    # (b) the per-map entry, map after map
    dx_ref, val_ref = outputs()
    msc = torch.empty(max(int(L.mgf_noise_regularize_scratch_bytes(s)) for s in sides) // 8, dtype=torch.float64, device="cuda")
    for t in range(n_sets):
        for m, o in enumerate(offsets):
            _lib.check(L.mgf_noise_regularize_grad_f32(dx_ref.t[t, o:].data_ptr(), val_ref.t[t:].data_ptr(), xg.t[t, o:].data_ptr(), sides[m], scale,
                                                       acc, int(acc or m > 0), msc.data_ptr(), st))
    # (a) float64 gates
    p = prior.double() if acc else None
    for t in range(n_sets):
        for m in range(len(sides)):
            pm = map_of(p, t, m, sides, offsets) if acc else 0.0
            gate(f"reg sets {which} set {t} map {m} (side {sides[m]}) acc={acc}", map_of(dx.t, t, m, sides, offsets),
                 (pm.float() if acc else 0.0) + scale * map_of(c["g32"], t, m, sides, offsets), pm + scale * map_of(c["g64"], t, m, sides, offsets))
        gate(f"reg sets value {which} set {t} acc={acc}", val.t[t, :1], ((v0 if acc else 0.0) + scale * c["v32"][t].sum()).reshape(1),
             ((v0 if acc else 0.0) + scale * c["v64"][t].sum()).reshape(1))
    for t in range(n_sets):
        for m in range(len(sides)):
            a, b = map_of(dx.t, t, m, sides, offsets), map_of(dx_ref.t, t, m, sides, offsets)
            assert torch.equal(a, b), (t, m, float((a - b).abs().max()))
    assert torch.equal(val.t[:, 0], val_ref.t[:, 0]), (val.t[:, 0], val_ref.t[:, 0])
    # (c) the gaps of dx, the slots between the values, the guard bands; x itself
    assert torch.equal(torch.isnan(dx.t), torch.isnan(xg.t)) and dx.guard_intact()
    assert bool(torch.isnan(val.t[:, 1:]).all()) and val.guard_intact()
    assert torch.equal(torch.nan_to_num(xg.t.cpu()), torch.nan_to_num(c["x"])) and xg.guard_intact()
    # (d) deterministic
    dx2, val2 = outputs()
    sc2 = _scratch(L, sides_c, n, n_sets, 0.0)
    _lib.check(L.mgf_noise_sets_regularize_grad_f32(dx2.ptr(), val2.ptr(), vstride, xg.ptr(), offs_c, sides_c, n, n_sets, stride, scale, acc, acc,
                                                    sc2.data_ptr(), st))
    assert torch.equal(torch.nan_to_num(dx.t), torch.nan_to_num(dx2.t)) and torch.equal(val.t[:, 0], val2.t[:, 0])


def test_regulariser_sets_without_a_value():
    _lib, L, st = _L()
    c = _reg_case("small", 1)
    sides_c, offs_c, n = _lib.map_table(c["sides"], c["offsets"])
    xg, dx = Guarded((1, c["stride"]), c["x"]), Guarded((1, c["stride"]))
    sc = _scratch(L, sides_c, n, 1, NAN)
    _lib.check(L.mgf_noise_sets_regularize_grad_f32(dx.ptr(), None, 0, xg.ptr(), offs_c, sides_c, n, 1, c["stride"], 1.0, 0, 0, sc.data_ptr(), st))
    gate("reg sets, no value", torch.nan_to_num(dx.t), c["g32"], c["g64"])


# ---------------------------------------------------------------------------------------------- normalise sets
def test_normalise_sets():
    """Three sets: set 0 live, set 1 at a step its `valid` row skips, set 2 past the end.  Set 0 has the per-map entry's bits, the others
    (and every gap) are bit-unchanged."""
    _lib, L, st = _L()
    sides = SIDES
    offsets, extent, stride = gapped_table(sides)
    sides_c, offs_c, n = _lib.map_table(sides, offsets)
    x = make_sets(make_map, sides, offsets, stride, 3, 300) * 1.7 + 0.3
    xg = Guarded((3, stride), x)
    step = torch.tensor([0, UNREAD, 1, UNREAD, 3, UNREAD], dtype=torch.int32, device="cuda")        # step_stride 2
    valid = torch.tensor([[1, 1, 1, 9], [1, 0, 1, 9], [1, 1, 1, 9]], dtype=torch.int32, device="cuda")      # valid_stride 4, steps_total 3
    sc = _scratch(L, sides_c, n, 3, NAN)
    _lib.check(L.mgf_noise_sets_normalize_f32(xg.ptr(), offs_c, sides_c, n, 3, stride, step.data_ptr(), 2, valid.data_ptr(), 4, 3, sc.data_ptr(), st))
    ref = x.cuda()
    nsc = torch.empty(int(L.mgf_noise_normalize_scratch_bytes()) // 8, dtype=torch.float64, device="cuda")
    for m, o in enumerate(offsets):
        _lib.check(L.mgf_noise_normalize_f32(ref[0, o:].data_ptr(), sides[m] ** 2, None, None, 0, nsc.data_ptr(), st))
    got = xg.t
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and xg.guard_intact()
    assert torch.equal(torch.nan_to_num(got[0]), torch.nan_to_num(ref[0]))
    assert torch.equal(torch.nan_to_num(got[1:].cpu()), torch.nan_to_num(x[1:]))
    t64 = normalize_sets(torch.nan_to_num(x), sides, offsets, [0], torch.float64)
    t32 = normalize_sets(torch.nan_to_num(x), sides, offsets, [0], torch.float32)
    for m in range(len(sides)):
        v = map_of(got, 0, m, sides, offsets)
        gate(f"normalise sets map {m}", v, map_of(t32, 0, m, sides, offsets), map_of(t64, 0, m, sides, offsets))
        assert abs(float(v.double().mean())) <= 1e-6 and abs(float(v.double().std(unbiased=True)) - 1.0) <= 1e-6, m
    # no counters at all: every set is live
    yg = Guarded((3, stride), x)
    _lib.check(L.mgf_noise_sets_normalize_f32(yg.ptr(), offs_c, sides_c, n, 3, stride, None, 0, None, 0, 0, sc.data_ptr(), st))
    assert torch.equal(torch.nan_to_num(yg.t[0]), torch.nan_to_num(ref[0]))
    for t in (1, 2):
        for m in range(len(sides)):
            v = map_of(yg.t, t, m, sides, offsets)
            assert abs(float(v.double().mean())) <= 1e-6 and abs(float(v.double().std(unbiased=True)) - 1.0) <= 1e-6, (t, m)


# ---------------------------------------------------------------------------------------------- channel sum
@pytest.mark.parametrize("c,hw", [(8, 16), (130, 67), (33, 70000)])
@pytest.mark.parametrize("acc", [0, 1])
def test_noise_sets_channel_sum(c, hw, acc):
    """Three samples in one launch: the 4 x 4 map, a pixel count that is no multiple of 4 with sliced channels, and more than one block;
    each sample against float64 and against its own per-map call (same slice form: same bits); the gap behind every map stays NaN."""
    _lib, L, st = _L()
    n, stride = 3, hw + 8
    torch.manual_seed(c + hw)
    d = torch.randn(n, c, hw)
    prior = torch.randn(n, hw)
    s = torch.tensor([0.37])

    def output():
        g = Guarded((n, stride))
        if acc:
            g.t[:, :hw] = prior.cuda()
        return g

    out, ref, dd, sd = output(), output(), d.cuda(), s.cuda()
    _lib.check(L.mgf_noise_sets_grad_f32(out.ptr(), stride, dd.data_ptr(), sd.data_ptr(), n, c, hw, acc, st))
    for j in range(n):
        _lib.check(L.mgf_noise_grad_f32(ref.t[j].data_ptr(), dd[j].data_ptr(), sd.data_ptr(), c, hw, acc, st))
        want64 = (prior[j].double() if acc else 0) + float(s) * d[j].double().sum(0)
        t32 = (prior[j] if acc else 0) + s * d[j].sum(0)
        gate(f"noise_sets_grad c={c} hw={hw} acc={acc} sample {j}", out.t[j, :hw], t32, want64)
        assert torch.equal(out.t[j, :hw], ref.t[j, :hw]), j
    assert bool(torch.isnan(out.t[:, hw:]).all()) and out.guard_intact()


# ---------------------------------------------------------------------------------------------- Adam sets
def test_adam_sets_match_the_elementwise_step_per_slice():
    """Three slices with different optimizer counts and step counters, slice 1 with a skipped step, slice 2 running past the end, over four
    steps: parameter, both moments and the count of every slice have the bits of mgf_adam_elementwise_f32 on that slice alone."""
    _lib, L, st = _L()
    n_sets, numel, stride, total = 3, 1000, 1024, 6
    g = torch.Generator().manual_seed(5)
    mk = lambda: torch.randn(n_sets, stride, generator=g)
    p0, grads = mk(), [mk() * (10.0 ** -(i % 3)) for i in range(4)]
    lr = torch.tensor([0.01, 0.02, 0.03, 0.015, 0.01, 0.005]).cuda()
    valid = torch.tensor([[1] * 6, [1, 1, 0, 1, 1, 1], [1] * 6], dtype=torch.int32, device="cuda")
    step0, t0 = [0, 1, 3], [0, 3, 1]

    def state():
        return (p0.cuda().clone(), torch.zeros(n_sets, stride, device="cuda"), torch.zeros(n_sets, stride, device="cuda"),
                torch.tensor(t0, dtype=torch.int32, device="cuda"), torch.tensor(step0, dtype=torch.int32, device="cuda"))

    pa, ma, va, ta, sa = state()
    pb, mb, vb, tb, sb = state()
    for i, gr in enumerate(grads):
        gd = gr.cuda()
        _lib.check(L.mgf_adam_sets_f32(pa.data_ptr(), ma.data_ptr(), va.data_ptr(), ta.data_ptr(), gd.data_ptr(), lr.data_ptr(), sa.data_ptr(), 1,
                                       valid.data_ptr(), total, numel, n_sets, stride, total, 0.9, 0.999, 1e-8, 1e-4, st))
        for t in range(n_sets):
            _lib.check(L.mgf_adam_elementwise_f32(pb[t].data_ptr(), mb[t].data_ptr(), vb[t].data_ptr(), tb[t:].data_ptr(), gd[t].data_ptr(),
                                                  lr.data_ptr(), sb[t:].data_ptr(), valid[t].data_ptr(), numel, total, 0.9, 0.999, 1e-8, 1e-4, st))
        sa.add_(1)
        sb.add_(1)
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(ta, tb), i
    assert ta.tolist() == [4, 6, 4]                      # slice 1 skipped one step, slice 2 ran out of steps after three
    assert torch.equal(pa[:, numel:].cpu(), p0[:, numel:]) and not torch.equal(pa[:, :numel].cpu(), p0[:, :numel])


# ---------------------------------------------------------------------------------------------- refusals of the entries
def test_set_entries_refuse_bad_tables_before_any_launch():
    _lib, L, st = _L()
    sides, offsets = [4, 8], [0, 16]
    sc_, oc_, n = _lib.map_table(sides, offsets)
    stride, n_sets = 80, 2
    x, dx = torch.zeros(n_sets * stride, device="cuda"), torch.full((n_sets * stride,), 5.0, device="cuda")
    val = torch.full((n_sets,), 5.0, device="cuda")
    sc = _scratch(L, sc_, n, n_sets, 0.0)
    step = torch.zeros(n_sets, dtype=torch.int32, device="cuda")

    def reg(dx=dx, x=x, oc=oc_, sd=sc_, n=n, n_sets=n_sets, stride=stride, scratch=sc):
        return L.mgf_noise_sets_regularize_grad_f32(_lib.ptr(dx), val.data_ptr(), 1, _lib.ptr(x), oc, sd, n, n_sets, stride, 1.0, 0, 0,
                                                    _lib.ptr(scratch), st)

    def norm(x=x, oc=oc_, sd=sc_, n=n, n_sets=n_sets, stride=stride, step=step, valid=None, scratch=sc):
        return L.mgf_noise_sets_normalize_f32(_lib.ptr(x), oc, sd, n, n_sets, stride, _lib.ptr(step), 1, _lib.ptr(valid), 0, 4, _lib.ptr(scratch), st)

    def pack(dst=dx, x=x, oc=oc_, sd=sc_, n=n, n_sets=n_sets, stride=stride):
        return L.mgf_noise_sets_pack_f32(_lib.ptr(dst), _lib.ptr(x), oc, sd, n, n_sets, stride, st)

    bad_side = _lib.map_table([4, 12], offsets)[0]
    overlap = _lib.map_table(sides, [0, 15])[1]
    negative = _lib.map_table(sides, [-4, 16])[1]
    many_s, many_o, _ = _lib.map_table([4] * 33, [16 * i for i in range(33)])
    for name, fn in (("regularize_grad", reg), ("normalize", norm), ("pack", pack)):
        cases = {"null x": dict(x=None), "null sides": dict(sd=None), "null offsets": dict(oc=None), "n_maps 0": dict(n=0),
                 "n_maps 33": dict(sd=many_s, oc=many_o, n=33, stride=33 * 16), "n_sets 0": dict(n_sets=0), "side 12": dict(sd=bad_side),
                 "stride below the extent": dict(stride=79), "overlapping maps": dict(oc=overlap), "negative offset": dict(oc=negative)}
        if name != "pack":
            cases["null scratch"] = dict(scratch=None)
        for what, kw in cases.items():
            rc = fn(**kw)
            assert rc == EINVAL, (name, what, rc)
            assert L.mgf_last_error().decode().startswith("noise_sets_" + name), (name, what)
    assert reg(dx=None) == EINVAL and reg(dx=x) == EINVAL and reg(dx=x[stride:]) == EINVAL        # dx aliases x (the same span, and a shifted one)
    assert b"dx must not alias x" in L.mgf_last_error()
    assert norm(step=None, valid=step) == EINVAL and pack(dst=None) == EINVAL and pack(dst=x[8:]) == EINVAL
    torch.cuda.synchronize()
    assert bool((dx == 5.0).all()) and bool((val == 5.0).all()) and not bool(x.any())              # nothing was launched
    # the table itself is fine
    assert reg() == 0 and norm(x=dx) == 0 and pack() == 0
    # channel sum and Adam
    t = torch.zeros(64, device="cuda")
    p = t.data_ptr()
    assert L.mgf_noise_sets_grad_f32(None, 16, p, p, 2, 2, 16, 0, st) == EINVAL and L.mgf_noise_sets_grad_f32(p, 16, None, p, 2, 2, 16, 0, st) == EINVAL
    assert L.mgf_noise_sets_grad_f32(p, 16, p, None, 2, 2, 16, 0, st) == EINVAL and L.mgf_noise_sets_grad_f32(p, 16, p, p, 0, 2, 16, 0, st) == EINVAL
    assert L.mgf_noise_sets_grad_f32(p, 15, p, p, 2, 2, 16, 0, st) == EINVAL and L.mgf_noise_sets_grad_f32(p, 16, p, p, 2, 0, 16, 0, st) == EINVAL

    def adam(param=p, step=step.data_ptr(), n_sets=2, numel=16, stride=16):
        return L.mgf_adam_sets_f32(param, p, p, p, p, p, step, 1, None, 0, numel, n_sets, stride, 4, 0.9, 0.999, 1e-8, 0.0, st)

    assert adam(param=None) == EINVAL and adam(step=None) == EINVAL and adam(n_sets=0) == EINVAL and adam(numel=0) == EINVAL
    assert adam(stride=15) == EINVAL
    # the per-map entries answer what they answered: an unsupported side is MGF_EUNSUPPORTED there
    assert L.mgf_noise_regularize_grad_f32(dx.data_ptr(), None, x.data_ptr(), 12, 1.0, 0, 0, sc.data_ptr(), st) == -2


# ---------------------------------------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def tiny():
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import TINY, make_state_dict
    from oracle.generator_ref import to_torch_state
    sd = make_state_dict(TINY, seed=0)
    return Generator(sd, TINY, "cuda", max_batch=2), to_torch_state(sd), TINY


def _engine(case, objective, noise_init, use_graph, G, cls=None, **extra):
    """base._engine with further keywords and the engine's class (the one-target engines of the comparison)."""
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine
    kw = dict(lm_valid=case["valid"], eps=case["eps"].cuda(), noise_mode="const", use_graph=use_graph, optimize_noise=True, noise_init=noise_init,
              adam_eps=ADAM_EPS, **extra)
    if objective == "lpips":
        kw.update(percept=PerceptualLoss(net="squeeze", allow_random_backbone=True), lm_target=case["lm_t"], lm_steps=case["lm_s"])
    eng = (cls or GradientProjectionEngine)(G, case["target"].cuda(), case["latent_mean"].cuda(), 1.0, case["args"], **kw)
    if noise_init == "randn":
        for k, v in case["start"].items():
            eng.noises[k].copy_(v)
    return eng


@pytest.mark.parametrize("objective,noise_init", [("mse", "randn"), ("lpips", "const")])
def test_one_target_on_the_set_path_is_the_one_target_engine(tiny, objective, noise_init):
    """One target is a set of one: the engine (set kernels; hipGraph replay, and eager) against PerMapNoiseEngine, the same engine with the
    regulariser, Adam and the normalisation restated as loops over the per-map entries: latent and map trajectories, images, losses, best
    step, best latent and best_noises bit for bit; and the engine's own seeded draws with noise_per_target on and off coincide."""
    from morphganformer_amd.projection import GradientProjectionEngine
    G, tsd, cfg = tiny
    case = base._loop_case(objective, noise_init)
    if noise_init == "randn":
        kw = dict(optimize_noise=True, seed=11, use_graph=False)
        a = GradientProjectionEngine(G, case["target"].cuda(), case["latent_mean"].cuda(), 1.0, case["args"], **kw)
        b = GradientProjectionEngine(G, case["target"].cuda(), case["latent_mean"].cuda(), 1.0, case["args"], noise_per_target=True, **kw)
        assert all(torch.equal(a.noises[k], b.noises[k]) and tuple(b.noises[k].shape) == tuple(a.noises[k].shape) for k in a.noises)
    ref_eng = _engine(case, objective, noise_init, True, G, cls=PerMapNoiseEngine)
    want = base._run(ref_eng) + (ref_eng.result(), {k: v.clone() for k, v in ref_eng.best_noises.items()})
    for use_graph in (True, False) if objective == "mse" else (True,):
        eng = _engine(case, objective, noise_init, use_graph, G, noise_per_target=True)
        assert eng.noise_flat.shape == (1, eng.noise_total) and eng.noise_adam_t.shape == (1,)
        traj, ntraj, imgs = base._run(eng)
        for i in range(STEPS):
            assert torch.equal(traj[i], want[0][i]), (use_graph, i)
            for k in ntraj[i]:
                assert torch.equal(ntraj[i][k], want[1][i][k]), (use_graph, i, k, float((ntraj[i][k] - want[1][i][k]).abs().max()))
            assert torch.equal(imgs[i], want[2][i]), (use_graph, i)
        lat, bstep, bloss, losses = eng.result()
        assert torch.equal(lat, want[3][0]) and bstep == want[3][1] and bloss == want[3][2] and np.array_equal(losses, want[3][3], equal_nan=True)
        assert all(torch.equal(eng.best_noises[k], want[4][k]) for k in want[4])
        assert not torch.equal(traj[SKIPPED + 1], traj[SKIPPED]) and torch.equal(traj[SKIPPED], traj[SKIPPED - 1])


@functools.lru_cache(maxsize=None)
def _other_case():
    """Target 0 of the two-target run: another image, another start latent, other eps, other start maps, no skipped step; MSE + regulariser,
    the float64 oracle of base._loop_case.  Computed once, read-only afterwards.  (The start latent's seed is one whose image lies as near
    its target as base's does: MSE 3.8 at step 0 by the CPU oracle against the regulariser's 2.5 at weight 10, a share of 0.40 -- most
    seeds start at an MSE of ~20, where the regulariser would be a tenth of the total and the maps' part of the gate would test little.)"""
    from morphganformer_amd.synth_weights import synthetic_latents
    from oracle.generator_ref import generator_ref, mapping_ref, synthesis_ref, to_torch_state
    from oracle.loss_ref import mse_ref
    one = base._loop_case("mse", "randn")
    cfg, args = one["cfg"], one["args"]
    tsd32 = to_torch_state(one["sd"])
    tsd = {k: v.double() for k, v in tsd32.items()}
    rng = np.random.Generator(np.random.PCG64(137))
    latent_mean = torch.from_numpy(rng.standard_normal((cfg.k, cfg.z_dim)).astype(np.float32))
    eps = torch.from_numpy(rng.standard_normal((STEPS, 1, cfg.k, cfg.z_dim)).astype(np.float32))
    target = generator_ref(tsd32, torch.from_numpy(synthetic_latents(cfg, 1, 1002)), cfg, "const").clamp(-1, 1)
    g = torch.Generator().manual_seed(78)
    start = {k: torch.randn(*v.shape, generator=g) for k, v in one["start"].items()}
    tgt = target.double()
    gen_fn = lambda z, maps: synthesis_ref(tsd, mapping_ref(tsd32, z, cfg).double(), cfg, "inject", maps)
    ref = projection_noise_ref(gen_fn, lambda i, img: args.beta * mse_ref(img, tgt), latent_mean, 1.0, eps, {k: v.double() for k, v in start.items()},
                               STEPS, args.noise_regularize, lr=args.lr, rampdown=args.lr_rampdown, rampup=args.lr_rampup, adam_eps=ADAM_EPS)
    return dict(latent_mean=latent_mean, eps=eps, target=target, start=start, ref=ref, valid=np.ones(STEPS, np.int32))


def _two_target_engine(G, use_graph=True, steps=STEPS):
    from morphganformer_amd.projection import GradientProjectionEngine
    cases = [_other_case(), base._loop_case("mse", "randn")]
    args = cases[1]["args"]
    assert not torch.equal(cases[0]["target"], cases[1]["target"])
    eng = GradientProjectionEngine(G, torch.cat([c["target"] for c in cases]).cuda(), torch.stack([c["latent_mean"] for c in cases]).cuda(), 1.0,
                                   args, lm_valid=np.stack([c["valid"] for c in cases]), eps=torch.cat([c["eps"] for c in cases], 1).cuda(),
                                   noise_mode="const", use_graph=use_graph, optimize_noise=True, noise_per_target=True, adam_eps=ADAM_EPS, seed=4)
    return eng, cases, args


def test_two_targets_each_match_their_own_autograd_adam_run(tiny):
    """Two DIFFERENT targets in lockstep with maps of their own: other start maps, other eps, a skipped step in target 1 only.  Gates of
    test_noise_projection_matches_autograd_adam, per target."""
    from morphganformer_amd.projection import seeded_randn
    G, tsd, cfg = tiny
    eng, cases, args = _two_target_engine(G)
    B, total = 2, eng.noise_total
    assert eng.noise_flat.shape == (B, total) and eng.best_noise_flat.shape == (B, total) and eng.noise_adam_t.shape == (B,)
    # the engine's own draws: target j under seed + 0x6E6F6973 + j
    off = 0
    for name, r in eng.noise_layers:
        assert tuple(eng.noises[name].shape) == (B, r, r) and tuple(eng.best_noises[name].shape) == (B, r, r)
        for j in range(B):
            assert torch.equal(eng.noises[name][j].reshape(-1), seeded_randn((total,), "cuda", 4 + 0x6E6F6973 + j)[off:off + r * r]), (name, j)
        off += r * r
    for j, c in enumerate(cases):
        for k, v in c["start"].items():
            eng.noises[k][j].copy_(v[0])
    traj, ntraj, imgs = [], [], []
    for i in range(STEPS):
        eng.run(1)
        traj.append(eng.latent_in.cpu().clone())
        ntraj.append({k: v.cpu().clone() for k, v in eng.noises.items()})
        imgs.append(eng.G.img.clone())
    lat, bstep, bloss, losses = eng.result()
    for j, c in enumerate(cases):
        ref = c["ref"]
        share = ref["reg"][0] / ref["losses"][0]
        print(f"OBS target {j}: regulariser share of the total at step 0: {share:.3f} (total {ref['losses'][0]:.4f})")
        assert 0.1 < share < 0.9
        assert float((ref["traj"][-1] - c["latent_mean"]).abs().max()) > 5 * args.lr * 0.2
        worst_l = worst_n = 0.0
        for i in range(STEPS):
            bound = 0.05 * args.lr * (i + 1)
            dl = float((traj[i][j] - ref["traj"][i][0]).abs().max())
            worst_l = max(worst_l, dl / bound)
            assert dl < bound, (j, i)
            for k in c["start"]:
                dn = float((ntraj[i][k][j] - ref["noise_traj"][i][k][0]).abs().max())
                worst_n = max(worst_n, dn / bound)
                assert dn < bound, (j, i, k)
        print(f"OBS target {j}: worst latent / map distance as a fraction of the bound: {worst_l:.3f} / {worst_n:.3f}")
        got = np.array([v for v in losses[j] if not np.isnan(v)])
        want = np.array([v for v in ref["losses"] if v is not None])
        assert len(got) == len(want) and np.abs(got - want).max() < 1e-3 * np.abs(want).max(), j
        assert int(bstep[j]) == ref["best_step"] and bstep[j] > 0, (j, bstep, ref["best_step"])
        assert float((lat[j] - ref["best_latent"][0]).abs().max()) < 0.05 * args.lr * STEPS
    # target 1's skipped step: its latent and maps bit-unchanged, target 0's moved
    assert np.isnan(losses[1][SKIPPED]) and not np.isnan(losses[0]).any()
    assert torch.equal(traj[SKIPPED][1], traj[SKIPPED - 1][1]) and not torch.equal(traj[SKIPPED][0], traj[SKIPPED - 1][0])
    for k in cases[0]["start"]:
        assert torch.equal(ntraj[SKIPPED][k][1], ntraj[SKIPPED - 1][k][1]), k
        assert not torch.equal(ntraj[SKIPPED][k][0], ntraj[SKIPPED - 1][k][0]), k
    assert eng.noise_adam_t.tolist() == [STEPS, STEPS - 1]
    # best_noises[j]: the maps target j's best image was generated with, i.e. as they stood BEFORE that step's update
    for j, c in enumerate(cases):
        b = int(bstep[j])
        for k in c["start"]:
            before = ntraj[b - 1][k][j]
            assert torch.equal(eng.best_noises[k][j].cpu(), before), (j, k)
            assert float((before - c["ref"]["best_noises"][k][0]).abs().max()) < 0.05 * args.lr * (b + 1), (j, k)
            assert not torch.equal(ntraj[b][k][j], before), (j, k)
    # G(best latent j, best_noises j) is target j's scored image: through the same two-sample forward bit for bit, and one at a time
    again = eng.gg.forward(lat.cuda(), noise_mode="inject", noises={k: v.contiguous() for k, v in eng.best_noises.items()}).clone()
    for j in range(B):
        scored = imgs[int(bstep[j])][j]
        assert torch.equal(again[j], scored), j
        plain = G.forward_workspace(lat[j:j + 1].cuda(), None, noise_mode="inject", noises={k: v[j:j + 1] for k, v in eng.best_noises.items()})[0]
        assert dist(plain[0], scored) < 1e-4, j


def test_two_targets_graph_equals_eager_and_rewind(tiny):
    G, tsd, cfg = tiny
    runs = []
    for use_graph in (True, False):
        eng, cases, args = _two_target_engine(G, use_graph)
        eng.run()
        runs.append((eng.latent_in.clone(), eng.noise_flat.clone(), eng.best_noise_flat.clone(), eng.result()))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert np.array_equal(a[3][1], b[3][1]) and np.array_equal(a[3][3], b[3][3], equal_nan=True)
    assert bool(a[2].abs().max() > 0)
    eng.rewind()
    assert eng.step_ctr.tolist() == [0, 0] and not bool(eng.best_noise_flat.any()) and all(int(s.count.item()) == 0 for s in eng.noise_slots)
    assert torch.equal(eng.noise_flat, b[1])                     # like the Adam moments: a rewound engine goes on from where the maps stand


def test_wplus_two_targets_moves_and_normalises_every_map(tiny):
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, mapping_only
    G, tsd, cfg = tiny
    cases = [_other_case(), base._loop_case("mse", "randn")]
    w_mean = mapping_only(G, torch.stack([c["latent_mean"] for c in cases]).cuda())
    w_mean = w_mean[:, :, None, :].expand(-1, -1, cfg.num_ws, -1).contiguous() if w_mean.ndim == 3 else w_mean
    args = ProjectionArgs(step=3, lr=LR, lr_rampup=0.2, noise_regularize=1.0)
    eng = GradientProjectionEngine(G, torch.cat([c["target"] for c in cases]).cuda(), w_mean, 1.0, args, noise_mode="const", latent_space="w+",
                                   optimize_noise=True, noise_per_target=True, noise_init="const", seed=3)
    start = eng.noise_flat.clone()
    assert torch.equal(start[0], start[1])                       # "const": every target starts from the layers' noise_const
    lat, bstep, bloss, losses = eng.run().result()
    assert tuple(lat.shape) == (2, cfg.k, cfg.num_ws, cfg.w_dim) and np.isfinite(losses).all()
    for k, v in eng.noises.items():
        for j in range(2):
            assert abs(float(v[j].double().mean())) < 1e-6 and abs(float(v[j].double().std()) - 1) < 1e-6, (k, j)
    assert not torch.equal(eng.noise_flat[0], eng.noise_flat[1]) and not torch.equal(eng.noise_flat, start)


def test_calls_per_step(tiny, monkeypatch):
    """The new path: one regulariser, one normalise, one Adam and one pack call per step whatever the number of targets and maps, one
    channel-sum call per noise layer, none of the per-map calls.  Without optimize_noise: none of either family.  One target: the same
    set calls without the pack, the per-map channel sum, and none of the per-map regulariser, normalise or Adam calls."""
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    G, tsd, cfg = tiny
    counts = base._count_calls(monkeypatch, PER_MAP_CALLS + SET_CALLS)
    eng, cases, args = _two_target_engine(G, use_graph=False)
    assert counts == {n: 0 for n in counts}
    nmaps = len(eng.noise_layers)
    for step in (1, 2):
        eng.run(1)
        assert counts == {**{n: 0 for n in PER_MAP_CALLS}, **{n: step for n in SET_CALLS}, "mgf_noise_sets_grad_f32": step * nmaps}, counts
    for n in counts:
        counts[n] = 0
    one = cases[1]
    tg2 = torch.cat([c["target"] for c in cases]).cuda()
    for use_graph in (False, True):
        GradientProjectionEngine(G, tg2, one["latent_mean"].cuda(), 1.0, ProjectionArgs(step=2, lr=LR), noise_mode="const", use_graph=use_graph).run()
    assert counts == {n: 0 for n in counts}, counts
    # one target is a set of one: the set calls (no pack, the per-map channel sum: one map per layer), none of the per-map loops
    loops = ["mgf_noise_regularize_f32", "mgf_noise_regularize_grad_f32", "mgf_noise_normalize_f32", "mgf_adam_elementwise_f32"]
    mk = lambda use_graph: GradientProjectionEngine(G, one["target"].cuda(), one["latent_mean"].cuda(), 1.0,
                                                    ProjectionArgs(step=2, lr=LR, noise_regularize=1.0), use_graph=use_graph, optimize_noise=True)
    eng = mk(False)
    for step in (1, 2):
        eng.run(1)
        assert counts == {**{n: 0 for n in loops}, "mgf_noise_grad_f32": step * nmaps, "mgf_noise_sets_regularize_grad_f32": step,
                          "mgf_noise_sets_normalize_f32": step, "mgf_adam_sets_f32": step, "mgf_noise_sets_pack_f32": 0,
                          "mgf_noise_sets_grad_f32": 0}, counts
    for n in counts:
        counts[n] = 0
    mk(True).run()
    assert all(counts[n] == 0 for n in loops), counts
    assert all(counts[n] >= 1 for n in ("mgf_noise_sets_regularize_grad_f32", "mgf_noise_sets_normalize_f32", "mgf_adam_sets_f32")), counts


def test_engine_refusals(tiny):
    from morphganformer_amd import _lib
    from morphganformer_amd.demorph import DemorphEngine
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    G, tsd, cfg = tiny
    one = base._loop_case("mse", "randn")
    tg, lm = one["target"].cuda(), one["latent_mean"].cuda()
    tg2 = tg.expand(2, -1, -1, -1).contiguous()
    a = ProjectionArgs(step=2)
    with pytest.raises(_lib.MgfError, match="optimize_noise runs with one target per engine.*per-target maps are not built"):
        GradientProjectionEngine(G, tg2, lm, 1.0, a, optimize_noise=True)
    with pytest.raises(ValueError, match="noise_per_target=True gives every lockstep target its own noise maps"):
        GradientProjectionEngine(G, tg2, lm, 1.0, a, noise_per_target=True)
    with pytest.raises(_lib.MgfError, match="target_b .morph refinement. does not combine with optimize_noise=True"):
        GradientProjectionEngine(G, tg2, lm, 1.0, a, optimize_noise=True, noise_per_target=True, target_b=tg2)

    class _Mdf:
        differentiable = True
    with pytest.raises(_lib.MgfError, match="the MDF objective runs with one target per engine"):
        GradientProjectionEngine(G, tg2, lm, 1.0, a, optimize_noise=True, noise_per_target=True, mdf=_Mdf())
    with pytest.raises(_lib.MgfError, match="DemorphEngine: optimize_noise=True is not built here"):
        DemorphEngine(G, tg, tg, lm, lm, 1.0, a, optimize_noise=True)
    with pytest.raises(TypeError, match="noise_per_target"):
        DemorphEngine(G, tg, tg, lm, lm, 1.0, a, optimize_noise=True, noise_per_target=True)
    eng = GradientProjectionEngine(G, tg2, lm, 1.0, a, optimize_noise=True, noise_per_target=True)
    with pytest.raises(_lib.MgfError, match="an engine of lockstep targets is not re-targeted"):
        eng.retarget(tg2)


# ---------------------------------------------------------------------------------------------- drivers
def test_project_group_returns_the_maps_and_project_many_writes_them(tiny, tmp_path):
    import scipy.io as sio
    from morphganformer_amd import drivers
    from morphganformer_amd.projection import ProjectionArgs
    G, tsd, cfg = tiny
    cases = [_other_case(), base._loop_case("mse", "randn")]
    targets = [c["target"].cuda() for c in cases]
    args = ProjectionArgs(step=4, lr=LR, lr_rampup=0.2, noise_regularize=REG_WEIGHT["mse"])
    kw = dict(args=args, latent_mean=cases[1]["latent_mean"].cuda(), latent_std=1.0, noise_mode="const", seed=2, optimize_noise=True, noise_init="const")
    res = drivers._project_group(G, targets, None, **kw)
    assert len(res["noises"]) == 2 and tuple(res["w"].shape) == (2, cfg.k, cfg.z_dim)
    names = [lp.name for lp in G.plan.layers if lp.noise_strength is not None]
    for j in range(2):
        assert sorted(res["noises"][j]) == sorted(names)
        for lp in G.plan.layers:
            if lp.noise_strength is not None:
                m = res["noises"][j][lp.name]
                assert tuple(m.shape) == (lp.res, lp.res) and abs(float(m.double().std()) - 1) < 1e-3, (j, lp.name)
    assert not torch.equal(res["noises"][0][names[-1]], res["noises"][1][names[-1]])
    prefixes = [str(tmp_path / "out" / f"item{i}") for i in range(2)]
    out = drivers.project_many(G, targets, lockstep=2, mode="gradient", out_prefixes=prefixes, **kw)
    assert "noises" not in out and tuple(out["latents"].shape) == (2, cfg.k, cfg.z_dim) and out["mine"] == [0, 1]
    assert torch.equal(out["latents"].cpu().float(), res["w"].cpu())
    for j, p in enumerate(prefixes):
        m = sio.loadmat(p + ".mat")
        assert sorted(k for k in m if k.startswith("noise_")) == sorted(drivers.noise_mat_key(n) for n in names)
        for n in names:
            assert np.array_equal(m[drivers.noise_mat_key(n)], res["noises"][j][n].cpu().numpy()), (j, n)
        assert np.array_equal(m["w"], res["w"][j:j + 1].numpy())
        assert (tmp_path / "out" / f"item{j}.png").exists()
    # without out_prefixes the maps are dropped: the gathered result is the same
    out2 = drivers.project_many(G, targets, lockstep=2, mode="gradient", **kw)
    assert torch.equal(out2["latents"], out["latents"]) and "noises" not in out2
