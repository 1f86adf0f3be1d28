"""Reference-based latent de-morphing (csrc/demorph.hip, demorph.DemorphEngine, drivers.demorph, `python -m morphganformer_amd.demorph`).

The three kernels against numpy evaluating the stated expressions in the stated order, bit for bit; the coupling's transparency (alpha = 1: the
rows are the parameters, the trajectories equal a plain lockstep engine's bit for bit); the loop against torch autograd + torch.optim.Adam over
both parameters on the CPU (tests/demorph_torch_ref.py), with the gates of tests/test_hip_gradient.py; the fixed point; W+; refusals; the driver
and the module entry; and that the default engine makes none of the new calls."""
import functools
import os

import numpy as np
import pytest
import torch

from demorph_torch_ref import demorph_ref
from test_hip_noise_opt import _count_calls

pytestmark = pytest.mark.gpu

NEW_CALLS = ["mgf_latent_mix_f32", "mgf_latent_mix_bwd_f32", "mgf_joint_losses_f32"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


# ---------------------------------------------------------------------------------------------- the kernels
def mix_np(coef, params):
    """rows[b] = sum_p coef[b, p] * params[p] in float32: every product rounded, summed in p order from the first product."""
    rows = np.empty((coef.shape[0], params.shape[1]), np.float32)
    for b in range(coef.shape[0]):
        acc = coef[b, 0] * params[0]
        for p in range(1, coef.shape[1]):
            acc = acc + coef[b, p] * params[p]
        assert acc.dtype == np.float32
        rows[b] = acc
    return rows


def mix_bwd_np(coef, drows, row_weight):
    """dparams[p] = f32(sum_b (f64(rw[b]) * f64(coef[b, p])) * f64(drows[b])): float64 in b order from the first product, one rounding."""
    rw = np.ones(coef.shape[0], np.float64) if row_weight is None else row_weight.astype(np.float64)
    wc = rw[:, None] * coef.astype(np.float64)
    d64 = drows.astype(np.float64)
    out = np.empty((coef.shape[1], drows.shape[1]), np.float32)
    for p in range(coef.shape[1]):
        acc = wc[0, p] * d64[0]
        for b in range(1, coef.shape[0]):
            acc = acc + wc[b, p] * d64[b]
        out[p] = acc.astype(np.float32)
    return out


def _coef(n_rows, n_params, seed):
    """Non-dyadic values (0.3, 0.7 and random ones) with zeros and a one among them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    c = rng.standard_normal((n_rows, n_params)).astype(np.float32)
    flat = c.reshape(-1)
    flat[0], flat[1] = np.float32(0.3), np.float32(0.7)
    flat[-1] = 0.0
    if flat.size > 3:
        flat[2] = 1.0
    return c


SHAPES = [(2, 2), (1, 2), (3, 2), (2, 3)]
NUMELS = [1, 5, 544, 4099, 9792]          # scalar tails, the z latent, more than one workgroup of the scalar path, the W+ latent (float4 path, ten workgroups)


@pytest.mark.parametrize("numel", NUMELS)
@pytest.mark.parametrize("n_rows,n_params", SHAPES)
def test_latent_mix_bit_for_bit(n_rows, n_params, numel):
    from morphganformer_amd import _lib
    L = _lib.lib()
    rng = np.random.Generator(np.random.PCG64(numel + 10 * n_rows + n_params))
    coef = _coef(n_rows, n_params, numel)
    params = rng.standard_normal((n_params, numel)).astype(np.float32)
    rows = torch.full((n_rows + 1, numel), 7.0, device="cuda")                 # a guard row behind the output
    d_params, d_coef = _dev(params), _dev(coef)                                # (held: a temporary's block would be handed to the next one)
    _lib.check(L.mgf_latent_mix_f32(rows.data_ptr(), d_params.data_ptr(), d_coef.data_ptr(), n_rows, n_params, numel, _lib.stream_ptr()))
    assert same_bits(rows[:n_rows], mix_np(coef, params))
    assert bool((rows[n_rows] == 7.0).all())


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("numel", NUMELS)
@pytest.mark.parametrize("n_rows,n_params", SHAPES)
def test_latent_mix_bwd_bit_for_bit(n_rows, n_params, numel, weighted):
    from morphganformer_amd import _lib
    L = _lib.lib()
    rng = np.random.Generator(np.random.PCG64(numel + 10 * n_rows + n_params + 1000))
    coef = _coef(n_rows, n_params, numel + 1)
    drows = (rng.standard_normal((n_rows, numel)) * 1e-3).astype(np.float32)
    rw = np.array([0.3, 1.7, 0.0][:n_rows], np.float32) if weighted else None
    out = torch.full((n_params + 1, numel), 7.0, device="cuda")
    d_drows, d_coef, d_rw = _dev(drows), _dev(coef), (None if rw is None else _dev(rw))
    _lib.check(L.mgf_latent_mix_bwd_f32(out.data_ptr(), d_drows.data_ptr(), d_coef.data_ptr(), _lib.ptr(d_rw), n_rows, n_params, numel, _lib.stream_ptr()))
    assert same_bits(out[:n_params], mix_bwd_np(coef, drows, rw))
    assert bool((out[n_params] == 7.0).all())


@pytest.mark.parametrize("shape", [(1, 17, 32), (1, 17, 6, 32)], ids=["z", "wplus"])
@pytest.mark.parametrize("alpha", [0.3, 0.5])
def test_latent_mix_is_merge_morphs_blend(alpha, shape):
    """coef = [[f32(1 - a), f32(a)], [1, 0]]: row 0 is drivers._blend_latents bit for bit (the a = 0.5 spelling included), row 1 is params[0]."""
    from morphganformer_amd import _lib, drivers
    rng = np.random.Generator(np.random.PCG64(int(alpha * 10)))
    wa, wb = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    coef = np.array([[np.float32(1.0 - alpha), np.float32(alpha)], [1.0, 0.0]], np.float32)
    params = _dev(np.stack([wa.reshape(-1), wb.reshape(-1)]))
    rows, d_coef = torch.empty_like(params), _dev(coef)
    _lib.check(_lib.lib().mgf_latent_mix_f32(rows.data_ptr(), params.data_ptr(), d_coef.data_ptr(), 2, 2, wa.size, _lib.stream_ptr()))
    assert same_bits(rows[0].reshape(shape), drivers._blend_latents(wa, wb, alpha))
    assert same_bits(rows[1].reshape(shape), wa)


def joint_np(p, w, m, rw, lamda, beta):
    rw64 = np.ones(len(p), np.float64) if rw is None else rw.astype(np.float64)

    def joint(slot):
        acc = rw64[0] * np.float64(slot[0])
        for b in range(1, len(slot)):
            acc = acc + rw64[b] * np.float64(slot[b])
        return acc
    totals = np.array([(0.0 + np.float64(p[b])) + np.float64(lamda) * w[b] + np.float64(np.float32(beta) * m[b]) for b in range(len(p))], np.float64)
    return np.float32(joint(p)), np.float64(joint(w)), np.float32(joint(m)), totals


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n_rows", [2, 3])
def test_joint_losses(n_rows, weighted):
    """A live step, a valid = 0 step (row totals NaN, joint slots written all the same), a step past the end (nothing written), and a
    repeated call (same bits: the kernel reads the step counter and does not advance it)."""
    from morphganformer_amd import _lib
    L, steps = _lib.lib(), 4
    rng = np.random.Generator(np.random.PCG64(n_rows))
    p, m = rng.random(n_rows).astype(np.float32), rng.random(n_rows).astype(np.float32)
    w = rng.random(n_rows) * 30
    rw = np.array([0.3, 1.7, 0.6][:n_rows], np.float32) if weighted else None
    lamda, beta = 0.01, 0.7
    valid = _dev(np.array([1, 0, 1, 1], np.int32))
    dp, dw, dm, drw = _dev(p), _dev(w), _dev(m), (None if rw is None else _dev(rw))
    pj, wj, mj = torch.full((1,), 5.0, device="cuda"), torch.full((1,), 5.0, dtype=torch.float64, device="cuda"), torch.full((1,), 5.0, device="cuda")
    totals = torch.full((n_rows, steps), 5.0, dtype=torch.float64, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(row_totals=totals):
        _lib.check(L.mgf_joint_losses_f32(pj.data_ptr(), wj.data_ptr(), mj.data_ptr(), _lib.ptr(row_totals), dp.data_ptr(), dw.data_ptr(), dm.data_ptr(),
                                          _lib.ptr(drw), lamda, beta, step.data_ptr(), valid.data_ptr(), n_rows, steps, _lib.stream_ptr()))
    want = joint_np(p, w, m, rw, lamda, beta)
    for rep in range(2):                       # live step 0, twice
        call()
        assert int(step.item()) == 0
        assert same_bits(pj, np.array([want[0]])) and same_bits(wj, np.array([want[1]])) and same_bits(mj, np.array([want[2]]))
        assert same_bits(totals[:, 0], want[3]) and bool((totals[:, 1:] == 5.0).all())
    for t in (pj, wj, mj):
        t.fill_(5.0)
    step.fill_(1)                              # a skipped step
    call()
    assert same_bits(pj, np.array([want[0]])) and same_bits(wj, np.array([want[1]])) and same_bits(mj, np.array([want[2]]))
    assert bool(torch.isnan(totals[:, 1]).all()) and same_bits(totals[:, 0], want[3]) and bool((totals[:, 2:] == 5.0).all())
    for t in (pj, wj, mj):
        t.fill_(5.0)
    before = totals.clone()
    step.fill_(steps)                          # past the end
    call()
    assert float(pj) == 5.0 and float(wj) == 5.0 and float(mj) == 5.0 and torch.equal(torch.nan_to_num(totals, nan=-1.0), torch.nan_to_num(before, nan=-1.0))
    step.fill_(2)                              # no trace asked for
    call(None)
    assert same_bits(pj, np.array([want[0]])) and bool((totals[:, 2] == 5.0).all())


def test_kernels_refuse_what_they_do_not_take():
    from morphganformer_amd import _lib
    L, st = _lib.lib(), _lib.stream_ptr()
    n = 16
    a, b = torch.zeros(2, n, device="cuda"), torch.zeros(2, n, device="cuda")
    coef, rw = torch.zeros(2, 2, device="cuda"), torch.ones(2, device="cuda")

    def refused(rc, word):
        msg = L.mgf_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg)
    A, B, Cf, R = a.data_ptr(), b.data_ptr(), coef.data_ptr(), rw.data_ptr()
    for mix, name in ((lambda rows, params, c, r, p, ne: L.mgf_latent_mix_f32(rows, params, c, r, p, ne, st), "latent_mix"),
                      (lambda rows, params, c, r, p, ne: L.mgf_latent_mix_bwd_f32(rows, params, c, R, r, p, ne, st), "latent_mix_bwd")):
        refused(mix(0, B, Cf, 2, 2, n), "NULL")
        refused(mix(A, 0, Cf, 2, 2, n), "NULL")
        refused(mix(A, B, 0, 2, 2, n), "NULL")
        for r, p in ((0, 2), (9, 2), (2, 0), (2, 9), (-1, 2)):
            refused(mix(A, B, Cf, r, p, n), "1..8")
        refused(mix(A, B, Cf, 2, 2, 0), "numel")
        refused(mix(A, B, Cf, 2, 2, -3), "numel")
        refused(mix(A, A, Cf, 2, 2, n), "alias")
        refused(mix(A, a[1:].data_ptr(), Cf, 2, 2, n), "alias")               # a partial overlap (refused before anything is launched)
        assert mix(A, B, Cf, 2, 2, n) == 0, name
    p, m, w = torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda"), torch.zeros(2, dtype=torch.float64, device="cuda")
    pj, mj, wj = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    jl = lambda pj_, wj_, mj_, p_, w_, m_, s_, rows=2, total=4: L.mgf_joint_losses_f32(pj_, wj_, mj_, 0, p_, w_, m_, R, 0.01, 1.0, s_, 0, rows, total, st)
    P, W, M, PJ, WJ, MJ, S = (t.data_ptr() for t in (p, w, m, pj, wj, mj, step))
    refused(jl(PJ, WJ, MJ, P, W, M, 0), "step counter")
    refused(jl(PJ, WJ, MJ, P, W, M, S, rows=0), "1..8")
    refused(jl(PJ, WJ, MJ, P, W, M, S, rows=9), "1..8")
    refused(jl(PJ, WJ, MJ, P, W, M, S, total=0), "steps_total")
    refused(jl(0, WJ, MJ, P, W, M, S), "together")
    refused(jl(PJ, WJ, MJ, 0, W, M, S), "together")
    refused(jl(0, 0, 0, 0, 0, 0, S), "no loss slot")
    refused(jl(P, WJ, MJ, P, W, M, S), "alias")
    refused(jl(PJ, W, MJ, P, W, M, S), "alias")
    assert jl(PJ, WJ, MJ, P, W, M, S) == 0 and jl(PJ, 0, 0, P, 0, 0, S) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the engine
STEPS, LR, SKIPPED = 10, 0.05, 3
ADAM_EPS = 1e-6                           # tests/test_hip_noise_opt.py's, for the reason documented there (elements whose gradient is rounding noise)


@pytest.fixture(scope="module")
def tiny():
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import TINY, make_state_dict
    return Generator(make_state_dict(TINY, seed=0), TINY, "cuda", max_batch=2), TINY


@functools.lru_cache(maxsize=None)
def _inputs():
    """The morph / reference pair and the starts of every loop test, computed once and read-only afterwards: the targets are the CPU oracle's
    images of a known latent pair (the morph at alpha 0.4), the descents start elsewhere."""
    from morphganformer_amd import drivers
    from morphganformer_amd.projection import synthetic_landmarks
    from morphganformer_amd.synth_weights import TINY as cfg, make_state_dict, synthetic_latents
    from oracle.generator_ref import generator_ref, to_torch_state
    sd = make_state_dict(cfg, seed=0)
    tsd32 = to_torch_state(sd)
    z = synthetic_latents(cfg, 2, 1001)
    zm = drivers._blend_latents(z[0:1], z[1:2], 0.4)
    with torch.no_grad():
        morph = generator_ref(tsd32, torch.from_numpy(zm), cfg, "const").clamp(-1, 1)
        reference = generator_ref(tsd32, torch.from_numpy(z[0:1]), cfg, "const").clamp(-1, 1)
    rng = np.random.Generator(np.random.PCG64(41))
    start_a = torch.from_numpy(rng.standard_normal((cfg.k, cfg.z_dim)).astype(np.float32))
    start_b = torch.from_numpy(rng.standard_normal((cfg.k, cfg.z_dim)).astype(np.float32))
    eps = torch.from_numpy(rng.standard_normal((STEPS, 2, cfg.k, cfg.z_dim)).astype(np.float32))
    lms = [synthetic_landmarks(STEPS, 64, 9 + b) for b in range(2)]
    valid = np.ones(STEPS, np.int32)
    valid[SKIPPED] = 0
    return dict(cfg=cfg, tsd32=tsd32, morph=morph, reference=reference, start_a=start_a, start_b=start_b, eps=eps, valid=valid,
                lm_t=np.stack([l[0] for l in lms]), lm_s=np.stack([l[1] for l in lms]))


def _args():
    from morphganformer_amd.projection import ProjectionArgs
    return ProjectionArgs(step=STEPS, lr=LR, lr_rampup=0.2)


@functools.lru_cache(maxsize=None)
def _oracle(objective, alpha):
    """The CPU oracle run of one loop case, once per session.  The synthesis network and the losses run in float64 on the float32 inputs, as
    tests/test_hip_noise_opt.py's _loop_case does and for its reason: the gates are spent on the engine's rounding, not the reference's own."""
    from morphganformer_amd.lpips import WEIGHTS_DIR
    from oracle.generator_ref import mapping_ref, synthesis_ref
    from oracle.loss_ref import backbone_random, lpips_ref, mse_ref, wing_loss_ref
    c = _inputs()
    cfg, tsd32, args, valid = c["cfg"], c["tsd32"], _args(), c["valid"]
    tsd = {k: v.double() for k, v in tsd32.items()}
    tg = [c["morph"].double(), c["reference"].double()]
    if objective == "mse":
        loss_fn = lambda i, b, img: None if not valid[i] else args.beta * mse_ref(img, tg[b])
    else:
        bb = {k: v.double() for k, v in backbone_random("squeeze", 0).items()}
        lin = np.load(os.path.join(WEIGHTS_DIR, "lpips_lin_squeeze.npz"))
        lins = [torch.from_numpy(lin[f"lin{i}"]).double().reshape(-1) for i in range(7)]

        def loss_fn(i, b, img):
            if not valid[i]:
                return None
            w = wing_loss_ref(torch.from_numpy(c["lm_s"][b, i]), torch.from_numpy(c["lm_t"][b]))
            return lpips_ref(bb, lins, img, tg[b]).sum() + args.lamda * w + args.beta * mse_ref(img, tg[b])
    # (the oracle's mapping network is float32 by construction, so the latents and the mix stay float32 on both sides)
    gen_fn = lambda z: synthesis_ref(tsd, mapping_ref(tsd32, z, cfg).double(), cfg, "const")
    return demorph_ref(gen_fn, loss_fn, c["start_a"], c["start_b"], 1.0, c["eps"], STEPS, alpha, lr=args.lr, rampdown=args.lr_rampdown,
                       rampup=args.lr_rampup, adam_eps=ADAM_EPS)


def _engine(G, objective, alpha, use_graph, **kw):
    from morphganformer_amd.demorph import DemorphEngine
    from morphganformer_amd.lpips import PerceptualLoss
    c = _inputs()
    if objective == "lpips":
        kw.update(percept=PerceptualLoss(net="squeeze", allow_random_backbone=True), lm_target=c["lm_t"], lm_steps=c["lm_s"])
    kw.setdefault("adam_eps", ADAM_EPS)
    kw.setdefault("lm_valid", c["valid"])
    return DemorphEngine(G, c["morph"].cuda(), c["reference"].cuda(), c["start_a"].cuda(), c["start_b"].cuda(), 1.0, _args(), alpha=alpha,
                         eps=c["eps"].cuda(), noise_mode="const", use_graph=use_graph, **kw)


def _run(eng):
    traj = []
    for _ in range(STEPS):
        eng.run(1)
        traj.append(eng.latent_in.cpu().clone())
    return traj


@pytest.mark.parametrize("alpha", [0.5, 0.3])
@pytest.mark.parametrize("objective,use_graph", [("mse", True), ("mse", False), ("lpips", True)])
def test_demorph_loop_matches_autograd_adam(tiny, objective, use_graph, alpha):
    """The coupled loop against autograd + Adam([p_A, p_B]) on the CPU: MSE (hipGraph replay and eager) and LPIPS(squeeze, random backbone) +
    Wing + MSE, a skipped step, injected eps.  Gates of test_gradient_projection_matches_autograd_adam."""
    G, cfg = tiny
    c, ref, args = _inputs(), _oracle(objective, alpha), _args()
    eng = _engine(G, objective, alpha, use_graph)
    traj = _run(eng)
    res = eng.result()
    # the oracle run is no no-op: both parameters moved, differently, and both rows carry a visible share of the joint loss
    moved_a, moved_b = ref["traj_a"][-1] - c["start_a"], ref["traj_b"][-1] - c["start_b"]
    share = ref["row_losses"][0][0] / ref["losses"][0]
    print(f"OBS oracle {objective} alpha {alpha}: moved p_A {float(moved_a.abs().max()):.4f} p_B {float(moved_b.abs().max()):.4f}  "
          f"morph row's share of the joint loss at step 0 {share:.3f} (joint {ref['losses'][0]:.4f})  best step {ref['best_step']}")
    assert float(moved_a.abs().max()) > 5 * args.lr * 0.2 and float(moved_b.abs().max()) > 5 * args.lr * 0.2
    assert not torch.equal(moved_a, moved_b)
    assert 0.1 < share < 0.9 and 0.1 < ref["row_losses"][1][0] / ref["losses"][0] < 0.9
    worst = 0.0
    for i in range(STEPS):
        bound = 0.05 * args.lr * (i + 1)
        da, db = float((traj[i][0] - ref["traj_a"][i]).abs().max()), float((traj[i][1] - ref["traj_b"][i]).abs().max())
        worst = max(worst, da / bound, db / bound)
        assert da < bound and db < bound, (i, da, db, bound)
    print(f"OBS engine-vs-oracle trajectories: worst {worst:.3f} of the bound")
    # the skipped step moved neither parameter
    assert torch.equal(traj[SKIPPED], traj[SKIPPED - 1]) and not torch.equal(traj[SKIPPED + 1], traj[SKIPPED])
    live = [i for i in range(STEPS) if ref["losses"][i] is not None]
    assert np.isnan(res["losses"][SKIPPED]) and np.isnan(res["row_losses"][:, SKIPPED]).all() and ref["losses"][SKIPPED] is None
    want = np.array([ref["losses"][i] for i in live])
    assert np.abs(res["losses"][live] - want).max() < 1e-3 * np.abs(want).max()
    for b in range(2):
        want_b = np.array([ref["row_losses"][b][i] for i in live])
        assert np.abs(res["row_losses"][b][live] - want_b).max() < 1e-3 * np.abs(want_b).max(), b
    assert res["best_step"] == ref["best_step"]
    assert abs(res["best_loss"] - ref["best_loss"]) < 1e-3 * abs(ref["best_loss"]) and res["best_loss"] == res["losses"][res["best_step"]]
    assert tuple(res["w_a"].shape) == (1, cfg.k, cfg.z_dim) and tuple(res["w_b"].shape) == (1, cfg.k, cfg.z_dim)
    assert float((res["w_a"][0] - ref["best_a"]).abs().max()) < 0.05 * args.lr * STEPS
    assert float((res["w_b"][0] - ref["best_b"]).abs().max()) < 0.05 * args.lr * STEPS


def test_demorph_graph_and_eager_give_the_same_trajectory(tiny):
    G, cfg = tiny
    runs = []
    for use_graph in (True, False):
        eng = _engine(G, "mse", 0.3, use_graph)
        runs.append((_run(eng), eng.result()))
    for i in range(STEPS):
        assert torch.equal(runs[0][0][i], runs[1][0][i]), i
    a, b = runs[0][1], runs[1][1]
    assert a["best_step"] == b["best_step"] and np.array_equal(a["losses"], b["losses"], equal_nan=True)
    assert np.array_equal(a["row_losses"], b["row_losses"], equal_nan=True) and torch.equal(a["w_b"], b["w_b"]) and torch.equal(a["w_a"], b["w_a"])


@pytest.mark.parametrize("objective", ["mse", "lpips"])
def test_coupling_is_transparent_at_alpha_one(tiny, objective):
    """alpha = 1, row_weight (1, 1): the rows are [p_B, p_A], uncoupled -- 0 * x + y and, in the float64 transposed mix, 0 * g + 1 * h are exact.
    Both parameters' trajectories equal, bit for bit, `latent_in` of a plain lockstep GradientProjectionEngine on targets [morph, reference]
    started at [p_B, p_A] with the eps rows swapped to match."""
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine
    G, cfg = tiny
    c = _inputs()
    kw = dict(percept=PerceptualLoss(net="squeeze", allow_random_backbone=True)) if objective == "lpips" else {}
    plain = GradientProjectionEngine(G, torch.cat([c["morph"], c["reference"]]).cuda(), torch.stack([c["start_b"], c["start_a"]]).cuda(), 1.0, _args(),
                                     eps=c["eps"][:, [1, 0]].contiguous().cuda(), noise_mode="const", use_graph=True, **kw)
    want = _run(plain)
    kw = dict(percept=PerceptualLoss(net="squeeze", allow_random_backbone=True)) if objective == "lpips" else {}
    eng = _engine(G, "mse", 1.0, True, lm_valid=None, adam_eps=1e-8, **kw)
    got = _run(eng)
    assert not torch.equal(want[-1][0], c["start_b"]) and not torch.equal(want[-1][1], c["start_a"])
    for i in range(STEPS):
        assert torch.equal(got[i][1], want[i][0]) and torch.equal(got[i][0], want[i][1]), i
    # the plain engine's per-target totals are the rows' own
    assert np.array_equal(eng.result()["row_losses"], plain.result()[3])


def test_fixed_point(tiny):
    """Targets rendered by the engine's own generator from a known (z_A, z_B) -- unclamped, noise_mode="const", morph = G(blend) -- and a start at the
    truth with latent_std = 0: the first joint loss is two MSE rows of at most (1e-4 max|img|)^2 each, 1e-4 being the project's gate between
    two forward flavours of one image (tests/test_hip_noise_opt.py)."""
    from morphganformer_amd import drivers
    from morphganformer_amd.demorph import DemorphEngine
    from morphganformer_amd.projection import ProjectionArgs
    from morphganformer_amd.synth_weights import synthetic_latents
    G, cfg = tiny
    z = synthetic_latents(cfg, 2, 77)
    alpha = 0.3
    reference = G(torch.from_numpy(z[0:1]).cuda(), None, noise_mode="const")[0].clone()
    morph = G(torch.from_numpy(drivers._blend_latents(z[0:1], z[1:2], alpha)).cuda(), None, noise_mode="const")[0].clone()
    args = ProjectionArgs(step=2, lr=LR)
    eng = DemorphEngine(G, morph, reference, torch.from_numpy(z[0]).cuda(), torch.from_numpy(z[1]).cuda(), 0.0, args, alpha=alpha, noise_mode="const",
                        use_graph=False)
    eng.run(1)
    assert torch.equal(eng.rows[0].cpu(), torch.from_numpy(drivers._blend_latents(z[0], z[1], alpha))) and torch.equal(eng.rows[1].cpu(), torch.from_numpy(z[0]))
    first = float(eng.losses[0, 0])
    peak = float(torch.maximum(morph.abs().max(), reference.abs().max()))
    bound = args.beta * 2 * (1e-4 * peak) ** 2
    print(f"OBS fixed point: losses[0] {first:.3e}  bound {bound:.3e}")
    assert 0.0 <= first <= bound


def test_wplus_runs_and_moves_both_parameters(tiny):
    from morphganformer_amd.demorph import DemorphEngine
    from morphganformer_amd.projection import ProjectionArgs, mapping_only
    G, cfg = tiny
    c = _inputs()
    w = mapping_only(G, torch.stack([c["start_a"], c["start_b"]]).cuda())
    eng = DemorphEngine(G, c["morph"].cuda(), c["reference"].cuda(), w[0], w[1], 1.0, ProjectionArgs(step=4, lr=LR, lr_rampup=0.2), alpha=0.5,
                        noise_mode="const", latent_space="w+", seed=3)
    start = eng.latent_in.clone()
    res = eng.run().result()
    shape = (1, cfg.k, cfg.num_ws, cfg.w_dim)
    assert tuple(res["w_a"].shape) == shape and tuple(res["w_b"].shape) == shape
    assert np.isfinite(res["losses"]).all() and np.isfinite(res["row_losses"]).all() and res["losses"].shape == (4,) and res["row_losses"].shape == (2, 4)
    assert float((eng.latent_in[0] - start[0]).abs().max()) > 0.2 * LR and float((eng.latent_in[1] - start[1]).abs().max()) > 0.2 * LR
    assert tuple(eng.restored().shape) == (1, 3, cfg.img_resolution, cfg.img_resolution)


def test_refusals(tiny):
    from morphganformer_amd._lib import MgfError
    from morphganformer_amd.demorph import DemorphEngine
    from morphganformer_amd.projection import ProjectionArgs
    G, cfg = tiny
    c = _inputs()
    mk = lambda **kw: DemorphEngine(G, c["morph"].cuda(), c["reference"].cuda(), c["start_a"].cuda(), c["start_b"].cuda(), 1.0, ProjectionArgs(step=2),
                                    noise_mode="const", use_graph=False, **kw)
    for alpha in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match=r"alpha must lie in \(0, 1\]"):
            mk(alpha=alpha)
    with pytest.raises(MgfError, match="optimize_noise"):
        mk(optimize_noise=True)
    with pytest.raises(MgfError, match="mdf"):
        mk(mdf=object())
    with pytest.raises(MgfError, match="target_b"):
        mk(target_b=c["reference"].cuda())
    with pytest.raises(MgfError, match="landmark detectors"):
        mk(landmark_fn=lambda img: None)
    with pytest.raises(ValueError, match="row_weight"):
        mk(row_weight=(0.0, 1.0))
    with pytest.raises(MgfError, match="pool_above"):                      # what GradientProjectionEngine refuses stays refused
        DemorphEngine(G, c["morph"].cuda(), c["reference"].cuda(), c["start_a"].cuda(), c["start_b"].cuda(), 1.0, ProjectionArgs(step=2, pixel_term="psnr"))
    eng = mk()
    with pytest.raises(MgfError, match="not re-targeted"):
        eng.retarget(c["morph"].cuda())


def test_driver_writes_the_restored_latent_and_image(tiny, tmp_path):
    from morphganformer_amd import drivers
    from morphganformer_amd.demorph import DemorphEngine
    from morphganformer_amd.projection import ProjectionArgs
    G, cfg = tiny
    c = _inputs()
    args = ProjectionArgs(step=4, lr=LR, lr_rampup=0.2, n_mean_latent=200)
    morph, reference = c["morph"].cuda(), c["reference"].cuda()
    w_m, w_r = c["start_b"][None].numpy(), c["start_a"][None].numpy()
    for name, kw in (("given", dict(w_morph=w_m, w_ref=w_r, latent_std=1.0)), ("mean", {})):
        prefix = str(tmp_path / name / "case")
        res = drivers.demorph(G, morph, reference, alpha=0.3, args=args, seed=5, noise_mode="const", out_prefix=prefix, **kw)
        assert sorted(os.listdir(tmp_path / name)) == ["case_reference.mat", "case_restored.mat", "case_restored.png"]
        assert drivers.load_latent_mat(prefix + "_restored.mat").shape == (1, cfg.k, cfg.z_dim)
        assert np.array_equal(drivers.load_latent_mat(prefix + "_restored.mat"), res["w_b"].numpy())
        assert np.array_equal(drivers.load_latent_mat(prefix + "_reference.mat"), res["w_a"].numpy())
        assert res["w_start_b"].shape == (1, cfg.k, cfg.z_dim) and np.isfinite(res["losses"]).all() and res["row_losses"].shape == (2, 4)
        if name == "given":
            assert np.array_equal(res["w_start_b"], drivers.demorph_latent(w_m, w_r, 0.3))
    with pytest.raises(ValueError, match="come together"):
        drivers.demorph(G, morph, reference, w_morph=w_m, args=args)
    # restored() is render_latent of the best w_b
    eng = DemorphEngine(G, morph, reference, c["start_a"].cuda(), c["start_b"].cuda(), 1.0, args, alpha=0.3, noise_mode="const", seed=5).run()
    assert torch.equal(eng.restored(), drivers.render_latent(G, eng.result()["w_b"], noise_mode="const"))


def test_module_entry_on_a_tiny_snapshot(tmp_path):
    from morphganformer_amd import cli, demorph, drivers
    from morphganformer_amd.synth_weights import TINY
    from test_host_and_abi import _tiny_snapshot
    pkl = str(tmp_path / "net.pkl")
    _tiny_snapshot(pkl, seed=3)
    assert cli.main(["generate", "--model", pkl, "--output-dir", str(tmp_path / "g"), "--images-num", "2", "--seed", "1"]) == 0
    argv = ["--model", pkl, "--morph", str(tmp_path / "g" / "sample_000000.png"), "--reference", str(tmp_path / "g" / "sample_000001.png"),
            "--alpha", "0.4", "--out", str(tmp_path / "o" / "case"), "--size", "64", "--step", "4", "--n_mean_latent", "200", "--seed", "0", "--no-lpips"]
    assert demorph.main(argv) == 0
    assert sorted(os.listdir(tmp_path / "o")) == ["case_reference.mat", "case_restored.mat", "case_restored.png"]
    assert drivers.load_latent_mat(str(tmp_path / "o" / "case_restored.mat")).shape == (1, TINY.k, TINY.z_dim)
    with pytest.raises(SystemExit, match="come together"):
        demorph.main(argv + ["--w-morph", str(tmp_path / "o" / "case_restored.mat")])
    with pytest.raises(SystemExit, match="alpha"):
        demorph.main(argv + ["--alpha", "0"])


def test_default_engine_makes_none_of_the_new_calls(tiny, monkeypatch):
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    G, cfg = tiny
    c = _inputs()
    counts = _count_calls(monkeypatch, NEW_CALLS)
    for use_graph in (False, True):
        GradientProjectionEngine(G, c["morph"].cuda(), c["start_a"].cuda(), 1.0, ProjectionArgs(step=3, lr=LR), eps=c["eps"][:3, :1].contiguous().cuda(),
                                 noise_mode="const", use_graph=use_graph).run().result()
    assert counts == {n: 0 for n in NEW_CALLS}
    # ... and the counter does count: one de-morphing step makes exactly one call of each
    _engine(G, "mse", 0.5, False).run(1)
    assert counts == {n: 1 for n in NEW_CALLS}
