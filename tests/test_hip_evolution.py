"""GPU tests of the evolution-strategy mode: mgf_es_recombine_f32 bit for bit against its numpy restatement (tests/evolution_numpy_ref.py) in
guarded buffers, and EvolutionProjectionEngine against the restated loop on the CPU oracle -- TINY (64^2) throughout."""
import os

import numpy as np
import pytest
import torch

from evolution_numpy_ref import elite_order, es_loop_ref, es_recombine_ref, log_weights, top_gaps
from guarded_buffers import Guarded

pytestmark = pytest.mark.gpu

MGF_EINVAL = -1                  # include/mgf.h
STD = 23.3                       # the latent_std of every loop here: sigma_0 = 1.165, a search that really moves
RANK_MARGIN = 1e-2               # least relative gap between the totals a ranking decides between: 10 x the 1e-3 the losses are held to


# ----------------------------------------------------------------------------------------------------------------- the kernel
def _call(mean, cand, totals, step0, weights, mu, batch, steps_total, numel, lr, used):
    from morphganformer_amd import _lib
    ptr = lambda t: 0 if t is None else (t.ptr() if isinstance(t, Guarded) else t.data_ptr())
    rc = _lib.lib().mgf_es_recombine_f32(ptr(mean), ptr(cand), ptr(totals), ptr(step0), ptr(weights), mu, batch, steps_total, numel, lr, ptr(used),
                                         _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


class _Case:
    """One generation in guarded buffers: `mean` and `used` are outputs (NaN guards behind them, and `used` sits behind a NaN head too), `cand`
    an operand at the head of a NaN-filled allocation; `totals` is the whole loss table."""

    def __init__(self, batch, numel, totals, seed=0):
        rng = np.random.Generator(np.random.PCG64(seed))
        self.batch, self.numel, self.steps_total = batch, numel, len(totals)
        self.mean0 = rng.standard_normal(numel).astype(np.float32)
        self.cand0 = (rng.standard_normal((batch, numel)) * 3).astype(np.float32)
        self.totals0 = np.asarray(totals, dtype=np.float64)
        self.mean = Guarded((numel,), torch.from_numpy(self.mean0))
        self.cand = Guarded((batch, numel), torch.from_numpy(self.cand0))
        self.totals = torch.from_numpy(self.totals0).cuda()
        self.ngen = -(-self.steps_total // batch)
        self.used = Guarded((self.ngen,), None, offset=32)
        self.used.t.view(torch.int32).fill_(-7)
        self.step0 = torch.zeros(1, dtype=torch.int32, device="cuda")

    def used_now(self):
        return self.used.t.view(torch.int32).cpu().numpy()

    def run(self, s0, weights, mu, lr=1.0, with_used=True):
        """Launch on a fresh copy of the start mean; -> (rc, mean after, used after)."""
        self.mean.t.copy_(torch.from_numpy(self.mean0))
        self.used.t.view(torch.int32).fill_(-7)
        self.step0.fill_(s0)
        w = torch.from_numpy(np.asarray(weights, dtype=np.float64)).cuda()
        rc = _call(self.mean, self.cand, self.totals, self.step0, w, mu, self.batch, self.steps_total, self.numel, lr, self.used if with_used else None)
        assert self.mean.guard_intact() and self.used.guard_intact() and bool(torch.isnan(self.used.buf[:32]).all()), "a write outside mean / used"
        assert torch.equal(self.cand.t.cpu(), torch.from_numpy(self.cand0)) and np.array_equal(self.totals.cpu().numpy(), self.totals0, equal_nan=True)
        return rc, self.mean.t.cpu().numpy(), self.used_now()

    def check(self, s0, weights, mu, lr=1.0):
        rc, got, used = self.run(s0, weights, mu, lr)
        want, m = es_recombine_ref(self.mean0, self.cand0, self.totals0, s0, weights, mu, self.batch, self.steps_total, lr)
        assert rc == 0
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (s0, mu, lr, np.abs(got - want).max())
        want_used = np.full(self.ngen, -7, np.int32)
        if m is not None:
            want_used[s0 // self.batch] = m
        assert np.array_equal(used, want_used), (used, want_used)
        return m


def _seeded_totals(batch, seed):
    """Three generations of totals; the middle one (s0 = batch) carries duplicated values (normals rounded to one decimal), and from five
    candidates up a NaN and a +inf row."""
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    t = np.round(rng.standard_normal(3 * batch), 1) if batch > 2 else np.array([9.0, 9.0, 0.5, 0.5, 1.0, 2.0])
    if batch >= 5:
        t[batch + 1] = np.nan
        t[2 * batch - 2] = np.inf
        t[batch + 2] = t[batch]                                 # a tie whatever the draw
    return t


@pytest.mark.parametrize("batch,numel,mu", [(2, 7, 1), (2, 544, 2), (5, 33, 3), (32, 544, 8), (64, 10336, 16), (256, 544, 64)])
def test_recombine_kernel_bit_exact(batch, numel, mu):
    c = _Case(batch, numel, _seeded_totals(batch, batch), seed=batch)
    mid = c.totals0[batch:2 * batch]
    fin = mid[np.isfinite(mid)]
    assert len(np.unique(fin)) < len(fin)                       # the generation really has a tie
    for weights in (log_weights(mu), np.full(mu, 1.0 / mu)):
        for lr in (1.0, 0.5):
            assert c.check(batch, weights, mu, lr) == min(mu, len(fin))
    assert c.check(0, log_weights(mu), mu) == mu or batch == 2
    # without the optional table the mean is the same and nothing else is written
    rc, got, used = c.run(batch, log_weights(mu), mu, 1.0, with_used=False)
    assert rc == 0 and (used == -7).all()
    assert np.array_equal(got, es_recombine_ref(c.mean0, c.cand0, c.totals0, batch, log_weights(mu), mu, batch, c.steps_total)[0])


def test_recombine_kernel_edge_generations():
    nan, inf = np.nan, np.inf
    #          generation 0: two valid           1: none valid            2: all valid, a tie          3: ragged (two steps)
    totals = [nan, 3.0, inf, 1.0, nan, nan,   nan, -inf, inf, nan, nan, inf,   2.0, 1.0, 2.0, 1.0, 5.0, 0.5,   0.7, 0.2]
    c = _Case(6, 33, totals, seed=5)
    w = log_weights(4)
    assert c.check(0, w, 4) == 2                                # fewer valid candidates than mu: those two, the head of the weights renormalised
    rc, got, used = c.run(6, w, 4)
    assert rc == 0 and np.array_equal(got, c.mean0) and used.tolist() == [-7, 0, -7, -7]      # none valid: the mean stays, used = 0
    assert c.check(6, w, 4) == 0
    assert c.check(12, w, 4, 0.5) == 4
    assert list(elite_order(c.totals0, 12, 6, 20, 4)) == [5, 1, 3, 0]                          # ties to the smaller index
    assert c.check(18, w, 4) == 2                               # ragged last generation: s0 + batch > steps_total, only steps 18 and 19 count
    assert list(elite_order(c.totals0, 18, 6, 20, 4)) == [1, 0]
    for s0 in (20, 21, 1000, -1):                               # at or past the end: nothing is written, `used` included
        rc, got, used = c.run(s0, w, 4)
        assert rc == 0 and np.array_equal(got, c.mean0) and (used == -7).all(), s0
    assert c.check(7, w, 4) is not None                         # a step counter off the generation grid still stays inside both tables


def test_recombine_kernel_refusals():
    from morphganformer_amd import _lib
    c = _Case(4, 16, np.arange(8.0), seed=1)
    w = torch.from_numpy(log_weights(4)).cuda()
    ok = dict(mean=c.mean, cand=c.cand, totals=c.totals, step0=c.step0, weights=w, mu=2, batch=4, steps_total=8, numel=16, lr=1.0, used=c.used)
    overlap = c.cand.t[1]                                       # a `mean` inside `cand`
    bad = [dict(mean=None), dict(cand=None), dict(totals=None), dict(step0=None), dict(weights=None), dict(mu=0), dict(mu=5), dict(numel=0),
           dict(steps_total=0), dict(batch=0), dict(batch=1025, mu=2), dict(mean=overlap), dict(mean=c.cand.t)]
    for change in bad:
        rc = _call(**dict(ok, **change))
        assert rc == MGF_EINVAL, change
        assert "es_recombine" in _lib.lib().mgf_last_error().decode()
        assert torch.equal(c.mean.t.cpu(), torch.from_numpy(c.mean0)) and torch.equal(c.cand.t.cpu(), torch.from_numpy(c.cand0)), change
        assert (c.used_now() == -7).all() and c.mean.guard_intact() and c.used.guard_intact()
    assert _call(**ok) == 0 and c.used_now().tolist() == [2, -7]


# ----------------------------------------------------------------------------------------------------------------- the engine
def _oracle():
    """(cfg, the CPU generator on candidates [n,k,D] numpy, the target image [1,3,64,64] cpu) -- built once, shared, never modified."""
    if not _oracle.__dict__:
        from morphganformer_amd.synth_weights import TINY, make_state_dict, synthetic_latents
        from oracle.generator_ref import generator_ref, to_torch_state
        sd = make_state_dict(TINY, seed=0)
        tsd = to_torch_state(sd)

        def gen(cand):
            with torch.no_grad():
                return generator_ref(tsd, torch.from_numpy(np.ascontiguousarray(cand)), TINY, "const")

        _oracle.v = (TINY, sd, gen, gen(synthetic_latents(TINY, 1, 1001)).clamp(-1, 1))
    return _oracle.v


def _tiny_G(batch):
    from morphganformer_amd.engine import Generator
    cfg, sd, _, _ = _oracle()
    return Generator(sd, cfg, "cuda", max_batch=batch)


def _draws(seed, steps):
    """latent_mean [k,D], then eps [steps,k,D]: float64 normals of PCG64(seed) rounded to float32."""
    cfg = _oracle()[0]
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal((cfg.k, cfg.z_dim)).astype(np.float32), rng.standard_normal((steps, cfg.k, cfg.z_dim)).astype(np.float32)


def _engine(kind, G, mean, eps, steps, batch, **kw):
    from morphganformer_amd.evolution import EvolutionProjectionEngine
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine
    args = kw.pop("args", None) or ProjectionArgs(step=steps)
    return (EvolutionProjectionEngine if kind == "evolution" else ProjectionEngine)(
        G, kw.pop("target", _oracle()[3]).cuda(), torch.from_numpy(mean).cuda(), STD, args, eps=torch.from_numpy(eps).cuda()[:, None],
        noise_mode="const", batch=batch, **kw)


def _follow(eng, ref, steps, batch, mu, weights, mean_lr=1.0):
    """Advance `eng` generation by generation beside the restated loop `ref`: the losses within 1e-3, in every generation with sigma > 0 the same
    elite (after the oracle's own totals have shown the margin for it), and the mean bit-equal to the numpy recombination of the engine's OWN
    candidates and losses."""
    for g, s0 in enumerate(range(0, steps, batch)):
        n = min(batch, steps - s0)
        before = eng.mean.cpu().numpy()[0]
        eng.run(n)
        torch.cuda.synchronize()
        cand, losses = eng.latent_n.cpu().numpy(), eng.losses.cpu().numpy()
        want, m = es_recombine_ref(before, cand, losses, s0, weights, mu, batch, steps, mean_lr)
        got = eng.mean.cpu().numpy()[0]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), g
        assert m == ref["used"][g] and eng.elite_used()[g] == m
        if ref["sigma"][s0] > 0:
            gaps = top_gaps(ref["losses"], s0, n, mu + 1)
            print("generation", g, "oracle gaps", gaps)
            assert (gaps >= RANK_MARGIN).all(), (g, gaps)       # a near-tie on the oracle would make the next line a coin toss: fail here, loudly
            assert list(s0 + elite_order(losses, s0, batch, steps, mu)) == list(ref["elites"][g]), g
        else:
            assert np.array_equal(got, cand[0]) and np.array_equal(cand[0], before)            # identical candidates: the mean is that candidate
    got, want = eng.losses.cpu().numpy(), ref["losses"]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    print("losses: largest relative difference", np.nanmax(np.abs(got - want) / np.abs(want)))
    assert np.nanmax(np.abs(got - want)) <= 1e-3 * np.nanmax(np.abs(want)), (got, want)


def test_engine_follows_the_restated_loop():
    """LPIPS(squeeze, random backbone) + MSE, 40 steps in generations of 8, mu = 2, PCG64 seed 4."""
    from morphganformer_amd.lpips import PerceptualLoss, random_squeeze_backbone
    from oracle.loss_ref import lpips_ref, mse_ref, squeeze_backbone_random
    cfg, _, gen, tgt = _oracle()
    steps, batch, mu = 40, 8, 2
    mean, eps = _draws(4, steps)
    P = PerceptualLoss(net="squeeze", backbone_state=random_squeeze_backbone(0))
    bb, lins = squeeze_backbone_random(0), [l.cpu() for l in P.lins]
    with torch.no_grad():
        ref = es_loop_ref(gen, lambda i, img: float(lpips_ref(bb, lins, img, tgt)) + float(mse_ref(img, tgt)), mean, STD, eps, steps, batch, mu)
    assert int((ref["sigma"] > 0).sum()) == 30 and (ref["used"] == mu).all()
    eng = _engine("evolution", _tiny_G(batch), mean, eps, steps, batch, percept=P, elite=mu)
    _follow(eng, ref, steps, batch, mu, log_weights(mu))
    lat, bstep, bloss, _ = eng.result()
    assert bstep == ref["best_step"] and np.array_equal(lat.numpy()[0], ref["best_latent"])
    assert abs(bloss - ref["best_loss"]) <= 1e-3 * ref["best_loss"]
    assert not np.array_equal(eng.mean.cpu().numpy()[0], mean)


def _state(eng):
    torch.cuda.synchronize()
    return [t.cpu().clone() for t in (eng.latent_in, eng.best_latent, eng.losses, eng.used, eng.min_loss, eng.best_step, eng.step_ctr)]


def _same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def test_graph_replay_equals_eager_and_rewind_repeats():
    steps, batch = 20, 8                                        # the last generation is ragged
    mean, eps = _draws(7, steps)
    G = _tiny_G(batch)
    runs = {}
    for use_graph in (False, True):
        eng = _engine("evolution", G, mean, eps, steps, batch, use_graph=use_graph, elite=3, mean_lr=0.5)
        runs[use_graph] = _state(eng.run())
        assert (eng.graph is not None) == use_graph
        assert runs[use_graph][3].tolist() == [3, 3, 3] and int(runs[use_graph][6]) == steps
        eng.rewind()
        torch.cuda.synchronize()
        assert np.array_equal(eng.mean.cpu().numpy()[0], mean) and eng.elite_used().tolist() == [0, 0, 0]
        assert _same(_state(eng.run()), runs[use_graph])        # a rewound engine repeats its run
    assert _same(runs[False], runs[True])
    assert not np.array_equal(runs[True][0].numpy()[0], mean)


def test_skipped_steps_never_steer_the_mean():
    """A Wing table whose `valid` is zero on the whole first generation and on part of the second."""
    from morphganformer_amd.projection import synthetic_landmarks
    steps, batch, mu = 24, 8, 4
    mean, eps = _draws(8, steps)
    lm_t, lm_s = synthetic_landmarks(steps, 64, 3)
    valid = np.ones(steps, np.int32)
    valid[:8] = 0
    valid[[8, 9, 11, 12, 14, 15]] = 0                           # generation 1 keeps steps 10 and 13: fewer than mu
    eng = _engine("evolution", _tiny_G(batch), mean, eps, steps, batch, lm_target=lm_t, lm_steps=lm_s, lm_valid=valid, elite=mu)
    eng.run(8)
    assert np.array_equal(eng.mean.cpu().numpy()[0], mean) and eng.elite_used().tolist() == [0, 0, 0]
    eng.run(8)
    cand, losses = eng.latent_n.cpu().numpy(), eng.losses.cpu().numpy()
    assert np.isnan(losses[:10]).all() and np.isfinite(losses[[10, 13]]).all() and np.isnan(losses[[11, 12, 14, 15]]).all()
    assert sorted(elite_order(losses, 8, batch, steps, mu)) == [2, 5]
    want, m = es_recombine_ref(mean, cand, losses, 8, log_weights(mu), mu, batch, steps)
    assert m == 2 and np.array_equal(eng.mean.cpu().numpy()[0], want)
    eng.run(8)
    assert eng.elite_used().tolist() == [0, 2, 4]


WINDOWS = 68                     # the toy detector: 68 fixed 16 x 16 windows, a landmark = the centroid of exp(gray) inside its window


def _toy_landmark_model(device):
    i = torch.arange(WINDOWS, device=device)
    oy, ox = (i * 11) % 48, (i * 7) % 48
    d = torch.arange(16, device=device)
    ys = (oy[:, None, None] + d[None, :, None]).expand(WINDOWS, 16, 16)
    xs = (ox[:, None, None] + d[None, None, :]).expand(WINDOWS, 16, 16)

    def model(img):
        w = torch.exp(img.double().mean(1))[:, ys, xs]                      # [B,68,16,16], smooth in the image and > 0
        tot = w.sum((-1, -2))
        lm = torch.stack([(w * xs).sum((-1, -2)) / tot, (w * ys).sum((-1, -2)) / tot], -1)
        return lm, torch.ones(img.shape[0], dtype=torch.int32, device=img.device)
    return model


TOY_SEED = 37                    # chosen on the CPU oracle among seeds 10..69: the three best Wing values of its four moving generations lie
                                 # 1.5e-2 / 4.2e-2 / 2.0e-2 / 1.9e-2 apart (relative), best loss 0.01608 against the fixed mean's 0.01864


def test_detector_driven_objective():
    """Wing on a device landmark model's output is the whole objective: no term of it has a backward pass, and the mean still follows it."""
    from oracle.loss_ref import wing_loss_ref
    cfg, _, gen, tgt = _oracle()
    steps, batch, mu = 40, 8, 2
    mean, eps = _draws(TOY_SEED, steps)
    cpu_model = _toy_landmark_model("cpu")
    lm_t = cpu_model(tgt)[0][0]
    ref = es_loop_ref(gen, lambda i, img: 0.01 * float(wing_loss_ref(cpu_model(img)[0][0], lm_t)), mean, STD, eps, steps, batch, mu)
    G = _tiny_G(batch)
    kw = dict(use_mse=False, lm_target=lm_t.numpy(), landmark_model=_toy_landmark_model("cuda"))
    eng = _engine("evolution", G, mean, eps, steps, batch, elite=mu, **kw)
    _follow(eng, ref, steps, batch, mu, log_weights(mu))
    _, bstep, bloss, _ = eng.result()
    assert bstep == ref["best_step"] and abs(bloss - ref["best_loss"]) <= 1e-3 * ref["best_loss"]
    fixed = _engine("literal", G, mean, eps, steps, batch, **kw).run().result()
    print("Wing term of the best step: moving mean", bloss / 0.01, "fixed mean", fixed[2] / 0.01)
    assert bloss < fixed[2]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_moving_mean_beats_the_literal_loop(seed):
    """MSE only, 128 steps, 16 candidates per generation, mu = 4: the best loss is at most 0.75 x the literal engine's on the same mean, eps and
    target (CPU oracle: 0.560 / 0.587 / 0.551, tests/test_evolution_host.py; a mean that never moves gives 1.0)."""
    steps, batch = 128, 16
    mean, eps = _draws(seed, steps)
    G = _tiny_G(batch)
    lit = _engine("literal", G, mean, eps, steps, batch).run().result()
    evo = _engine("evolution", G, mean, eps, steps, batch, elite=4).run().result()
    print("seed", seed, "fixed", lit[2], "moving", evo[2], "ratio", evo[2] / lit[2])
    assert evo[2] <= 0.75 * lit[2]


def test_one_elite_full_step_is_the_best_candidate():
    steps, batch = 16, 8
    mean, eps = _draws(9, steps)
    eng = _engine("evolution", _tiny_G(batch), mean, eps, steps, batch, elite=1, mean_lr=1.0)
    for s0 in (0, 8):
        eng.run(8)
        cand, losses = eng.latent_n.cpu().numpy(), eng.losses.cpu().numpy()
        j = int(np.argmin(losses[s0:s0 + 8]))
        assert np.array_equal(eng.mean.cpu().numpy()[0].view(np.uint32), cand[j].view(np.uint32))


def test_drivers_outputs_retargeting_and_module_entry(tmp_path):
    from morphganformer_amd import drivers, evolution
    from morphganformer_amd.projection import ProjectionArgs, synthetic_landmarks
    from morphganformer_amd.synth_weights import TINY, synthetic_latents
    steps, batch = 16, 4
    G = _tiny_G(batch)
    mean, _ = _draws(12, 1)
    mean = torch.from_numpy(mean).cuda()
    targets = [G(torch.from_numpy(synthetic_latents(TINY, 1, 3000 + j)).cuda(), None, noise_mode="const")[0].clamp(-1, 1).clone() for j in range(2)]
    lms = [synthetic_landmarks(steps, 64, 20 + j) for j in range(2)]
    kw = dict(args=ProjectionArgs(step=steps), latent_mean=mean, latent_std=STD, batch=batch, noise_mode="const", mode="evolution", elite=2,
              mean_lr=0.5, es_weights="equal")
    out = tmp_path / "trail"
    r = [drivers.project_image(G, targets[j], *lms[j], seed=50 + j, out_prefix=str(out / f"t{j}"), path_to_gen=str(out), **kw) for j in range(2)]
    files = sorted(os.listdir(out))
    assert "t0.mat" in files and "t1.mat" in files and "t0.png" not in files            # the trail stands for the rendering, as in literal mode
    assert all(len(q["images"]) >= 1 and all(os.path.dirname(p) == str(out) and os.path.exists(p) for p in q["images"]) for q in r)
    assert np.array_equal(drivers.load_latent_mat(str(out / "t0.mat")), r[0]["w"].numpy())
    assert tuple(r[0]["mean"].shape) == (1, TINY.k, TINY.z_dim) and r[0]["elite_used"].tolist() == [2, 2, 2, 2]
    assert not torch.equal(r[0]["mean"], mean.cpu()[None])
    # one engine walked over both targets equals the fresh ones bit for bit
    eng = None
    for j in range(2):
        q = drivers.project_image(G, targets[j], *lms[j], seed=50 + j, path_to_gen=str(tmp_path / "again"), engine=eng, return_engine=True, **kw)
        graph = eng.graph if eng is not None else None
        eng = q["engine"]
        assert graph is None or eng.graph is graph
        assert q["step"] == r[j]["step"] and q["loss"] == r[j]["loss"] and torch.equal(q["w"], r[j]["w"]) and torch.equal(q["mean"], r[j]["mean"])
        assert np.array_equal(q["losses"], r[j]["losses"]) and np.array_equal(q["elite_used"], r[j]["elite_used"])
    with pytest.raises(ValueError, match="another mode"):
        drivers.project_image(G, targets[0], *lms[0], engine=eng, **dict(kw, mode="literal"))
    with pytest.raises(ValueError, match="elite"):
        drivers.project_image(G, targets[0], *lms[0], engine=eng, path_to_gen=str(tmp_path / "again"), **dict(kw, elite=3))
    many = drivers.project_many(G, targets, landmarks=lms, seed=50, **kw)
    assert many["latents"].shape[0] == 2
    # the module entry, end to end on a seeded TINY pickle
    from PIL import Image
    from test_host_and_abi import _tiny_snapshot
    pkl = str(tmp_path / "net.pkl")
    _tiny_snapshot(pkl, seed=3)
    drivers.save_image(G, targets[0], str(tmp_path / "face.png"))
    assert Image.open(tmp_path / "face.png").size == (64, 64)
    np.savez(tmp_path / "lm.npz", target=lms[0][0], steps=lms[0][1])
    argv = ["--model", pkl, "--image", str(tmp_path / "face.png"), "--landmarks", str(tmp_path / "lm.npz"), "--path_to_gen", str(tmp_path / "cli"),
            "--size", "64", "--step", "16", "--n_mean_latent", "200", "--batch", "4", "--elite", "2", "--seed", "0"]
    with pytest.raises(SystemExit, match="lpips-backbone"):
        evolution.main(argv)
    assert evolution.main(argv + ["--lpips-random-backbone"]) == 0
    files = sorted(os.listdir(tmp_path / "cli"))
    assert "face.mat" in files and len([f for f in files if f.endswith(".png")]) >= 1


def test_refusals():
    from morphganformer_amd import drivers
    from morphganformer_amd._lib import MgfError
    from morphganformer_amd.projection import ProjectionArgs
    steps, batch = 8, 4
    mean, eps = _draws(13, steps)
    G = _tiny_G(batch)
    for kw, why in ((dict(pipeline=True), "pipeline"), (dict(args=ProjectionArgs(step=steps, latent_copies=2)), "latent_copies"),
                    (dict(batch=1), "batch"), (dict(elite=0), "elite"), (dict(elite=5), "elite"), (dict(mean_lr=0.0), "mean_lr"),
                    (dict(mean_lr=1.25), "mean_lr"), (dict(mean_lr=float("nan")), "mean_lr"), (dict(es_weights="rank"), "es_weights")):
        with pytest.raises(MgfError, match=why):
            _engine("evolution", G, mean, eps, steps, kw.pop("batch", batch), **kw)
    tgt = _oracle()[3].cuda()
    common = dict(args=ProjectionArgs(step=steps), latent_mean=torch.from_numpy(mean).cuda(), latent_std=STD, batch=batch, mode="evolution")
    with pytest.raises(ValueError, match="w\\+"):
        drivers.project_image(G, tgt, None, None, latent_space="w+", **common)
    with pytest.raises(MgfError, match="pipelined"):
        drivers.project_image(G, tgt, None, None, pipeline=True, **common)
