"""GPU tests of noise_mode="keyed": mgf_randn_keyed_f32 against its numpy restatement (tests/randn_keyed_numpy_ref.py) in guarded buffers,
and the mode through the generator, the three projection loops and the drivers -- TINY (64^2) throughout.  What the mode promises is that a
run does not depend on how its steps were launched: the loop tests compare results BITWISE across launch forms of one batch size."""
import numpy as np
import pytest
import torch

from guarded_buffers import Guarded
from randn_keyed_numpy_ref import map_normals, randn_keyed_ref

pytestmark = pytest.mark.gpu

MGF_EINVAL = -1                  # include/mgf.h
KEY = 0xC0FFEE0123456789         # (bit 63 set: the key travels as the int64 that holds these bits)
Z_TOL = 1e-5                     # |z - z_ref| absolute: logf, sqrtf and sincospif are a few float32 ulp each, |z| <= 6.7 -> ~1.6e-6; 6 x that
# The lockstep comparison of test_gradient_mode_*: measured under noise_mode="const" on this commit, the larger of the two rows' figures
# (max over the steps of |loss_lockstep - loss_single| / max |loss_single|: 3.594e-6 for target 0, 1.207e-6 for target 1) is LOCKSTEP_CONST;
# keyed mode is allowed twice that (it showed 1.230e-6 and 5.94e-7 in the same run).
LOCKSTEP_CONST = 3.594e-6
LOCKSTEP_TOL = 2 * LOCKSTEP_CONST


def _i64(key):
    v = int(key) & 0xFFFFFFFFFFFFFFFF
    return v - ((v >> 63) << 64)


def _key(key):
    return torch.tensor([_i64(key)], dtype=torch.int64, device="cuda")


def _call(out, sides, n, key, step, stride=0, add=1, smax=2 ** 31 - 1, aux0=1, aux_add=0, n_layers=None):
    from morphganformer_amd import _lib
    ptr = lambda t: 0 if t is None else (t.ptr() if isinstance(t, Guarded) else (t if isinstance(t, int) else t.data_ptr()))
    arr = None if sides is None else (_lib.i32 * len(sides))(*sides)
    rc = _lib.lib().mgf_randn_keyed_f32(ptr(out), arr, len(sides) if n_layers is None else n_layers, n, ptr(key), ptr(step), stride, add, smax,
                                        aux0, aux_add, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


# ----------------------------------------------------------------------------------------------------------------- the kernel
SIDES = [4, 8, 16]
PER = sum(s * s for s in SIDES)


@pytest.mark.parametrize("n", [1, 3, 5])
def test_kernel_against_the_restatement(n):
    """Every element within Z_TOL of the float64 restatement for step_stride, step_add and aux_add in {0, 1} each, with a clamp that bites
    (step + j > step_max, or the counter itself above it), through the 16-byte stores and -- `out` offset by one float -- the scalar ones."""
    key = _key(KEY)
    worst = 0.0
    for first in (7, 12):
        steps = [first, 3, 9, 8, 20]
        step = torch.tensor(steps, dtype=torch.int32, device="cuda")
        for stride in (0, 1):
            for add in (0, 1):
                for aux_add in (0, 1):
                    ref = randn_keyed_ref(SIDES, n, KEY, steps, stride, add, 8, 2, aux_add)
                    outs = []
                    for offset in (0, 1):
                        out = Guarded((n * PER,), None, offset=offset)
                        assert (out.ptr() % 16 == 0) == (offset == 0)
                        assert _call(out, SIDES, n, key, step, stride, add, 8, 2, aux_add) == 0
                        assert out.written() and out.guard_intact() and bool(torch.isnan(out.buf[:offset]).all())
                        got = out.numpy()
                        err = float(np.abs(got - ref).max())
                        worst = max(worst, err)
                        assert err <= Z_TOL, (first, stride, add, aux_add, offset, err)
                        outs.append(got)
                    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))       # the two store paths write the same numbers
    print(f"n = {n}: largest |z - z_ref| {worst:.3e}")
    # the clamp really bit somewhere, and the counters really differ between the samples
    if n >= 3:
        a = randn_keyed_ref(SIDES, n, KEY, [7], 0, 1, 8)
        assert np.array_equal(a[2 * 16:3 * 16], a[16:2 * 16]) and not np.array_equal(a[:16], a[16:32])


def test_sample_independence_repeats_and_refusals():
    from morphganformer_amd import _lib
    n, s = 4, 11
    key, step = _key(KEY), torch.tensor([s], dtype=torch.int32, device="cuda")
    out = Guarded((n * PER,), None)
    assert _call(out, SIDES, n, key, step) == 0
    batch = out.numpy().copy()
    # sample j of a call at step s = sample 0 of a call at step s + j, to the bit
    ones = []
    for j in range(n):
        one = Guarded((PER,), None)
        assert _call(one, SIDES, 1, key, torch.tensor([s + j], dtype=torch.int32, device="cuda")) == 0
        ones.append(one.numpy().copy())
    lo = 0
    for side in SIDES:
        for j in range(n):
            got = batch[n * lo + j * side * side:n * lo + (j + 1) * side * side]
            assert np.array_equal(got.view(np.uint32), ones[j][lo:lo + side * side].view(np.uint32)), (side, j)
        lo += side * side
    assert not np.array_equal(ones[0], ones[1])
    again = Guarded((n * PER,), None)
    assert _call(again, SIDES, n, key, step) == 0 and np.array_equal(again.numpy().view(np.uint32), batch.view(np.uint32))
    other = Guarded((n * PER,), None)
    assert _call(other, SIDES, n, _key(KEY + 1), step) == 0 and not np.array_equal(other.numpy(), batch)
    assert abs(float(np.corrcoef(other.numpy(), batch)[0, 1])) < 0.2
    # refusals: MGF_EINVAL, nothing written, the message names the entry point
    two = torch.zeros(2, dtype=torch.int64, device="cuda")
    ok = dict(out=None, sides=SIDES, n=n, key=key, step=step)
    bad = [dict(out=0), dict(sides=None, n_layers=3), dict(key=None), dict(step=None), dict(n=0), dict(n_layers=0), dict(smax=-1), dict(stride=-1),
           dict(aux0=0), dict(sides=[4, 5, 16]), dict(sides=[4, 0, 16]), dict(key=two.data_ptr() + 4)]
    for change in bad:
        victim = Guarded((n * PER,), None)
        args = dict(ok, out=victim)
        args.update(change)
        rc = _call(**args)
        assert rc == MGF_EINVAL, change
        assert "randn_keyed" in _lib.lib().mgf_last_error().decode(), change
        assert bool(torch.isnan(victim.buf).all()), change


# ----------------------------------------------------------------------------------------------------------------- the generator
def _tiny_G(max_batch=1, seed=0):
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import TINY, make_state_dict
    return Generator(make_state_dict(TINY, seed=seed), TINY, "cuda", max_batch=max_batch)


def test_generator_keyed_mode():
    from morphganformer_amd._lib import MgfError
    from morphganformer_amd.synth_weights import TINY, synthetic_latents
    G = _tiny_G(2)
    z = torch.from_numpy(synthetic_latents(TINY, 2, seed=5)).cuda()
    img = lambda **kw: G(z, None, **kw)[0]
    a = img(noise_mode="keyed", noise_key=KEY, noise_step=3)
    # the maps the layers read are the restated stream's: layer index = position among the layers that add noise, sample j at step 3 + j
    names = [lp.name for lp in G.plan.layers if lp.noise_strength is not None]
    assert G.last_noise[0] == "keyed" and list(G.last_noise[1]) == names
    for l, lp in enumerate(l for l in G.plan.layers if l.noise_strength is not None):
        got = G.last_noise[1][lp.name].cpu().numpy()
        for j in range(2):
            assert np.abs(got[j] - map_normals(lp.res, l, 3 + j, 1, KEY)).max() <= Z_TOL, (lp.name, j)
    b = img(noise_mode="keyed", noise_key=_key(KEY), noise_step=torch.tensor([3], dtype=torch.int32, device="cuda"))       # device words: the same
    assert torch.equal(a, b) and torch.equal(a, img(noise_mode="keyed", noise_key=KEY, noise_step=3))
    assert not torch.equal(a, img(noise_mode="keyed", noise_key=KEY, noise_step=4))
    assert not torch.equal(a, img(noise_mode="keyed", noise_key=KEY + 1, noise_step=3))
    assert not torch.equal(a, img(noise_mode="const"))
    # sample 1 at step 3 (+ 1 per sample) is sample 0 of a call at step 4 (the same maps; the image to the batch-position bound of
    # tests/test_hip_generator.py::test_full_1024_bench_batch_equals_batch1)
    c = G(z.flip(0).contiguous(), None, noise_mode="keyed", noise_key=KEY, noise_step=4)[0]
    assert float((a[1] - c[0]).abs().max()) <= 3e-5 * float(a[1].abs().max())
    assert float((a[1] - c[1]).abs().max()) > 1e-3 * float(a[1].abs().max())
    # the keyed path touches no random-mode state: a keyed call between two random draws changes neither
    torch.manual_seed(11)
    r1, r2 = img(noise_mode="random"), img(noise_mode="random")
    assert not torch.equal(r1, r2)
    torch.manual_seed(11)
    q1 = img(noise_mode="random")
    img(noise_mode="keyed", noise_key=KEY, noise_step=9)
    q2 = img(noise_mode="random")
    assert torch.equal(r1, q1) and torch.equal(r2, q2)
    for kw in (dict(noise_key=KEY), dict(noise_step=3), {}):
        with pytest.raises(MgfError, match="keyed"):
            img(noise_mode="keyed", **kw)
        with pytest.raises(MgfError, match="keyed"):
            G.synthesis(G._mapping_into(z), noise_mode="keyed", **kw)


# ----------------------------------------------------------------------------------------------------------------- the literal loop
STEPS, BATCH = 50, 4             # 13 launch sequences, the last one ragged (two of its four candidates lie past the final step)


def _loop_inputs(golden):
    g = golden("loop_tiny.npz")
    assert g["eps"].shape[0] == STEPS and g["lm_steps"].shape[0] == STEPS
    return g


def _literal(G, g, noise_mode, batch=BATCH, seed=7, **kw):
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine
    return ProjectionEngine(G, torch.from_numpy(g["target"]).cuda(), torch.from_numpy(g["latent_mean"]).cuda(), float(g["latent_std"]),
                            ProjectionArgs(step=STEPS), use_mse=True, lm_target=g["lm_target"], lm_steps=g["lm_steps"],
                            eps=torch.from_numpy(g["eps"]).cuda(), noise_mode=noise_mode, seed=seed, batch=batch, **kw)


def _same(a, b):
    return torch.equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64))


def test_literal_loop_is_bitwise_independent_of_the_launch_form(golden):
    """MSE + a Wing table, 50 steps in batches of 4.  Keyed mode: (best latent, best step, best loss, loss history) is bit-identical between the
    plain engine eager and replayed, the pipelined engine eager and replayed (each split over two run() calls), after rewind(), and after
    retarget() to another target and back.  Control: in random mode the plain and the pipelined engine do NOT agree."""
    from morphganformer_amd.projection import synthetic_landmarks
    g = _loop_inputs(golden)
    G = _tiny_G(BATCH)
    want = _literal(G, g, "keyed", use_graph=False).run().result()
    assert 0 <= want[1] < STEPS and not np.isnan(want[3]).any()
    other_target = torch.from_numpy(g["target"]).cuda().flip(3).contiguous()
    lm2 = synthetic_landmarks(STEPS, 64, 31)
    back = dict(lm_target=g["lm_target"], lm_steps=g["lm_steps"], eps=torch.from_numpy(g["eps"]).cuda(), seed=7)
    for pipeline in (False, True):
        for use_graph in (False, True):
            eng = _literal(G, g, "keyed", use_graph=use_graph, pipeline=pipeline)
            got = (eng.run(24).run() if pipeline else eng.run()).result()
            assert _same(got, want), (pipeline, use_graph)
            if pipeline:
                assert (eng.graphs[0] is not None) == use_graph and eng.pipeline
            if not use_graph:
                continue
            assert _same(eng.rewind().run().result(), want), ("rewind", pipeline)
            away = eng.retarget(other_target, lm_target=lm2[0], lm_steps=lm2[1], seed=8).run().result()
            assert not np.array_equal(away[3], want[3])
            assert int(eng.noise_key.item()) == 8
            assert _same(eng.retarget(torch.from_numpy(g["target"]).cuda(), **back).run().result(), want), ("retarget", pipeline)
    # another key, other noise: the history moves
    assert not np.array_equal(_literal(G, g, "keyed", seed=8, use_graph=True).run().result()[3], want[3])
    # control: the same comparison in random mode is not an equality (the draws follow the launch order)
    rnd = []
    for pipeline in (False, True):
        torch.manual_seed(3)
        rnd.append(_literal(G, g, "random", use_graph=True, pipeline=pipeline).run().result())
    assert not np.array_equal(rnd[0][3], rnd[1][3])


def test_literal_loop_across_batch_sizes(golden):
    """Batch 1 and batch 4 take different convolution kernels: the same best step, the losses within the 1e-3 tests/test_hip_evolution.py holds
    losses to."""
    g = _loop_inputs(golden)
    one = _literal(_tiny_G(1), g, "keyed", batch=1).run().result()
    four = _literal(_tiny_G(BATCH), g, "keyed", batch=BATCH).run().result()
    err = float(np.abs(one[3] - four[3]).max())
    print(f"batch 1 vs batch 4: best steps {one[1]} / {four[1]}, largest loss difference {err:.3e} of {np.abs(one[3]).max():.3f}")
    assert one[1] == four[1]
    assert err <= 1e-3 * float(np.abs(one[3]).max())


# ----------------------------------------------------------------------------------------------------------------- gradient mode
GSTEPS = 6


def _gradient_inputs():
    from morphganformer_amd.synth_weights import TINY
    gen = torch.Generator(device="cuda").manual_seed(23)
    mean = torch.randn(TINY.k, TINY.z_dim, device="cuda", generator=gen)
    eps = torch.randn(GSTEPS, 2, TINY.k, TINY.z_dim, device="cuda", generator=gen)
    near = mean[None] + 0.3 * torch.randn(2, TINY.k, TINY.z_dim, device="cuda", generator=gen)
    return mean, eps, near


def _gradient(G, targets, mean, eps, noise_mode, use_graph):
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    # the drivers' own optimizer settings (ProjectionArgs' defaults: lr 0.01 and its ramps)
    return GradientProjectionEngine(G, targets, mean, 1.0, ProjectionArgs(step=GSTEPS), percept=None, use_mse=True, eps=eps,
                                    noise_mode=noise_mode, seed=5, use_graph=use_graph)


def _lockstep_figures(G, targets, mean, eps, noise_mode):
    """Per row t: max over the steps of |loss of row t of the two-target engine - loss of a one-target engine on target t| / max |the latter|."""
    multi = _gradient(G, targets, mean, eps, noise_mode, True).run().result()[3]
    out = []
    for t in range(2):
        single = _gradient(G, targets[t:t + 1].contiguous(), mean, eps[:, t:t + 1].contiguous(), noise_mode, True).run().result()[3]
        out.append(float(np.abs(multi[t] - single).max() / np.abs(single).max()))
    return out


def test_gradient_mode_replays_and_lockstep_rows_equal_single_targets():
    """MSE only, 6 steps.  Eager equals graph replay bitwise; a second run after rewind() is bit-identical (rewind() leaves the latent and its
    Adam moments where the descent stands, by design, so the test puts those back on their start as well: what is compared is the noise);
    row t of a two-target lockstep engine matches a one-target engine on target t with the same seed within LOCKSTEP_TOL = 2 x 3.594e-6, the
    larger of the two rows' figures of the SAME comparison under noise_mode="const", measured on this commit (3.594e-6 and 1.207e-6; keyed:
    1.230e-6 and 5.94e-7; both pairs are printed below).  The two forwards take different kernels (batch 2 against batch 1) and the runs are
    free, not teacher-forced: the figures are float32 rounding carried through six Adam steps with the drivers' own optimizer settings."""
    G = _tiny_G(2)
    mean, eps, near = _gradient_inputs()
    targets = G(near, None, noise_mode="const")[0].clamp(-1, 1).clone()
    one, eps1 = targets[:1].contiguous(), eps[:, :1].contiguous()
    runs = {}
    for use_graph in (False, True):
        eng = _gradient(G, one, mean, eps1, "keyed", use_graph)
        start = [t.clone() for t in (eng.latent_in, eng.exp_avg, eng.exp_avg_sq, eng.adam_t)]
        runs[use_graph] = eng.run().result()
        assert (eng.graph is not None) == use_graph
        eng.rewind()
        for dst, src in zip((eng.latent_in, eng.exp_avg, eng.exp_avg_sq, eng.adam_t), start):
            dst.copy_(src)
        assert _same(eng.run().result(), runs[use_graph]), use_graph
    assert _same(runs[False], runs[True])
    assert not np.array_equal(_gradient(G, one, mean, eps1, "const", True).run().result()[3], runs[True][3])       # the noise really is in the loss
    const = _lockstep_figures(G, targets, mean, eps, "const")
    keyed = _lockstep_figures(G, targets, mean, eps, "keyed")
    print(f"lockstep rows vs single targets: const {const}, keyed {keyed}")
    assert max(keyed) <= LOCKSTEP_TOL, (keyed, const)


# ----------------------------------------------------------------------------------------------------------------- evolution mode
def test_evolution_engine_repeats_bitwise(golden):
    from morphganformer_amd.evolution import EvolutionProjectionEngine
    from morphganformer_amd.projection import ProjectionArgs
    g = _loop_inputs(golden)
    G = _tiny_G(8)
    steps = 20                                                  # generations of 8: the last one is ragged

    def state(eng):
        torch.cuda.synchronize()
        return [t.cpu().clone() for t in (eng.latent_in, eng.best_latent, eng.losses, eng.used, eng.min_loss, eng.best_step, eng.step_ctr)]

    same = lambda a, b: all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))
    runs = {}
    for use_graph in (False, True):
        eng = EvolutionProjectionEngine(G, torch.from_numpy(g["target"]).cuda(), torch.from_numpy(g["latent_mean"]).cuda(), 23.3,
                                        ProjectionArgs(step=steps), eps=torch.from_numpy(g["eps"][:steps]).cuda(), noise_mode="keyed", seed=3,
                                        batch=8, elite=3, mean_lr=0.5, use_graph=use_graph)
        runs[use_graph] = state(eng.run())
        assert (eng.graph is not None) == use_graph and int(runs[use_graph][6]) == steps
        assert same(state(eng.rewind().run()), runs[use_graph])
    assert same(runs[False], runs[True])
    assert not torch.equal(runs[True][0], torch.from_numpy(g["latent_mean"])[None])       # the mean moved


# ----------------------------------------------------------------------------------------------------------------- the drivers
def test_project_image_returns_the_key_and_the_best_image_renders_again(golden, tmp_path):
    """The trail image of the best step -- the image the loop scored -- against render_latent under that step's keyed noise: within 3e-5 of
    max|img|, the bound tests/test_hip_generator.py::test_full_1024_bench_batch_equals_batch1 holds batch-versus-batch-1 dispatch to."""
    from PIL import Image
    from morphganformer_amd import drivers
    from morphganformer_amd.projection import ProjectionArgs
    g = _loop_inputs(golden)
    G = _tiny_G(BATCH)
    res = drivers.project_image(G, torch.from_numpy(g["target"]).cuda(), g["lm_target"], g["lm_steps"], args=ProjectionArgs(step=STEPS),
                                latent_mean=torch.from_numpy(g["latent_mean"]).cuda(), latent_std=float(g["latent_std"]), seed=12, batch=BATCH,
                                noise_mode="keyed", path_to_gen=str(tmp_path / "trail"), out_prefix=str(tmp_path / "face"), return_engine=True)
    assert res["noise_key"] == 12 and res["step"] >= 0
    step, loss, scored = res["engine"].improvements()[-1]
    assert step == res["step"] and loss == res["loss"]
    again = drivers.render_latent(G, res["w"], noise_mode="keyed", noise_key=res["noise_key"], noise_step=res["step"])
    top = float(scored.abs().max())
    err = float((again[0] - scored.cuda()).abs().max()) / top
    const = float((drivers.render_latent(G, res["w"], noise_mode="const")[0] - scored.cuda()).abs().max()) / top
    print(f"re-rendered best image: {err:.3e} of max|img| from the scored one (constant noise: {const:.3e})")
    assert err <= 3e-5
    assert const > 100 * 3e-5                                  # the check can fail: constant noise is not the scored image
    # without a trail the final PNG is that image too
    res2 = drivers.project_image(G, torch.from_numpy(g["target"]).cuda(), g["lm_target"], g["lm_steps"], args=ProjectionArgs(step=STEPS),
                                 latent_mean=torch.from_numpy(g["latent_mean"]).cuda(), latent_std=float(g["latent_std"]), seed=12, batch=BATCH,
                                 noise_mode="keyed", out_prefix=str(tmp_path / "solo"))
    assert res2["step"] == res["step"] and torch.equal(res2["w"], res["w"]) and res2["noise_key"] == 12
    png = np.asarray(Image.open(res2["image"])).astype(np.int32)
    want = np.rint(again[0].cpu().numpy().transpose(1, 2, 0) * 127.5 + 127.5).clip(0, 255).astype(np.int32)
    assert png.shape == want.shape and np.abs(png - want).max() <= 1
