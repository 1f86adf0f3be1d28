"""PerceptualLoss(pool_above=32) inside the projection loops on the tiny 64^2 generator: gradient mode against torch
autograd + Adam through the CPU oracle with LPIPS at 32^2 beside MSE at 64^2 (the combination ProjectionArgs.pool_above cannot express), the
literal loop against the oracle's pooling + LPIPS, lockstep targets against single runs, graph replay against the eager loop, and the module
entry that has --lpips-pool-above.  No engine knows about the option: each gate is the one the un-pooled loop is held to in
tests/test_hip_gradient.py and tests/test_hip_projection.py."""
import os

import numpy as np
import pytest
import torch

from lpips_pool_torch_ref import block_mean_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.grad import GeneratorGrad
    from morphganformer_amd.synth_weights import TINY, make_state_dict
    from oracle.generator_ref import to_torch_state
    sd = make_state_dict(TINY, seed=0)
    G = Generator(sd, TINY, "cuda", max_batch=2)
    return GeneratorGrad(G), to_torch_state(sd), TINY


def _lins():
    from morphganformer_amd.lpips import WEIGHTS_DIR
    lin = np.load(os.path.join(WEIGHTS_DIR, "lpips_lin_squeeze.npz"))
    return [torch.from_numpy(lin[f"lin{i}"]).float().reshape(-1) for i in range(7)]


def _pooled_percept():
    from morphganformer_amd.lpips import PerceptualLoss
    return PerceptualLoss(net="squeeze", allow_random_backbone=True, pool_above=32)


@pytest.mark.parametrize("use_graph", [False, True])
def test_gradient_projection_with_pooled_lpips_matches_autograd_adam(tiny, use_graph):
    """The setup of test_gradient_projection_matches_autograd_adam -- 10 steps, lr 0.05, lr_rampup 0.2, step 3 skipped, PCG64(4) streams --
    with loss = lpips_ref(pool_2 img, pool_2 target) + lamda Wing + beta mse_ref(img, target); the same gates: losses 1e-3 relative,
    trajectory 0.05 lr (i + 1), the best step equal."""
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, synthetic_landmarks
    from morphganformer_amd.synth_weights import synthetic_latents
    from oracle.generator_ref import generator_ref
    from oracle.loss_ref import backbone_random, lpips_ref, mse_ref, projection_gradient_ref, wing_loss_ref
    gg, tsd, cfg = tiny
    steps = 10
    rng = np.random.Generator(np.random.PCG64(4))
    latent_mean = torch.from_numpy(rng.standard_normal((cfg.k, cfg.z_dim)).astype(np.float32))
    eps = torch.from_numpy(rng.standard_normal((steps, 1, cfg.k, cfg.z_dim)).astype(np.float32))
    target = generator_ref(tsd, torch.from_numpy(synthetic_latents(cfg, 1, 1001)), cfg, "const").clamp(-1, 1)
    lm_t, lm_s = synthetic_landmarks(steps, 64, 9)
    valid = np.ones(steps, np.int32)
    valid[3] = 0
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.2)
    bb, lins = backbone_random("squeeze", 0), _lins()
    pool = lambda t: block_mean_ref(t, 2).float()

    def loss_fn(i, img):
        if not valid[i]:
            return None
        w = wing_loss_ref(torch.from_numpy(lm_s[i]), torch.from_numpy(lm_t))
        return lpips_ref(bb, lins, pool(img), pool(target)).sum() + args.lamda * w + args.beta * mse_ref(img, target)

    ref = projection_gradient_ref(lambda z: generator_ref(tsd, z, cfg, "const"), loss_fn, latent_mean, 1.0, eps, steps, lr=args.lr,
                                  rampdown=args.lr_rampdown, rampup=args.lr_rampup)
    eng = GradientProjectionEngine(gg.G, target.cuda(), latent_mean.cuda(), 1.0, args, percept=_pooled_percept(), lm_target=lm_t, lm_steps=lm_s,
                                   lm_valid=valid, eps=eps.cuda(), noise_mode="const", use_graph=use_graph)
    traj = []
    for i in range(steps):
        eng.run(1)
        traj.append(eng.latent_in.cpu().clone())
    lat, bstep, bloss, losses = eng.result()
    moved = float((ref[4][-1] - latent_mean).abs().max())
    assert moved > 5 * args.lr * 0.2, "the oracle run must actually move the latent"
    for i in range(steps):
        assert float((traj[i] - ref[4][i]).abs().max()) < 0.05 * args.lr * (i + 1), i
    got = np.array([v for v in losses if not np.isnan(v)])
    want = np.array([v for v in ref[3] if v is not None])
    assert np.isnan(losses[3]) and ref[3][3] is None
    print(f"OBS pooled gradient loop use_graph={use_graph}: moved {moved:.3f}, losses rel {np.abs(got - want).max() / np.abs(want).max():.3e}, "
          f"best step {bstep} (oracle {ref[1]})")
    assert np.abs(got - want).max() < 1e-3 * np.abs(want).max()
    assert bstep == ref[1]
    assert float((lat - ref[0]).abs().max()) < 0.05 * args.lr * steps


def test_literal_loop_with_pooled_lpips(golden):
    """ProjectionEngine, LPIPS only, batch 4, the target at 64^2: every recorded loss against lpips_ref(pool_above_ref(oracle image, 32), pooled
    target) at the 1e-3 of test_v1_pooled_percept_objective; the pipelined loop gives the same bits."""
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine
    from morphganformer_amd.synth_weights import TINY, make_state_dict
    from oracle.generator_ref import generator_ref, to_torch_state
    from oracle.loss_ref import lpips_ref, pool_above_ref, squeeze_backbone_random
    g = golden("loop_tiny.npz")
    steps = 8
    sd = make_state_dict(TINY, seed=0)
    tsd = to_torch_state(sd)
    target = torch.from_numpy(g["target"])
    assert tuple(target.shape) == (1, 3, 64, 64)
    mk = lambda pipe: ProjectionEngine(Generator(sd, TINY, "cuda", max_batch=1), target.cuda(), torch.from_numpy(g["latent_mean"]).cuda(),
                                       float(g["latent_std"]), ProjectionArgs(step=steps), percept=_pooled_percept(), use_mse=False,
                                       eps=torch.from_numpy(g["eps"][:steps]).cuda(), noise_mode="const", batch=4, pipeline=pipe).run()
    eng = mk(False)
    lat, bstep, bloss, losses = eng.result()
    bb, lins = squeeze_backbone_random(0), _lins()
    pooled_target = torch.from_numpy(pool_above_ref(g["target"], 32).astype(np.float32))
    for i in range(steps):
        sigma = np.float32(np.float32(float(g["latent_std"])) * np.float32(0.05)) * np.float32(max(0, 1 - (i / steps) / 0.75) ** 2)
        z = torch.from_numpy(g["latent_mean"])[None] + torch.from_numpy(g["eps"][i]) * float(sigma)
        with torch.no_grad():
            img = torch.from_numpy(pool_above_ref(generator_ref(tsd, z, TINY, "const").numpy(), 32))
            want = float(lpips_ref(bb, lins, img, pooled_target).sum())
        assert abs(losses[i] - want) < 1e-3 * abs(want), (i, losses[i], want)
    assert bstep == int(np.argmin(losses))
    piped = mk(True)
    assert torch.equal(piped.losses, eng.losses) and torch.equal(piped.best_latent, eng.best_latent)


def test_lockstep_targets_with_pooled_lpips_equal_single_runs(tiny):
    """Two targets in one engine against two single-target engines, every percept with pool_above = 32: the lockstep gate of
    test_gradient_projection_lockstep_targets_equal_single_runs."""
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, synthetic_landmarks
    gg, tsd, cfg = tiny
    G = gg.G
    steps, B = 8, 2
    torch.manual_seed(21)
    latent_mean = torch.randn(cfg.k, cfg.z_dim, device="cuda")
    eps = torch.randn(steps, B, cfg.k, cfg.z_dim, device="cuda")
    targets = G(torch.randn(B, cfg.k, cfg.z_dim, device="cuda"), None, noise_mode="const")[0].clamp(-1, 1).clone()
    lms = [synthetic_landmarks(steps, 64, 9 + j) for j in range(B)]
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.25)
    singles = []
    for j in range(B):
        e = GradientProjectionEngine(G, targets[j:j + 1].contiguous(), latent_mean, 1.0, args, percept=_pooled_percept(), lm_target=lms[j][0],
                                     lm_steps=lms[j][1], eps=eps[:, j:j + 1].contiguous(), noise_mode="const", use_graph=False).run()
        singles.append((e.result(), e.latent_in.cpu().clone()))
    multi = GradientProjectionEngine(G, targets, latent_mean, 1.0, args, percept=_pooled_percept(), lm_target=np.stack([l[0] for l in lms]),
                                     lm_steps=np.stack([l[1] for l in lms]), eps=eps, noise_mode="const", use_graph=True).run()
    lat, bstep, bloss, losses = multi.result()
    assert sorted(multi.percept._pooled) == [(B, 64, 64)]
    for j in range(B):
        (slat, sstep, sloss, slosses), sfinal = singles[j]
        first = np.arange(steps) < 2
        assert np.abs(losses[j][first] - slosses[first]).max() < 1e-5 * np.abs(slosses).max()
        assert np.abs(losses[j] - slosses).max() < 5e-2 * np.abs(slosses).max()
        assert int(bstep[j]) == sstep
        assert float((multi.latent_in[j].cpu() - sfinal[0]).abs().max()) < 0.25 * args.lr * steps


def test_graph_replay_gives_the_eager_bits_and_allocates_nothing(tiny):
    """use_graph=True against use_graph=False: the same loss history bit for bit; torch.cuda.memory_allocated() does not grow between replay 2
    and replay 6 (the pooled-image buffers are allocated in the capture's warm-up)."""
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    gg, tsd, cfg = tiny
    G = gg.G
    steps = 8
    torch.manual_seed(5)
    latent_mean = torch.randn(cfg.k, cfg.z_dim, device="cuda")
    eps = torch.randn(steps, 1, cfg.k, cfg.z_dim, device="cuda")
    target = G(torch.randn(1, cfg.k, cfg.z_dim, device="cuda"), None, noise_mode="const")[0].clamp(-1, 1).clone()
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.25)
    mk = lambda use_graph: GradientProjectionEngine(G, target, latent_mean, 1.0, args, percept=_pooled_percept(), eps=eps, noise_mode="const",
                                                    use_graph=use_graph)
    eager = mk(False).run().result()[3]
    eng = mk(True)
    eng.run(2)
    torch.cuda.synchronize()
    after2 = torch.cuda.memory_allocated()
    pooled = {k: v.data_ptr() for k, v in eng.percept._pooled.items()}
    eng.run(4)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() <= after2
    assert {k: v.data_ptr() for k, v in eng.percept._pooled.items()} == pooled and sorted(pooled) == [(1, 64, 64)]
    losses = eng.run().result()[3]
    assert np.array_equal(losses, eager) and np.isfinite(losses).all()


def test_demorph_module_entry_with_the_flag(tmp_path, monkeypatch):
    """`python -m morphganformer_amd.demorph --lpips-pool-above 32` on a tiny snapshot (gradient mode): the term is built with the option,
    pools the engine's 64^2 images, and the run writes its files."""
    from morphganformer_amd import cli, demorph
    from test_host_and_abi import _tiny_snapshot
    pkl = str(tmp_path / "net.pkl")
    _tiny_snapshot(pkl, seed=3)
    assert cli.main(["generate", "--model", pkl, "--output-dir", str(tmp_path / "g"), "--images-num", "2", "--seed", "1"]) == 0
    made, build = [], cli._lpips_term
    monkeypatch.setattr(cli, "_lpips_term", lambda *a, **kw: made.append(build(*a, **kw)) or made[-1])
    argv = ["--model", pkl, "--morph", str(tmp_path / "g" / "sample_000000.png"), "--reference", str(tmp_path / "g" / "sample_000001.png"),
            "--alpha", "0.4", "--out", str(tmp_path / "o" / "case"), "--size", "64", "--step", "4", "--n_mean_latent", "200", "--seed", "0",
            "--lpips-random-backbone", "--lpips-pool-above", "32"]
    assert demorph.main(argv) == 0
    assert sorted(os.listdir(tmp_path / "o")) == ["case_reference.mat", "case_restored.mat", "case_restored.png"]
    assert len(made) == 1 and made[0].pool_above == 32
    assert made[0]._pooled and all(k[1:] == (64, 64) and tuple(v.shape[2:]) == (32, 32) for k, v in made[0]._pooled.items())
