"""Host checks of the evolution-strategy mode (no GPU): the recombination weights, the numpy restatements of tests/evolution_numpy_ref.py
against hand-computed cases and against the premise the mode was built on (a moving mean beats the fixed one on the CPU oracle), the module
entry's parser, and the library's declarations."""
import math
import os
import re

import numpy as np
import pytest
import torch

from evolution_numpy_ref import es_loop_ref, es_recombine_ref, log_weights, sigma_schedule


@pytest.mark.parametrize("mu", [1, 2, 4, 8, 64])
def test_recombination_weights_closed_form(mu):
    from morphganformer_amd._lib import MgfError
    from morphganformer_amd.evolution import recombination_weights
    raw = [math.log(mu + 0.5) - math.log(r) for r in range(1, mu + 1)]
    want = np.array([v / math.fsum(raw) for v in raw])
    w = recombination_weights(mu, "log")
    assert w.dtype == np.float64 and w.shape == (mu,)
    assert np.abs(w - want).max() <= 1e-15 and abs(math.fsum(w) - 1.0) <= 1e-15
    assert (w > 0).all() and (np.diff(w) < 0).all()                      # strictly decreasing, best candidate first
    assert np.array_equal(w, log_weights(mu))                             # the restatement the GPU tests use
    e = recombination_weights(mu, "equal")
    assert e.dtype == np.float64 and np.array_equal(e, np.full(mu, 1.0 / mu)) and abs(math.fsum(e) - 1.0) <= 1e-15
    with pytest.raises(MgfError, match="es_weights"):
        recombination_weights(mu, "rank")
    with pytest.raises(MgfError, match=">= 1"):
        recombination_weights(0)


def test_recombination_restatement_hand_cases():
    f32 = np.float32
    mean = np.array([1.0, -2.0, 0.5], f32)
    cand = np.array([[2.0, 0.0, 1.5], [4.0, 4.0, 4.0]], f32)
    # two candidates, mu = 1: the mean becomes the better one (candidate 1: 0.25 < 0.75)
    out, m = es_recombine_ref(mean, cand, [0.75, 0.25], 0, [1.0], 1, 2, 2)
    assert m == 1 and np.array_equal(out, cand[1])
    # a tie goes to the smaller index
    out, m = es_recombine_ref(mean, cand, [0.5, 0.5], 0, [1.0], 1, 2, 2)
    assert m == 1 and np.array_equal(out, cand[0])
    # ... and with both recombined, weights 3/4 and 1/4 in that order
    out, m = es_recombine_ref(mean, cand, [0.5, 0.5], 0, [0.75, 0.25], 2, 2, 2)
    assert m == 2 and np.array_equal(out, np.array([2.5, 1.0, 2.125], f32))
    # all totals invalid: the mean stays, nothing is recombined
    out, m = es_recombine_ref(mean, cand, [np.nan, np.inf], 0, [0.75, 0.25], 2, 2, 2)
    assert m == 0 and np.array_equal(out, mean)
    # one invalid: the valid one alone, its weight renormalised to 1 (-inf is no loss either)
    out, m = es_recombine_ref(mean, cand, [-np.inf, 7.0], 0, [0.75, 0.25], 2, 2, 2)
    assert m == 1 and np.array_equal(out, cand[1])
    # mean_lr = 0.5: half way to the recombined point
    out, m = es_recombine_ref(mean, cand, [0.75, 0.25], 0, [1.0], 1, 2, 2, mean_lr=0.5)
    assert m == 1 and np.array_equal(out, np.array([2.5, 1.0, 2.25], f32))
    # a generation in the middle of the table reads its own rows; a ragged last one only the steps that exist; past the end nothing happens
    totals = [9.0, 9.0, 0.75, 0.25, 0.1]
    assert np.array_equal(es_recombine_ref(mean, cand, totals, 2, [1.0], 1, 2, 5)[0], cand[1])
    out, m = es_recombine_ref(mean, cand, totals, 4, [1.0], 1, 2, 5)
    assert m == 1 and np.array_equal(out, cand[0])
    out, m = es_recombine_ref(mean, cand, totals, 5, [1.0], 1, 2, 5)
    assert m is None and np.array_equal(out, mean)


def test_sigma_restatement_is_the_drivers_schedule():
    from morphganformer_amd.projection import noise_schedule
    for steps, std in ((128, 23.3), (40, 23.3), (20, 1.0)):
        assert np.array_equal(sigma_schedule(steps, std), noise_schedule(steps, std, 0.05, 0.75))


# fixed-mean and moving-mean best loss of the loop on the CPU oracle: TINY, make_state_dict(TINY, 0), const noise, target = the image of
# synthetic_latents(TINY, 1, 1001) clamped, MSE only, 128 steps, 16 candidates per generation, mu = 4, log weights, latent_std 23.3,
# PCG64(seed) draws latent_mean then eps as float64 normals rounded to float32
CPU_TABLE = {1: (2.30116, 1.28845), 2: (1.40606, 0.82489), 3: (3.96339, 2.18393)}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_moving_mean_beats_fixed_mean_on_the_cpu_oracle(seed):
    from morphganformer_amd.synth_weights import TINY, make_state_dict, synthetic_latents
    from oracle.generator_ref import generator_ref, to_torch_state
    cfg = TINY
    tsd = to_torch_state(make_state_dict(cfg, seed=0))
    with torch.no_grad():
        tgt = generator_ref(tsd, torch.from_numpy(synthetic_latents(cfg, 1, 1001)), cfg, "const").clamp(-1, 1)

    def gen(cand):
        with torch.no_grad():
            return generator_ref(tsd, torch.from_numpy(cand), cfg, "const")

    loss = lambda i, img: float((img - tgt).square().mean())
    rng = np.random.Generator(np.random.PCG64(seed))
    mean = rng.standard_normal((cfg.k, cfg.z_dim)).astype(np.float32)
    eps = rng.standard_normal((128, cfg.k, cfg.z_dim)).astype(np.float32)
    fixed = es_loop_ref(gen, loss, mean, 23.3, eps, 128, 16, 4, move=False)
    moving = es_loop_ref(gen, loss, mean, 23.3, eps, 128, 16, 4)
    print(seed, fixed["best_loss"], moving["best_loss"], moving["best_loss"] / fixed["best_loss"])
    assert moving["best_loss"] <= 0.75 * fixed["best_loss"]
    assert abs(fixed["best_loss"] - CPU_TABLE[seed][0]) <= 1e-4 * CPU_TABLE[seed][0]
    assert abs(moving["best_loss"] - CPU_TABLE[seed][1]) <= 1e-4 * CPU_TABLE[seed][1]
    assert np.array_equal(fixed["means"][-1], mean) and not np.array_equal(moving["means"][0], mean)
    assert (moving["used"] == 4).all()


def test_module_entry_parser_and_the_untouched_cli():
    from morphganformer_amd import evolution
    ap = evolution.build_parser()
    a = ap.parse_args(["--image", "face.png"])
    assert (a.batch, a.elite, a.es_weights, a.mean_lr, a.landmarks, a.step, a.pixel_term) == (32, None, "log", 1.0, None, 5000, "mse")
    a = ap.parse_args(["--model", "n.pkl", "--image", "f.png", "--landmarks", "lm.npz", "--path_to_gen", "out", "--batch", "16", "--elite", "4",
                       "--es-weights", "equal", "--mean-lr", "0.5", "--size", "64", "--step", "32", "--no-lpips", "--pixel-term", "dssim",
                       "--lamda", "0.1", "--seed", "3", "--net", "vgg", "--biometric", "iresnet18", "--gamma", "2", "--pool-above", "256"])
    assert (a.batch, a.elite, a.es_weights, a.mean_lr, a.size, a.step, a.no_lpips, a.pixel_term, a.seed) == (16, 4, "equal", 0.5, 64, 32, True, "dssim", 3)
    for bad in (["--es-weights", "rank"], ["--pixel-term", "lbp"], []):
        with pytest.raises(SystemExit):
            ap.parse_args(bad if not bad else ["--image", "f.png"] + bad)
    # the checks of the command line run before anything is loaded
    for argv, what in ((["--batch", "1"], "--batch"), (["--batch", "4", "--elite", "5"], "--elite"), (["--mean-lr", "0"], "--mean-lr"),
                       (["--mean-lr", "1.5"], "--mean-lr")):
        with pytest.raises(SystemExit, match=what):
            evolution.main(["--image", "f.png", "--model", "/nonexistent.pkl"] + argv)
    # the package's own command line has no evolution verb or mode (tests/test_cli_parser_host.py pins its whole table)
    from morphganformer_amd import cli
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["project", "--image", "f.png", "--mode", "evolution"])


def test_entry_point_is_declared_bound_and_built():
    from morphganformer_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mgf.h")).read()
    assert re.search(r"int mgf_es_recombine_f32\(float\* mean, const float\* cand, const double\* totals, const int32_t\* step0,", header)
    assert "mgf_es_recombine_f32" in _lib.EXPORTED_SYMBOLS and "evolution.hip" in build.SOURCES
    assert len(_lib._SIGS["mgf_es_recombine_f32"][1]) == 12
