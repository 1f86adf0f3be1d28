"""The command line's surface, held against the commit before its options were regrouped (host only): every subcommand's option table, the one
state-dict reader, ProjectionArgs.pool_factor against the expressions it replaced, and the ProjectionArgs `morph --refine` builds."""
import argparse
import json
import os
import pickle
import types

import numpy as np
import pytest
import torch

from morphganformer_amd import cli
from morphganformer_amd.projection import ProjectionArgs

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_parser_table.json")


def parser_table(ap):
    """{subcommand: {dest: what argparse holds for the option, help text left out}} -- the fixture is json.dump of this on the earlier parser."""
    sub = next(a for a in ap._actions if isinstance(a, argparse._SubParsersAction))
    row = lambda a: {"option_strings": list(a.option_strings), "dest": a.dest, "type": getattr(a.type, "__name__", None), "default": a.default,
                     "choices": None if a.choices is None else list(a.choices), "required": a.required, "nargs": a.nargs,
                     "action": type(a).__name__}
    return {name: {a.dest: row(a) for a in p._actions if not isinstance(a, argparse._HelpAction)} for name, p in sub.choices.items()}


def test_every_subcommand_keeps_its_options():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = parser_table(cli.build_parser())
    assert list(got) == list(want) == ["generate", "project", "morph-pairs", "morph", "merge-files", "morph-tree", "warp", "extract-facenet", "lpips-map"]
    assert [len(v) for v in want.values()] == [7, 51, 49, 39, 2, 6, 7, 5, 9]
    for name in want:
        assert sorted(got[name]) == sorted(want[name]), name
        for dest, row in want[name].items():
            assert got[name][dest] == row, (name, dest)


def test_state_dict_reader_takes_plain_wrapped_and_npz_alike(tmp_path):
    rng = np.random.default_rng(0)
    state = {"conv.weight": rng.standard_normal((3, 2, 3, 3)).astype(np.float32), "bn.running_var": rng.random(3).astype(np.float32),
             "bn.num_batches_tracked": np.array(7, dtype=np.int64)}
    tensors = {k: torch.from_numpy(v.copy()) for k, v in state.items()}
    torch.save(tensors, tmp_path / "plain.pth")
    torch.save({"state_dict": tensors, "epoch": 3}, tmp_path / "wrapped.pth")
    np.savez(tmp_path / "arrays.npz", **state)
    for name in ("plain.pth", "wrapped.pth", "arrays.npz"):
        got = cli._read_state_dict(str(tmp_path / name))
        assert list(got) == list(state), name
        for k, v in state.items():
            a = np.asarray(got[k])
            assert a.dtype == v.dtype and a.shape == v.shape and np.array_equal(a, v), (name, k)


class _NotATensorDict:
    def __init__(self):
        self.weights = [1.0, 2.0]


def test_state_dict_reader_refuses_a_pickle_of_arbitrary_objects(tmp_path):
    torch.save({"net": _NotATensorDict()}, tmp_path / "objects.pth")
    with pytest.raises(pickle.UnpicklingError):
        cli._read_state_dict(str(tmp_path / "objects.pth"))


@pytest.mark.parametrize("resolution", [64, 256, 1024])
@pytest.mark.parametrize("pool_above", [0, 32, 64, 100, 256, 1024, 2048])
def test_pool_factor_is_the_three_expressions_it_replaced(resolution, pool_above):
    r, pa = resolution, pool_above
    f = ProjectionArgs(pool_above=pa).pool_factor(r)
    assert f == (r // pa if (pa and r > pa) else 1)                                        # the engine's pool_factor
    assert r // f == (r // (r // pa) if (pa and r > pa) else r)                            # the target size of the command line and of project_many
    assert (f > 1) == bool(pa and r > pa and r // pa > 1) and (f <= 1 or f == r // pa)     # project_image: rescale the face crop, and by what


class _Recorded(Exception):
    pass


def test_morph_refine_does_not_take_the_rendering_psi_for_a_loop_argument(tmp_path, monkeypatch):
    """morph's --truncation_psi renders the linear morph; the refinement's ProjectionArgs keep their own default (and get exactly ten fields)."""
    from morphganformer_amd import drivers, loader
    seen = {}

    def refine_morph(G, w1, w2, ta, tb, alphas, **kw):
        seen.update(kw, alphas=alphas)
        raise _Recorded()

    def merge_morph(G, w1, w2, alphas, psi, **kw):
        seen["render_psi"] = psi
    for key in ("HSA_ENABLE_IPC_MODE_LEGACY", "CUDA_VISIBLE_DEVICES"):                     # main() sets them if absent: restored after the test
        monkeypatch.setenv(key, os.environ.get(key, "0"))
    monkeypatch.setattr(loader, "load_network", lambda path, device: {"Gs": types.SimpleNamespace(device=torch.device("cpu"))})
    monkeypatch.setattr(drivers, "load_latent_mat", lambda path: np.zeros((1, 2, 8), np.float32))
    monkeypatch.setattr(drivers, "image_transform", lambda src, size, device: torch.zeros(1, 3, size, size))
    monkeypatch.setattr(drivers, "merge_morph", merge_morph)
    monkeypatch.setattr(drivers, "refine_morph", refine_morph)
    argv = ["morph", "--model", "net.pkl", "--w1", "a.mat", "--w2", "b.mat", "--out", str(tmp_path / "m"), "--alphas", "0.25,0.5", "--refine",
            "--image-a", "a.png", "--image-b", "b.png", "--no-lpips", "--truncation_psi", "0.3", "--step", "7", "--lr", "0.2", "--lamda", "0.5",
            "--beta", "2", "--noise", "0.1", "--n_mean_latent", "11", "--ratio", "0.5", "--percept_weight", "3", "--pixel-term", "msssim",
            "--msssim-levels", "2", "--size", "64"]
    with pytest.raises(_Recorded):
        cli.main(argv)
    assert seen["render_psi"] == 0.3 and seen["alphas"] == [0.25, 0.5]
    assert seen["args"].truncation_psi == 0.7
    assert seen["args"] == ProjectionArgs(step=7, lamda=0.5, beta=2, lr=0.2, noise=0.1, n_mean_latent=11, ratio=0.5, percept_weight=3.0,
                                          pixel_term="msssim", msssim_levels=2)
    assert seen["percept"] is None and seen["biometric"] is None and seen["ratio"] == 0.5 and seen["use_mse"] is True
