"""CPU: the conditions under which tests/test_hip_latent_counts.py compares integer latent assignments.

Those tests demand the kernel's argmax to equal the reference's "wherever the two best are more than 1e-4 apart".  The pixels this leaves
out must be few, or the comparison says little: at most 3 % of a layer's pixels (latent_count_cases.MAX_UNDECIDED).  Here that cap is
asserted on the references alone -- the float64 formula on every direct-kernel case, the CPU oracle on every generator case -- with the
seeds and shapes the GPU tests use (both import them from tests/latent_count_cases.py).  Also host-side: the TF kwarg translation of a
snapshot with 8 components, and the refusal of latent counts / widths the kernels do not take, which needs no device."""
import numpy as np
import pytest
import torch

import latent_count_cases as lc


@pytest.mark.parametrize("n,c,f,T,with_ep", lc.FORWARD_CASES)
def test_forward_cases_leave_at_most_3_percent_undecided(n, c, f, T, with_ep):
    S, P, y = lc.attention_forward_ref(lc.attention_inputs(n, c, f, T), with_ep)
    assert tuple(S.shape) == (n, f, T) and tuple(y.shape) == (n, c, f)
    assert float((P.sum(-1) - 1).abs().max()) < 1e-12
    share = lc.undecided_share(S)
    assert share <= lc.MAX_UNDECIDED, share
    if T == 1:
        assert share == 0.0 and bool((S.argmax(-1) == 0).all())


def test_backward_cases_have_the_operands_of_the_forward_ones():
    """The backward cases draw from the same seeded generator: their probabilities are those of the forward formula."""
    for (n, c, res, T) in lc.BACKWARD_CASES[::5]:
        inp = lc.attention_inputs(n, c, res * res, T)
        P, dx, dv = lc.attention_backward_ref(inp)
        assert torch.equal(P, lc.attention_forward_ref(inp, False)[1])
        assert tuple(dx.shape) == (n, c, res * res) and tuple(dv.shape) == (n, c, T)
        if T == 1:                                                   # one latent: P = 1, the scores carry no gradient
            r = torch.rsqrt(inp["x"].square().mean(1, keepdim=True) + 1e-8)
            assert float((dv[..., 0] - (inp["da"] * inp["x"] * r).sum(-1)).abs().max()) < 1e-9


@pytest.mark.parametrize("cid", lc.GENERATOR_IDS)
def test_generator_cases_leave_at_most_3_percent_undecided_per_layer(cid):
    from morphganformer_amd.synth_weights import make_state_dict
    cfg = lc.generator_cases()[cid]
    T = cfg.k - 1
    sd = make_state_dict(cfg, seed=lc.weights_seed(cid))
    z, img, maps = lc.oracle_image_and_maps(cid, cfg, sd)
    assert tuple(img.shape) == (3, 3, cfg.img_resolution, cfg.img_resolution) and bool(torch.isfinite(img).all())
    want = [f"synthesis.b{res}.{name}" for res, name, _ci, _co, _up, _slot, att, _nb in cfg.layer_table() if att]
    assert sorted(maps) == sorted(want) and len(want) >= 5
    for key, probs in maps.items():
        assert probs.shape[0] == 3 and probs.shape[-1] == T, key
        share = lc.undecided_share(probs)
        assert share <= lc.MAX_UNDECIDED, (key, share)
        if T == 1:
            assert bool((probs == 1).all()), key


def test_projection_case_moves_the_latent():
    """The 3-step projection of the GPU test, oracle side only: the run must move the latent by more than the comparison's tolerance,
    or agreement with it would be no evidence (the condition test_gradient_projection_matches_autograd_adam puts on its own run)."""
    pr = lc.projection_reference()
    ref, args = pr["ref"], pr["args"]
    moved = float((ref[4][-1] - pr["latent_mean"]).abs().max())
    assert moved > 5 * args.lr * 0.2, moved
    assert len(ref[3]) == lc.PROJECTION_STEPS and all(v is not None and np.isfinite(v) for v in ref[3])
    assert ref[1] >= 0                                               # a best step was recorded


def test_tf_snapshot_with_8_components_gives_k_9():
    from morphganformer_amd.loader import config_from_tf_kwargs
    kw = {"architecture": "resnet", "transformer": True, "style": True, "local_noise": True, "kmeans": True, "use_pos": True,
          "integration": "mul", "norm": "layer", "mapping_resnet": True, "mapping_ltnt2ltnt": True,
          "resolution": 256, "latent_size": 32, "dlatent_size": 32, "components_num": 8}
    cfg = config_from_tf_kwargs(kw)
    assert cfg.k == 9 and cfg.num_components == 8 and cfg.w_dim == 32 and not cfg.normalize_global
    assert config_from_tf_kwargs({**kw, "components_num": 16}).k == 17


@pytest.mark.parametrize("bad,names", [(dict(k=18), "16"), (dict(w_dim=64, z_dim=64), "32")])
def test_generator_refuses_unsupported_latent_counts_and_widths_without_a_device(bad, names):
    """k = 18 (17 local latents; the attention kernels hold 16) and w_dim = 64 (the mapping kernel is built for 32) are refused by the
    constructor itself, with the limit in the message -- before the library is loaded, a weight is uploaded or a workspace is sized, so
    the refusal arrives on a machine without any GPU as well."""
    import dataclasses
    from morphganformer_amd import _lib
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import GeneratorConfig
    cfg = dataclasses.replace(GeneratorConfig(img_resolution=32, channel_base=256, channel_max=16), **bad)
    with pytest.raises((_lib.MgfError, ValueError), match=names):
        Generator({}, cfg, "cuda", max_batch=1)                      # (no weight is looked at: the state dict may as well be empty)
