"""The dispatch bench.py times -- 1024^2, 32 candidates per forward, LPIPS(squeeze) + MSE, graph replay, the losses of one batch on a side
stream beside the generator of the next -- held to the one-stream loop bit for bit, which only noise_mode="keyed" makes comparable: in random
mode the two draw their per-layer noise in different launch orders (tests/test_hip_drivers.py keeps that comparison to 64^2 and constant
noise)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_pipelined_headline_dispatch_equals_the_one_stream_loop_at_1024():
    """Three launch sequences of 32 candidates (96 steps: the prime graph, a steady-state graph of either parity's neighbour and the tail graph
    all run), then retarget() to another target under another seed and two more sequences (prime and both steady-state parities): best latent,
    best step, loss history and the improvement trail's images are bit-identical between pipeline=True and the one-stream engine."""
    from morphganformer_amd.drivers import DEFAULT_BATCH
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.lpips import PerceptualLoss, random_squeeze_backbone
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine
    from morphganformer_amd.synth_weights import FULL1024, make_state_dict, synthetic_latents
    cfg, B = FULL1024, DEFAULT_BATCH
    assert B == 32
    steps = 3 * B
    G = Generator(make_state_dict(cfg, seed=0), cfg, "cuda", max_batch=1)
    zs = torch.from_numpy(synthetic_latents(cfg, 2, seed=515)).cuda()
    targets = [G(zs[j:j + 1].contiguous(), None, noise_mode="const")[0].clamp(-1, 1).clone() for j in range(2)]
    mean = torch.from_numpy(synthetic_latents(cfg, 1, seed=516)[0]).cuda()

    def outcome(eng):
        lat, bstep, bloss, hist = eng.result()
        return lat, bstep, bloss, hist, [(s, l, im.cpu().clone()) for s, l, im in eng.improvements()]

    runs = {}
    for pipeline in (False, True):
        P = PerceptualLoss(net="squeeze", backbone_state=random_squeeze_backbone(0))
        eng = ProjectionEngine(G, targets[0], mean, 1.0, ProjectionArgs(step=steps), percept=P, use_mse=True, noise_mode="keyed", seed=21, batch=B,
                               pipeline=pipeline, keep_images=B, use_graph=True)
        first = outcome(eng.run())
        if pipeline:
            assert eng.pipeline and eng.prime_graph is not None and eng._seq_launched == 3
        second = outcome(eng.retarget(targets[1], seed=22).run(2 * B))
        runs[pipeline] = (first, second)
        del eng, P
    for which, (a, b) in enumerate(zip(runs[False], runs[True])):
        assert torch.equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2], which
        assert np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64)), which
        assert [(t[0], t[1]) for t in a[4]] == [(t[0], t[1]) for t in b[4]] and len(a[4]) >= 1, which
        assert all(torch.equal(x[2], y[2]) for x, y in zip(a[4], b[4])), which
    first, second = runs[True]
    assert not np.isnan(first[3]).any() and int(np.isnan(second[3]).sum()) == B            # the second run stopped after two of three sequences
    assert not np.array_equal(first[3][:2 * B], second[3][:2 * B])                         # the other target and key really count
