"""conv_last + ToRGB of the last block as ONE composed per-sample 3x3 convolution into the image channels
(mgf_torgb_compose_weights_f32 + mgf_conv3x3_few_outputs_f32) against float64 references and against the two-layer / fused-epilogue
path it replaces (MGF_TORGB_COMPOSE=0 is the same switch as Generator.torgb_compose = False)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def compose_ref(w_last, s_last, d_last, w_rgb, s_rgb):
    """float64 host composition: w_eff[n, c, i, k] = s_last[n, i] sum_o w_rgb[c, o] s_rgb[n, o] d_last[n, o] w_last[o, i, k]."""
    a = w_rgb.double()[None] * s_rgb.double()[:, None, :] * d_last.double()[:, None, :]           # [n, c, o]
    return torch.einsum("nco,oikl->ncikl", a, w_last.double()) * s_last.double()[:, None, :, None, None]


@pytest.mark.parametrize("n,cin,cout,rc", [(1, 32, 32, 3), (5, 32, 32, 1), (32, 32, 32, 3), (3, 36, 20, 4)])
def test_compose_weights_vs_float64(n, cin, cout, rc):
    from morphganformer_amd import _lib
    torch.manual_seed(n * 100 + rc)
    w_last = torch.randn(cout, cin, 3, 3) / (3 * cin ** 0.5)
    s_last, d_last = 1 + 0.3 * torch.randn(n, cin), 0.5 + torch.rand(n, cout)
    w_rgb, s_rgb = torch.randn(rc, cout), torch.randn(n, cout) / cout ** 0.5
    dv = [t.cuda().contiguous() for t in (w_last, s_last, d_last, w_rgb, s_rgb)]       # (alive until the launch has run)
    out = torch.empty(n, rc, cin, 3, 3, device="cuda")
    _lib.check(_lib.lib().mgf_torgb_compose_weights_f32(out.data_ptr(), *[t.data_ptr() for t in dv], n, cin, cout, rc, _lib.stream_ptr()),
               "torgb_compose_weights")
    torch.cuda.synchronize()
    ref = compose_ref(w_last, s_last, d_last, w_rgb, s_rgb)
    ulp = torch.from_numpy(np.spacing(np.abs(ref.float().numpy())).astype(np.float64))
    assert bool(((out.cpu().double() - ref).abs() <= 2 * ulp).all())


@pytest.mark.parametrize("n,rc,cin,h,w", [
    (1, 3, 32, 64, 64), (3, 1, 4, 37, 29), (32, 3, 32, 48, 64), (3, 4, 36, 33, 40), (1, 4, 4, 5, 3), (3, 3, 32, 256, 256),
    (32, 1, 36, 20, 21), (1, 3, 36, 1, 1), (3, 2, 32, 17, 1030),
])
def test_conv3x3_few_outputs_vs_float64(n, rc, cin, h, w):
    from morphganformer_amd import conv as cv
    torch.manual_seed(h * 7 + w + rc)
    x = torch.randn(n, cin, h, w)
    wt = torch.randn(n, rc, cin, 3, 3) / (3 * cin ** 0.5)
    b = torch.randn(rc)
    ref = torch.stack([torch.nn.functional.conv2d(x[j:j + 1].double(), wt[j].double(), b.double(), padding=1)[0] for j in range(n)])
    out = cv.conv3x3_few_outputs(x.cuda(), wt.cuda(), b.cuda())
    assert rel_err(out, ref) <= 5e-6
    nob = cv.conv3x3_few_outputs(x.cuda(), wt.cuda(), None)
    assert rel_err(nob, ref - b.double()[None, :, None, None]) <= 5e-6


def test_conv3x3_few_outputs_full_size():
    """The shape the last block runs at (32 -> 3 at 1024^2), two samples."""
    from morphganformer_amd import conv as cv
    torch.manual_seed(1024)
    n, rc, cin = 2, 3, 32
    x = torch.randn(n, cin, 1024, 1024)
    wt = torch.randn(n, rc, cin, 3, 3) / (3 * cin ** 0.5)
    b = torch.randn(rc)
    out = cv.conv3x3_few_outputs(x.cuda(), wt.cuda(), b.cuda()).cpu()
    for j in range(n):
        ref = torch.nn.functional.conv2d(x[j:j + 1].double(), wt[j].double(), b.double(), padding=1)[0]
        assert rel_err(out[j], ref) <= 5e-6, j


@pytest.mark.parametrize("batch", [32, 1])
def test_generator_composed_equals_two_layer(batch):
    """1024^2 generator, random latents: the composed last block vs the full conv_last with ToRGB fused into its epilogue."""
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import FULL1024, make_state_dict, synthetic_latents
    G = Generator(make_state_dict(FULL1024, seed=0), FULL1024, "cuda", max_batch=batch)
    assert G.torgb_compose and G.fuse_torgb
    assert [lp for lp in G.plan.layers if lp.name.endswith(".conv_last")][0].w_gained is not None
    z = torch.from_numpy(synthetic_latents(FULL1024, batch, seed=77)).cuda()
    new = G.forward_workspace(z, None, noise_mode="const")[0].clone()
    G.torgb_compose = False
    old = G.forward_workspace(z, None, noise_mode="const")[0].clone()
    assert float((new - old).abs().max()) <= 1e-5 * float(old.abs().max())


def test_projection_engine_composed_equals_old_path():
    """configs[1] as bench.py runs it (1024^2, Wing + LPIPS(squeeze) + MSE, 32 candidates per forward, graph replay, pipelined) with the
    composed last block and with the old one: same best step, bit-identical best latent, loss history within 1e-5."""
    from morphganformer_amd.drivers import DEFAULT_BATCH
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine, latent_stats, synthetic_landmarks
    from morphganformer_amd.synth_weights import FULL1024, make_state_dict, synthetic_latents
    G = Generator(make_state_dict(FULL1024, seed=0), FULL1024, "cuda", max_batch=1)
    target = G(torch.from_numpy(synthetic_latents(FULL1024, 1, 1000)).cuda(), None, noise_mode="const")[0].clamp(-1, 1).clone()
    gen = torch.Generator(device="cuda"); gen.manual_seed(0)
    mean, std = latent_stats(G, 10000, "cuda", gen)
    steps = 70
    lm_t, lm_s = synthetic_landmarks(steps, 1024, 7)
    eps = torch.randn(steps, 1, FULL1024.k, FULL1024.z_dim, device="cuda", generator=gen)
    out = {}
    for compose in (True, False):
        G.torgb_compose = compose
        P = PerceptualLoss(net="squeeze", allow_random_backbone=True)
        eng = ProjectionEngine(G, target, mean, std, ProjectionArgs(step=steps), percept=P, use_mse=True, lm_target=lm_t, lm_steps=lm_s,
                               eps=eps, noise_mode="const", use_graph=True, batch=DEFAULT_BATCH, pipeline=True)
        out[compose] = eng.run().result()
    (lat_a, step_a, loss_a, hist_a), (lat_b, step_b, loss_b, hist_b) = out[True], out[False]
    assert not np.isnan(hist_a).any() and not np.isnan(hist_b).any()
    assert step_a == step_b
    assert torch.equal(lat_a, lat_b)
    assert np.abs(hist_a - hist_b).max() <= 1e-5 * np.abs(hist_b).max()
    assert abs(loss_a - loss_b) <= 1e-5 * abs(loss_b)
