"""GPU parity of the MobileFaceNet embedder: the depthwise kernels of csrc/depthwise.hip per element against
float64 torch, the embedder and its backward pass against what the reference module recorded in tests/golden/mobilefacenet.npz
(tools/make_mobilefacenet_golden.py), and the biometric term on it inside both projection engines and the command line.

The per-element gate is the replay convention of tests/conv_replay.py: |got - ref64| <= c A with A = sum |w| |x| |scale| + |shift| and
c = max(4 r, sqrt(K) 2^-24), r = max |ref32 - ref64| / A of the same evaluator (F.conv2d, groups = channels) in float32, K the taps per
output.  A PReLU with a slope in [0, 1] is 1-Lipschitz, so A bounds the activated value as well."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mobilefacenet_torch_ref import as_state, biometric_loss_torch, embed_image_torch, fixture_gradients, mobilefacenet_torch  # noqa: E402

pytestmark = pytest.mark.gpu

M_DIRECT = 4.0
CANARY = 0x7FC0BEEF                       # a NaN with a payload: any write changes the bits
# (k, stride, pad, in_h, in_w): 3x3 pad 1 at both strides on odd, non-square, tile-ragged and multi-block maps; stride 2 with inputs 7 and 8
# (both -> 4), 14, 55 / 57 and 56; the 7x7 valid conv on its own 7x7 map (-> 1x1) and on 9x8 (-> 3x2)
GEOMETRIES = [(3, 1, 1, 7, 7), (3, 1, 1, 8, 9), (3, 1, 1, 56, 56), (3, 1, 1, 57, 55), (3, 2, 1, 7, 7), (3, 2, 1, 8, 9), (3, 2, 1, 14, 14),
              (3, 2, 1, 56, 56), (3, 2, 1, 57, 55), (7, 1, 0, 7, 7), (7, 1, 0, 9, 8)]
EPILOGUES = [(True, True, True), (False, False, False), (False, False, True), (True, True, False)]


def _gate(ref32, ref64, A, K):
    ok = A > 0
    r = float(((ref32.double() - ref64).abs()[ok] / A[ok]).max())
    return max(M_DIRECT * r, math.sqrt(K) * 2.0 ** -24)


def _case(gen, n, c, h, w, k):
    x = torch.randn(n, c, h, w, generator=gen)
    wt = torch.randn(c, 1, k, k, generator=gen) / k
    scale = torch.rand(c, generator=gen) + 0.5
    shift = torch.randn(c, generator=gen) * 0.3
    slope = torch.rand(c, generator=gen) * 0.3 + 0.1
    return x, wt, scale, shift, slope


def _forward_ref(x, wt, scale, shift, slope, stride, pad, dtype):
    bc = lambda v: v.to(dtype).reshape(1, -1, 1, 1)
    y = F.conv2d(x.to(dtype), wt.to(dtype), None, stride, pad, 1, x.shape[1])
    if scale is not None:
        y = y * bc(scale)
    if shift is not None:
        y = y + bc(shift)
    return F.prelu(y, slope.to(dtype)) if slope is not None else y


def _dw(L, y, x, w, scale, shift, slope, n, c, h, wd, k, stride, pad):
    from morphganformer_amd import _lib
    return L.mgf_dwconv_f32(_lib.ptr(y), _lib.ptr(x), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(slope), n, c, h, wd, k, k, stride,
                            pad, _lib.stream_ptr())


def _dw_bwd(L, dx, dy, w, scale, y, slope, xa, xs, n, c, h, wd, k, stride, pad):
    from morphganformer_amd import _lib
    return L.mgf_dwconv_bwd_data_f32(_lib.ptr(dx), _lib.ptr(dy), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(y), _lib.ptr(slope), _lib.ptr(xa),
                                     _lib.ptr(xs), n, c, h, wd, k, k, stride, pad, _lib.stream_ptr())


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "k{}s{}p{}_{}x{}".format(*g))
def test_depthwise_forward_per_element(geo):
    from morphganformer_amd import _lib
    L = _lib.lib()
    k, stride, pad, h, w = geo
    gen = torch.Generator().manual_seed(1000 * k + 100 * stride + h)
    for n in (1, 3):
        for c in (1, 5, 64, 130):
            x, wt, scale, shift, slope = _case(gen, n, c, h, w, k)
            xd, wd = x.cuda(), wt.reshape(c, k * k).contiguous().cuda()
            for use_scale, use_shift, use_slope in EPILOGUES:
                sc, sh, sl = scale if use_scale else None, shift if use_shift else None, slope if use_slope else None
                ref64 = _forward_ref(x, wt, sc, sh, sl, stride, pad, torch.float64)
                ref32 = _forward_ref(x, wt, sc, sh, sl, stride, pad, torch.float32)
                A = F.conv2d(x.double().abs(), wt.double().abs(), None, stride, pad, 1, c)
                if sc is not None:
                    A = A * sc.double().reshape(1, -1, 1, 1)
                if sh is not None:
                    A = A + sh.double().abs().reshape(1, -1, 1, 1)
                numel = ref64.numel()
                assert tuple(ref64.shape[2:]) == ((h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1)
                buf = torch.full((numel + 64,), CANARY, dtype=torch.int32, device="cuda")
                dev = [None if t is None else t.cuda() for t in (sc, sh, sl)]
                _lib.check(_dw(L, buf.view(torch.float32), xd, wd, *dev, n, c, h, w, k, stride, pad), "dwconv")
                got = buf[:numel].view(torch.float32).cpu().double().reshape(ref64.shape)
                assert bool((buf[numel:] == CANARY).all()), (geo, n, c, "wrote past the output")
                cgate = _gate(ref32, ref64, A, k * k)
                excess = ((got - ref64).abs() - cgate * A).max()
                assert float(excess) <= 0, (geo, n, c, (use_scale, use_shift, use_slope), float(((got - ref64).abs() / (cgate * A)).max()))


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "k{}s{}p{}_{}x{}".format(*g))
def test_depthwise_data_gradient_per_element(geo):
    """dx against float64 autograd through conv -> scale -> PReLU, with and without the two masks; the masked forms are the unmasked
    kernel on (mask * dy) and mask * (unmasked result), bit for bit."""
    from morphganformer_amd import _lib
    L = _lib.lib()
    k, stride, pad, h, w = geo
    gen = torch.Generator().manual_seed(2000 * k + 100 * stride + h)
    for n in (1, 3):
        for c in (1, 5, 64, 130):
            x, wt, scale, shift, slope = _case(gen, n, c, h, w, k)
            in_slope = torch.rand(c, generator=gen) * 0.3 + 0.1
            xa = F.prelu(x, in_slope)                                     # the post-activation map the layer reads
            y32 = _forward_ref(xa, wt, scale, shift, slope, stride, pad, torch.float32)
            dy = torch.randn(y32.shape, generator=gen)
            bc = lambda v: v.reshape(1, -1, 1, 1)
            m_out = torch.where(y32 > 0, torch.ones(()), bc(slope))
            m_in = torch.where(xa > 0, torch.ones(()), bc(in_slope))
            dev = {name: t.cuda() for name, t in dict(dy=dy, w=wt.reshape(c, k * k).contiguous(), scale=scale, y=y32, slope=slope, xa=xa,
                                                      xs=in_slope, mdy=(m_out * dy)).items()}
            numel = x.numel()

            def run(dy_, scale_, y_, slope_, xa_, xs_):
                buf = torch.full((numel + 64,), CANARY, dtype=torch.int32, device="cuda")
                _lib.check(_dw_bwd(L, buf.view(torch.float32), dy_, dev["w"], scale_, y_, slope_, xa_, xs_, n, c, h, w, k, stride, pad), "dwconv_bwd")
                assert bool((buf[numel:] == CANARY).all()), (geo, n, c, "wrote past dx")
                return buf[:numel].view(torch.float32).reshape(x.shape).clone()

            def ref(dtype, masked):
                z = torch.zeros(x.shape, dtype=dtype, requires_grad=True)
                out = F.conv2d(z, wt.to(dtype), None, stride, pad, 1, c) * bc(scale).to(dtype)
                g = dy.to(dtype) * (m_out.to(dtype) if masked else 1)
                (dz,) = torch.autograd.grad(out, z, g)
                return dz * m_in.to(dtype) if masked else dz

            for masked in (False, True):
                got = run(dev["dy"], dev["scale"], *((dev["y"], dev["slope"], dev["xa"], dev["xs"]) if masked else (None,) * 4)).cpu().double()
                ref64, ref32 = ref(torch.float64, masked), ref(torch.float32, masked)
                zA = torch.zeros(x.shape, dtype=torch.float64, requires_grad=True)
                gA = dy.double().abs() * (m_out.double() if masked else 1)
                (A,) = torch.autograd.grad(F.conv2d(zA, wt.double().abs(), None, stride, pad, 1, c) * bc(scale).double(), zA, gA)
                A = A * m_in.double() if masked else A
                cgate = _gate(ref32, ref64, A, math.ceil(k / stride) ** 2)
                err = (got - ref64).abs()
                assert float((err - cgate * A).max()) <= 0, (geo, n, c, masked, float((err[A > 0] / (cgate * A[A > 0])).max()))
                assert float(err[A == 0].max() if bool((A == 0).any()) else 0.0) == 0.0          # an input no window covers: exactly 0
            plain = run(dev["dy"], None, None, None, None, None)
            assert torch.equal(run(dev["dy"], None, dev["y"], dev["slope"], None, None), run(dev["mdy"], None, None, None, None, None))
            assert torch.equal(run(dev["dy"], None, None, None, dev["xa"], dev["xs"]), plain * m_in.cuda())


def test_depthwise_bad_geometry_is_refused():
    from morphganformer_amd import _lib
    L = _lib.lib()
    t = torch.zeros(4096, device="cuda")
    for what, args in (("empty output", (t, t, t, None, None, None, 1, 2, 6, 7, 7, 1, 0)),
                       ("stride 3", (t, t, t, None, None, None, 1, 2, 9, 9, 3, 3, 1)),
                       ("null x", (t, None, t, None, None, None, 1, 2, 9, 9, 3, 1, 1)),
                       ("no channels", (t, t, t, None, None, None, 1, 0, 9, 9, 3, 1, 1))):
        with pytest.raises(_lib.MgfError, match="dwconv"):
            _lib.check(_dw(L, *args), "dw")
    with pytest.raises(_lib.MgfError, match="empty output"):
        _lib.check(_dw(L, t, t, t, None, None, None, 1, 2, 6, 7, 7, 1, 0))
    with pytest.raises(_lib.MgfError, match="stride 3"):
        _lib.check(_dw_bwd(L, t, t, t, None, None, None, None, None, 1, 2, 9, 9, 3, 3, 1))
    with pytest.raises(_lib.MgfError, match="NULL"):
        _lib.check(_dw_bwd(L, t, None, t, None, None, None, None, None, 1, 2, 9, 9, 3, 1, 1))
    with pytest.raises(_lib.MgfError, match="5x3"):                                # a kernel that is not square
        _lib.check(L.mgf_dwconv_f32(t.data_ptr(), t.data_ptr(), t.data_ptr(), None, None, None, 1, 2, 9, 9, 5, 3, 1, 1, None))
    with pytest.raises(_lib.MgfError, match="come together"):
        _lib.check(_dw_bwd(L, t, t, t, None, t, None, None, None, 1, 2, 9, 9, 3, 1, 1))


# ---------------------------------------------------------------------------------------------------------------- the embedder
@pytest.fixture(scope="module")
def fx(golden):
    from morphganformer_amd.mobilefacenet import MobileFaceNetEmbedder, random_state
    g = golden("mobilefacenet.npz")
    sd = random_state(0)
    return g, sd, as_state(sd, torch.float64), MobileFaceNetEmbedder(sd, n=2), fixture_gradients(g)[1]


def test_embedder_matches_the_reference_module(fx):
    g, sd, sd64, net, _ = fx
    x = torch.from_numpy(g["x"]).cuda()
    emb = net.embed(x).cpu().numpy()
    assert emb.shape == (2, 512) and net.out.shape == (2, 512) and net.n == 2
    print("embedding error / max|embedding|:", np.abs(emb - g["embedding"]).max() / np.abs(g["embedding"]).max())
    assert np.abs(emb - g["embedding"]).max() < 2e-4 * np.abs(g["embedding"]).max()
    assert len(net.stages) == 9
    for s, m, r in zip(net.stages, g["stage_mean"], g["stage_rms"]):
        assert abs(float(s.double().mean()) - m) < 1e-4 * r and abs(float(s.double().square().mean().sqrt()) - r) < 1e-4 * r
    # a batch size change re-allocates; the sample's result does not depend on the batch (17 crosses the 16-row GEMV split)
    scale = np.abs(emb).max()
    e1 = net.clone_for(1).embed(x[1:]).cpu().numpy()
    assert np.abs(e1[0] - emb[1]).max() < 1e-5 * scale
    x17 = torch.cat([x[:1].expand(16, -1, -1, -1), x[1:]]).contiguous()
    e17 = net.clone_for(17).embed(x17).cpu().numpy()
    assert np.abs(e17[16] - emb[1]).max() < 1e-5 * scale and np.abs(e17[:16] - emb[0]).max() < 1e-5 * scale


@pytest.mark.parametrize("size", [(64, 64), (96, 80)])
def test_embed_image_resizes_like_interpolate(fx, size):
    g, sd, sd64, net, _ = fx
    img = torch.rand(2, 3, *size, generator=torch.Generator().manual_seed(size[1])) * 2 - 1
    with torch.no_grad():
        want = embed_image_torch(sd64, img.double()).numpy()
    e = net.clone_for(2)
    got = e(img.cuda()).cpu().numpy()
    assert got is not None and np.abs(got - want).max() < 2e-4 * np.abs(want).max()


def test_backward_matches_the_float64_gradient(fx):
    g, sd, sd64, net, g64 = fx
    e = net.clone_for(2)
    e.embed(torch.from_numpy(g["x"]).cuda())
    v = torch.from_numpy(g["v"]).cuda()
    d = e.backward(v).cpu().numpy().astype(np.float64) - g64
    l2, mx = np.linalg.norm(d.ravel()) / np.linalg.norm(g64.ravel()), np.abs(d).max() / np.abs(g64).max()
    print("gradient error: relative L2", l2, "max / max|g|", mx, "reference's own:", float(g["r_grad_l2"]), float(g["r_grad_max"]))
    assert l2 <= max(8 * float(g["r_grad_l2"]), 1e-5) and mx <= max(8 * float(g["r_grad_max"]), 1e-5)
    # accumulate adds to what was there; without it dimg is overwritten
    dimg = torch.full((2, 3, 112, 112), 0.5, device="cuda")
    e.backward(v, dimg, accumulate=True)
    first = dimg.clone()
    e.backward(v, dimg)
    assert torch.allclose(first - 0.5, dimg, rtol=0, atol=1e-6 * float(np.abs(g64).max()))
    assert float((dimg.cpu().double() - torch.from_numpy(g64)).abs().max()) <= max(8 * float(g["r_grad_max"]), 1e-5) * np.abs(g64).max()


def test_backward_scatters_through_the_resize(fx):
    """backward into a 64x64 dimg.  The scatter itself is the adjoint of F.interpolate applied to the embedder's own 112x112 gradient, against
    float64 autograd: |err| <= 4 * 2^-24 * A + W * S, A = sum |weight| |g|, S = sum |g| over the outputs within one pixel of the source pixel's
    support.  W bounds a float32 bilinear weight's ABSOLUTE error: the source coordinate (dst + 0.5) * scale - 0.5 < 64 carries three roundings of
    2^-19 and the scale's 2^-24 * 64, under 4 * 2^-18 in all, and a weight is a product of two such factors: W = 2 * 4 * 2^-18.  The whole chain against float64 autograd is
    gated by the float32-against-float64 distance of the restatement ON THIS INPUT (r_in, measured here on the CPU), times the factor 8 of the
    backward gate: an up-sampled image is smooth, and on every such input drawn the network's own two precisions sit 1e-2 apart in the gradient
    (seeds 3..11: 0.7e-2 .. 3.2e-2 of max|g|; the MI355X result equals the float32 restatement to four digits)."""
    g, sd, sd64, net, _ = fx
    img = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)) * 2 - 1)
    v = torch.from_numpy(g["v"]).double()
    refs = []
    for state, dt in ((sd64, torch.float64), (as_state(sd, torch.float32), torch.float32)):
        x = img.to(dt).requires_grad_(True)
        refs.append(torch.autograd.grad((embed_image_torch(state, x) * v.to(dt)).sum(), x)[0].double())
    ref, ref32 = refs
    r_max, r_l2 = float((ref32 - ref).abs().max() / ref.abs().max()), float((ref32 - ref).norm() / ref.norm())
    e = net.clone_for(2)
    e.embed_image(img.cuda())
    d112 = e.backward(v.float().cuda()).clone()
    dimg = torch.zeros(2, 3, 64, 64, device="cuda")
    e.backward(v.float().cuda(), dimg)
    got = dimg.cpu().double()
    z = torch.zeros(2, 3, 64, 64, dtype=torch.float64, requires_grad=True)
    up = F.interpolate(z, size=(112, 112), mode="bilinear", align_corners=False)
    (adj,) = torch.autograd.grad(up, z, d112.cpu().double())
    (A,) = torch.autograd.grad(up, z, d112.cpu().double().abs())
    src = np.floor(np.clip((np.arange(112) + 0.5) * 64 / 112 - 0.5, 0, None)).astype(np.int64)
    S, absg = np.zeros((2, 3, 64, 64)), d112.cpu().double().abs().numpy()
    for dy in (-1, 0, 1, 2):
        for dx in (-1, 0, 1, 2):
            np.add.at(S, (slice(None), slice(None), np.clip(src + dy, 0, 63)[:, None], np.clip(src + dx, 0, 63)[None, :]), absg)
    bound = 4 * 2.0 ** -24 * A + 8 * 2.0 ** -18 * torch.from_numpy(S)
    print("scatter vs the adjoint of interpolate: max |err| / bound", float(((got - adj).abs() / bound.clamp_min(1e-300)).max()),
          "max |err| / max|g64|", float((got - adj).abs().max() / adj.abs().max()))
    assert float(((got - adj).abs() - bound).max()) <= 0
    err, l2 = float((got - ref).abs().max() / ref.abs().max()), float((got - ref).norm() / ref.norm())
    print("gradient through the resize: max error / max|g|", err, "relative L2", l2, "the restatement's own float32:", r_max, r_l2)
    assert err <= max(8 * r_max, 1e-5) and l2 <= max(8 * r_l2, 1e-5)


def test_non_positive_slopes_and_unbuilt_variants_are_refused():
    from morphganformer_amd import _lib
    from morphganformer_amd.iresnet import BiometricLoss
    from morphganformer_amd.mobilefacenet import MobileFaceNetEmbedder, random_state
    sd = random_state(1)
    sd["layers.3.layers.1.layers.1.layers.2.weight"] = sd["layers.3.layers.1.layers.1.layers.2.weight"].copy()
    sd["layers.3.layers.1.layers.1.layers.2.weight"][5] = -0.1
    e = MobileFaceNetEmbedder(sd, n=1)
    emb = e.embed(torch.zeros(1, 3, 112, 112, device="cuda"))                   # the forward pass takes any slope
    assert bool(torch.isfinite(emb).all())
    with pytest.raises(_lib.MgfError, match="PReLU slopes must be positive"):
        e.backward(torch.ones(1, 512, device="cuda"))
    with pytest.raises(_lib.MgfError, match="fp16"):
        MobileFaceNetEmbedder(None, fp16=True)
    with pytest.raises(_lib.MgfError, match="num_features"):
        MobileFaceNetEmbedder(None, num_features=128)
    with pytest.raises(ValueError, match="mobilefacenet"):
        BiometricLoss("resnet1000")
    with pytest.raises(_lib.MgfError, match="no CPU fallback"):
        e.embed(torch.zeros(1, 3, 112, 112))


# ---------------------------------------------------------------------------------------------------------------- in the loops
@pytest.fixture(scope="module")
def tiny():
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import TINY, make_state_dict
    return Generator(make_state_dict(TINY, seed=0), TINY, "cuda", max_batch=4), TINY


def _setup(G, cfg, steps, targets=1, seed=5):
    torch.manual_seed(seed)
    latent_mean = torch.randn(cfg.k, cfg.z_dim, device="cuda")
    eps = torch.randn(steps, targets, cfg.k, cfg.z_dim, device="cuda")
    target = G(torch.randn(targets, cfg.k, cfg.z_dim, device="cuda"), None, noise_mode="const")[0].clamp(-1, 1).clone()
    return latent_mean, eps, target


def test_literal_loop_with_the_mobilefacenet_term(tiny, fx):
    """The biometric term alone as the objective, 4 candidates per replayed graph: every recorded loss is the float64 helper's value of
    that candidate's image, the best step is its arg-min; retarget() swaps the target in place."""
    from morphganformer_amd.iresnet import BiometricLoss
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine
    G, cfg = tiny
    sd64 = fx[2]
    steps, gamma = 8, 1.0
    latent_mean, eps, target = _setup(G, cfg, steps)
    bio = BiometricLoss("mobilefacenet", state=fx[1], n=4)
    eng = ProjectionEngine(G, target, latent_mean, 1.0, ProjectionArgs(step=steps, min_loss_init=1e30), eps=eps, noise_mode="const", batch=4,
                           biometric=bio, gamma=gamma, use_mse=False, use_graph=True)
    lat, bstep, bloss, losses = eng.run().result()
    assert eng.graph is not None

    def want(eps_, target_):
        lats = latent_mean[None] + eps_[:, 0] * eng.sigma[:steps].reshape(-1, 1, 1)
        imgs = torch.cat([G(lats[i:i + 4].contiguous(), None, noise_mode="const")[0] for i in range(0, steps, 4)]).cpu().double()
        with torch.no_grad():
            return gamma * biometric_loss_torch(sd64, imgs, target_.cpu().double()).numpy()

    ref = want(eps, target)
    print("literal loop: max relative loss error", np.abs(losses - ref).max() / np.abs(ref).max())
    assert np.abs(losses - ref).max() < 1e-3 * np.abs(ref).max() and np.all(np.abs(losses - ref) < 1e-3 * np.abs(ref) + 1e-12)
    assert bstep == int(np.argmin(ref)) and abs(bloss - ref.min()) < 1e-3 * ref.min()
    # another target, same engine, same graph
    _, eps2, target2 = _setup(G, cfg, steps, seed=6)
    graph = eng.graph
    eng.retarget(target2, eps=eps2)
    _, bstep2, _, losses2 = eng.run().result()
    ref2 = want(eps2, target2)
    assert eng.graph is graph and np.abs(losses2 - ref2).max() < 1e-3 * np.abs(ref2).max() and bstep2 == int(np.argmin(ref2))


@pytest.mark.parametrize("targets", [1, 2])
def test_gradient_loop_with_the_mobilefacenet_term(tiny, fx, targets):
    """Gradient mode, one target and two in lockstep: the first step (lr = 0) scores the literal engine's candidate, the latent moves."""
    from morphganformer_amd.iresnet import BiometricLoss
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, ProjectionEngine
    G, cfg = tiny
    steps, gamma = 4, 10.0
    latent_mean, eps, target = _setup(G, cfg, steps, targets, seed=8)
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.25, min_loss_init=1e30)
    firsts = []
    for j in range(targets):
        lit = ProjectionEngine(G, target[j:j + 1].contiguous(), latent_mean, 1.0, args, eps=eps[:, j:j + 1].contiguous(), noise_mode="const", batch=1,
                               biometric=BiometricLoss("mobilefacenet", state=fx[1], n=1), gamma=gamma, use_graph=False).run(1)
        firsts.append(float(lit.losses[0]))
    eng = GradientProjectionEngine(G, target, latent_mean, 1.0, args, eps=eps, noise_mode="const", use_graph=True,
                                   biometric=BiometricLoss("mobilefacenet", state=fx[1], n=targets), gamma=gamma).run()
    losses = eng.result()[3].reshape(targets, steps)
    assert np.isfinite(losses).all()
    for j in range(targets):
        assert abs(losses[j, 0] - firsts[j]) < 1e-4 * abs(firsts[j])
    assert float((eng.latent_in.reshape(targets, -1) - latent_mean.reshape(1, -1)).abs().max()) > 0.01


def test_biometric_grad_into_matches_autograd(fx):
    """d(scale * MSE(embed(pred), embed(target)))/d(pred) under the backward gate, on the fixture's input: which PReLU units sit at a kink depends
    on the input alone, and that input is the one on which the reference's two precisions agree (r_grad_*)."""
    from morphganformer_amd.iresnet import BiometricLoss
    g, sd, sd64, net, _ = fx
    pred = torch.from_numpy(g["x"]).double().requires_grad_(True)
    target = torch.rand(1, 3, 112, 112, generator=torch.Generator().manual_seed(11), dtype=torch.float64) * 2 - 1
    val = biometric_loss_torch(sd64, pred, target)
    (ref,) = torch.autograd.grad(val.sum() * 0.3, pred)
    val = val.detach()
    bio = BiometricLoss(net.clone_for(2))
    bio.set_target(target.float().cuda())
    out = torch.empty(2, device="cuda")
    bio.distance_into(out, pred.detach().float().cuda())
    assert float((out.cpu().double() - val).abs().max()) < 1e-4 * float(val.abs().max())
    dimg = torch.full((2, 3, 112, 112), 0.5, device="cuda")
    bio.grad_into(dimg, scale=0.3)
    err = (dimg.cpu().double() - ref).abs().max() / ref.abs().max()
    l2 = (dimg.cpu().double() - ref).norm() / ref.norm()
    print("grad_into: max error / max|g|", float(err), "relative L2", float(l2))
    assert float(err) <= max(8 * float(g["r_grad_max"]), 1e-5) and float(l2) <= max(8 * float(g["r_grad_l2"]), 1e-5)


def test_cli_project_with_mobilefacenet(tmp_path):
    from morphganformer_amd import cli
    from test_host_and_abi import _tiny_snapshot
    pkl = str(tmp_path / "net.pkl")
    _tiny_snapshot(pkl, seed=3)
    assert cli.main(["generate", "--model", pkl, "--output-dir", str(tmp_path / "src"), "--images-num", "1", "--seed", "1"]) == 0
    proj = ["project", "--model", pkl, "--image", str(tmp_path / "src" / "sample_000000.png"), "--size", "64", "--step", "4", "--n_mean_latent", "200",
            "--batch", "2", "--seed", "0", "--no-lpips", "--biometric", "mobilefacenet", "--gamma", "1e-12"]       # (random weights: distances far above min_loss)
    with pytest.raises(SystemExit, match="biometric-weights"):
        cli.main(proj + ["--path_to_gen", str(tmp_path / "a")])
    assert cli.main(proj + ["--biometric-random", "--path_to_gen", str(tmp_path / "b")]) == 0
    assert cli.main(proj + ["--biometric-random", "--mode", "gradient", "--path_to_gen", str(tmp_path / "c")]) == 0
