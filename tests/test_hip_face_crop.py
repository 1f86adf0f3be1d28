"""GPU: the aligned, antialiased face crop of the ArcFace biometric term -- mgf_face_crop_f32 / mgf_face_crop_bwd_f32 against the float64
restatement tests/face_crop_torch_ref.py, and the plumbing above them: ArcFaceEmbedder.set_crop, BiometricLoss.set_crop, both engines, the drivers.

Kernel tolerance: |got - ref| <= 1e-6 max|ref|.  The kernels compute in float64 and round once to float32 at the store (6e-8 relative); the margin
covers float64 sums taken in another order than the reference's.  With `accumulate`, max|ref| includes the prior content.  Every matrix has
sqrt|det| at least 0.05 away from an integer, so S = ceil(sqrt|det|) is no tie between the kernel's and the reference's arithmetic."""
import math

import numpy as np
import pytest
import torch

from face_crop_torch_ref import face_crop_torch, face_crop_torch_adjoint, similarity, subsamples

pytestmark = pytest.mark.gpu

TOL = 1e-6
FILTERS = {"area": 0, "bilinear": 1}


def _rand(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _mats(m):
    return torch.as_tensor(m, dtype=torch.float64).reshape(-1, 2, 3).contiguous()


def crop_fwd(x, m, size, filt="area"):
    from morphganformer_amd import _lib
    mats = _mats(m).cuda()
    n, _, h, w = x.shape
    y = torch.full((n, 3, size, size), float("nan"), device="cuda")
    _lib.check(_lib.lib().mgf_face_crop_f32(y.data_ptr(), x.data_ptr(), mats.data_ptr(), n, h, w, size, mats.shape[0], FILTERS[filt], _lib.stream_ptr()),
               "face_crop")
    torch.cuda.synchronize()
    return y


def crop_bwd(dy, m, h, w, filt="area", prior=None):
    from morphganformer_amd import _lib
    mats = _mats(m).cuda()
    n, _, size, _ = dy.shape
    dx = torch.full((n, 3, h, w), float("nan"), device="cuda") if prior is None else prior.clone()
    _lib.check(_lib.lib().mgf_face_crop_bwd_f32(dx.data_ptr(), dy.data_ptr(), mats.data_ptr(), n, h, w, size, mats.shape[0], FILTERS[filt],
                                                0 if prior is None else 1, _lib.stream_ptr()), "face_crop_bwd")
    torch.cuda.synchronize()
    return dx


def _close(tag, got, ref, scale=None):
    ref = ref.double()
    scale = float(ref.abs().max()) if scale is None else scale
    err = float((got.cpu().double() - ref).abs().max())
    print(f"{tag}: max error {err:.3e}, max|ref| {scale:.3e}, ratio {err / scale:.3e}")
    assert scale > 0 and err <= TOL * scale, tag


# name: (n, h, w, size, matrices, expected S per matrix)
CASES = {
    "up-0.5": (1, 160, 160, 112, similarity(0.5, 7.0, 30.0, 40.0), [1]),                     # many crop pixels per source pixel
    "s2-rot10": (1, 160, 160, 112, similarity(1.3, 10.0, 20.0, -6.0), [2]),
    "s3": (1, 300, 300, 112, similarity(2.6, -3.0, 6.0, 10.0), [3]),
    "border": (1, 160, 160, 112, similarity(1.3, 0.0, -48.0, 5.0), [2]),                     # a third of the crop left of the source
    "n2-two": (2, 120, 120, 56, torch.stack([similarity(1.3, 10.0, 20.0, 8.0), similarity(2.6, -8.0, -10.0, -4.0)]), [2, 3]),
    "n2-shared": (2, 120, 120, 56, similarity(1.7, 5.0, 10.0, 12.0), [2]),
    "96x160": (1, 96, 160, 112, similarity(1.3, -12.0, 2.0, -20.0), [2]),
    "1024-s8": (1, 1024, 1024, 112, similarity(7.3, 4.0, 130.0, 60.0), [8]),                 # the typical face: 64 sub-samples, the large indices
}
_REF = {}


def reference(name):
    """(x, dy, forward reference, adjoint reference) of a case, float64 on the host, computed once."""
    if name not in _REF:
        n, h, w, size, m, s = CASES[name]
        assert [subsamples(k) for k in _mats(m)] == s
        for k in _mats(m):
            r = math.sqrt(abs(float(k[0, 0] * k[1, 1] - k[0, 1] * k[1, 0])))
            assert abs(r - round(r)) >= 0.05
        seed = sorted(CASES).index(name)
        x, dy = _rand((n, 3, h, w), 100 + seed), _rand((n, 3, size, size), 200 + seed)
        _REF[name] = (x, dy, face_crop_torch(x, m, size), face_crop_torch_adjoint(dy, m, h, w))
    return _REF[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernels_vs_float64_reference(name):
    n, h, w, size, m, _ = CASES[name]
    x, dy, y_ref, dx_ref = reference(name)
    if name == "border":
        assert float(y_ref[0, :, :, :30].abs().max()) == 0.0 and float(y_ref[0, :, :, 40:].abs().min()) > 0.0
    _close(name + " forward", crop_fwd(x.cuda(), m, size), y_ref)
    _close(name + " adjoint", crop_bwd(dy.cuda(), m, h, w), dx_ref)


def test_bilinear_filter_is_one_sample_per_pixel():
    n, h, w, size, m, _ = CASES["s3"]
    x, dy, y_area, _ = reference("s3")
    y_ref = face_crop_torch(x, m, size, "bilinear")
    assert float((y_ref - y_area).abs().max()) > 1e-2              # (the area filter really averages here)
    _close("bilinear forward", crop_fwd(x.cuda(), m, size, "bilinear"), y_ref)
    _close("bilinear adjoint", crop_bwd(dy.cuda(), m, h, w, "bilinear"), face_crop_torch_adjoint(dy, m, h, w, "bilinear"))
    # with S = 1 the two filters are the same operator, bit for bit
    m1 = CASES["up-0.5"][4]
    x1, dy1 = reference("up-0.5")[:2]
    assert torch.equal(crop_fwd(x1.cuda(), m1, 112, "bilinear"), crop_fwd(x1.cuda(), m1, 112, "area"))
    assert torch.equal(crop_bwd(dy1.cuda(), m1, 160, 160, "bilinear"), crop_bwd(dy1.cuda(), m1, 160, 160, "area"))


@pytest.mark.parametrize("name", ["s2-rot10", "n2-two"])
def test_adjoint_accumulates_onto_prior_content(name):
    n, h, w, size, m, _ = CASES[name]
    _, dy, _, dx_ref = reference(name)
    prior = _rand((n, 3, h, w), 7) * 3
    want = prior.double() + dx_ref
    _close(name + " accumulate", crop_bwd(dy.cuda(), m, h, w, prior=prior.cuda()), want, scale=float(torch.maximum(want.abs(), prior.double().abs()).max()))


@pytest.mark.parametrize("name", ["s2-rot10", "1024-s8"])
def test_adjoint_bits_are_equal_over_two_calls(name):
    n, h, w, size, m, _ = CASES[name]
    dy = reference(name)[1].cuda()
    a, b = crop_bwd(dy, m, h, w), crop_bwd(dy, m, h, w)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    prior = _rand((n, 3, h, w), 8).cuda()
    assert torch.equal(crop_bwd(dy, m, h, w, prior=prior), crop_bwd(dy, m, h, w, prior=prior))


def test_refusals():
    from morphganformer_amd import _lib
    from morphganformer_amd.mobilefacenet import MobileFaceNetEmbedder
    L = _lib.lib()
    x, y, m = torch.zeros(2, 3, 16, 16, device="cuda"), torch.zeros(2, 3, 8, 8, device="cuda"), _mats(similarity(1.3, 0, 0, 0)).cuda()
    st = _lib.stream_ptr()
    assert L.mgf_face_crop_f32(y.data_ptr(), x.data_ptr(), m.data_ptr(), 2, 16, 16, 8, 3, 0, st) == -1          # 3 matrices for 2 images
    assert L.mgf_face_crop_f32(y.data_ptr(), x.data_ptr(), m.data_ptr(), 2, 16, 16, 8, 1, 5, st) == -1          # unknown filter
    assert L.mgf_face_crop_f32(y.data_ptr(), x.data_ptr(), 0, 2, 16, 16, 8, 1, 0, st) == -1                     # no matrices
    assert L.mgf_face_crop_bwd_f32(x.data_ptr(), y.data_ptr(), m.data_ptr(), 2, 16, 0, 8, 1, 0, 0, st) == -1
    assert L.mgf_face_crop_bwd_f32(0, y.data_ptr(), m.data_ptr(), 2, 16, 16, 8, 1, 0, 0, st) == -1
    bad = {"singular": [[1.0, 2.0, 0.0], [2.0, 4.0, 0.0]], "16 sub-samples": similarity(16.1, 0, 0, 0), "non-finite": [[1.0, 0.0, float("inf")], [0.0, 1.0, 0.0]]}
    for text, mat in bad.items():
        host = np.ascontiguousarray(_mats(mat).numpy())
        assert L.mgf_face_crop_check(host.ctypes.data, 1, 0) == -1 and text.encode() in L.mgf_last_error(), text
    e = MobileFaceNetEmbedder(None, n=1)
    for text, mat in bad.items():
        with pytest.raises(_lib.MgfError, match=text):
            e.set_crop(mat)
    assert e._crop is None                                        # a refused matrix sets nothing
    e.set_crop(similarity(16.1, 0, 0, 0), filter="bilinear")      # the bilinear filter forms no S
    with pytest.raises(ValueError, match="filter"):
        e.set_crop(similarity(1.3, 0, 0, 0), filter="lanczos")
    with pytest.raises(ValueError, match=r"\[2,3\]"):
        e.set_crop(np.zeros((3, 3)))
    e.set_crop(torch.stack([similarity(1.3, 0, 0, 0)] * 3))
    with pytest.raises(_lib.MgfError, match="3 matrices"):
        e.embed_image(torch.zeros(2, 3, 64, 64, device="cuda"))


# ------------------------------------------------------------------------------------------------------------------ the embedders
@pytest.fixture(scope="module")
def nets():
    from morphganformer_amd.iresnet import IResNetEmbedder
    from morphganformer_amd.mobilefacenet import MobileFaceNetEmbedder
    return {"iresnet18": IResNetEmbedder(None, depth=18, n=1, seed=3), "mobilefacenet": MobileFaceNetEmbedder(None, n=1, seed=3)}


M_A, M_B = similarity(1.3, 10.0, 20.0, 8.0), similarity(2.6, -8.0, 4.0, -4.0)


@pytest.mark.parametrize("name", ["iresnet18", "mobilefacenet"])
def test_embedder_with_a_crop(nets, name):
    e = nets[name].clone_for(2)
    assert e._crop is None
    img = _rand((2, 3, 300, 300), 31).cuda()
    plain = e.embed_image(img).clone()
    plain_x112 = e.x112.clone()
    demb = _rand((2, 512), 32).cuda()
    plain_dimg = e.backward(demb, torch.zeros_like(img)).clone()
    mats = torch.stack([M_A, M_B])
    e.set_crop(mats)
    buf = e._crop[0]
    emb = e.embed_image(img).clone()
    _close(name + " x112", e.x112, face_crop_torch(img.cpu(), mats, 112))
    assert torch.equal(emb, e.embed(e.x112.clone())) and not torch.equal(emb, plain)
    d112 = e.backward(demb).clone()
    dimg = e.backward(demb, torch.full_like(img, float("nan")))
    assert torch.equal(dimg, crop_bwd(d112, mats, 300, 300))
    prior = _rand((2, 3, 300, 300), 33).cuda()
    assert torch.equal(e.backward(demb, prior.clone(), accumulate=True), crop_bwd(d112, mats, 300, 300, prior=prior))
    # the share of pixels the identity gradient reaches: a lattice of 4 per crop pixel without the crop, the crop's whole footprint with it
    print(name, "pixels with a gradient: resize", float((plain_dimg != 0).float().mean()), "crop", float((dimg != 0).float().mean()))
    # a 112 x 112 input is cropped too (the resize passes it through)
    small = _rand((2, 3, 112, 112), 34).cuda()
    e.embed_image(small)
    _close(name + " x112 from 112", e.x112, face_crop_torch(small.cpu(), mats, 112))
    # same shape: rewritten in place; a shared matrix: a new buffer
    e.set_crop(torch.stack([M_B, M_A]), filter="bilinear")
    assert e._crop[0] is buf and e._crop[1] == 1 and torch.equal(buf.cpu(), torch.stack([M_B, M_A]))
    e.embed_image(img)
    _close(name + " x112 bilinear", e.x112, face_crop_torch(img.cpu(), torch.stack([M_B, M_A]), 112, "bilinear"))
    e.set_crop(M_A.numpy())
    assert e._crop[0] is not buf and tuple(e._crop[0].shape) == (1, 2, 3)
    e.embed_image(img)
    _close(name + " x112 shared", e.x112, face_crop_torch(img.cpu(), M_A, 112))
    assert e.clone_for(2)._crop is None and e.clone_for(1)._crop is None          # a clone carries no crop
    e.set_crop(None)
    assert torch.equal(e.embed_image(img), plain) and torch.equal(e.x112, plain_x112)
    assert torch.equal(e.backward(demb, torch.zeros_like(img)), plain_dimg)


# ------------------------------------------------------------------------------------------------------------------ BiometricLoss
def _embed(net, img, mat):
    """One image through a clone of `net` under `mat`: the hand-composed side of the checks below (float64 [1,512])."""
    e = net.clone_for(1)
    e.set_crop(mat)
    return e.embed_image(img).double().cpu()


# float32 embeddings are the same kernels on both sides; the loss kernels sum 512 float32 terms (at worst 512 x 2^-24 x 2 = 6e-5 relative)
LOSS_TOL = 1e-4


def test_biometric_loss_with_distinct_matrices(nets):
    from morphganformer_amd import _lib
    from morphganformer_amd.biometric import BiometricLoss
    net = nets["mobilefacenet"]
    pred, ta, tb = (_rand((1, 3, 200, 200), s).cuda() for s in (41, 42, 43))
    M_P = similarity(1.3, 4.0, 12.0, 15.0)
    d = lambda a, b: float(((a - b) ** 2).mean())
    out = torch.zeros(1, device="cuda")
    # one target, pred / target matrices distinct
    bio = BiometricLoss(net.clone_for(1))
    bio.set_crop(M_P, target=M_A)
    bio.set_target(ta)
    bio.distance_into(out, pred, scale=2.0)
    want = 2.0 * d(_embed(net, pred, M_P), _embed(net, ta, M_A))
    print("distinct matrices", float(out), want)
    assert abs(float(out) - want) <= LOSS_TOL * want
    # set_crop after set_target re-embeds the stored target
    bio2 = BiometricLoss(net.clone_for(1))
    bio2.set_target(ta)
    stale = bio2._target.clone()
    bio2.set_crop(M_P, target=M_A)
    assert not torch.equal(bio2._target, stale) and torch.equal(bio2._target, bio._target)
    out2 = torch.zeros(1, device="cuda")
    bio2.distance_into(out2, pred, scale=2.0)
    assert torch.equal(out2, out)
    # the default target matrix is pred's
    bio2.set_crop(M_P)
    bio2.distance_into(out2, pred)
    want = d(_embed(net, pred, M_P), _embed(net, ta, M_P))
    assert abs(float(out2) - want) <= LOSS_TOL * want
    # the gradient goes through the crop's adjoint
    dimg = torch.zeros_like(pred)
    bio2.grad_into(dimg)
    assert float((dimg != 0).float().mean()) > 0.3 and bool(torch.isfinite(dimg).all())
    # None restores the resize, target included
    bio2.set_crop(None)
    plain = BiometricLoss(net.clone_for(1))
    plain.set_target(ta)
    assert torch.equal(bio2._target, plain._target)
    out3 = torch.zeros(1, device="cuda")
    assert torch.equal(bio2.distance_into(out2, pred), plain.distance_into(out3, pred))
    # a pair with target_b under its own matrix
    alpha, delta = 0.3, 0.5
    bio.set_crop(M_P, target=M_A, target_b=M_B)
    bio.set_target_pair(ta, tb, alpha, id_balance=delta, metric="mse")
    bio.distance_into(out, pred, scale=2.0)
    ep = _embed(net, pred, M_P)
    da, db = d(ep, _embed(net, ta, M_A)), d(ep, _embed(net, tb, M_B))
    want = 2.0 * ((1 - alpha) * da + alpha * db) + delta * abs(da - db)
    print("pair", float(out), want, da, db)
    assert abs(float(out) - want) <= LOSS_TOL * want
    pair_a = bio._pair["ta"].clone()
    bio.set_crop(M_P, target=M_B, target_b=M_A)                     # after set_target_pair: both are embedded again
    assert not torch.equal(bio._pair["ta"], pair_a)
    bio.distance_into(out, pred, scale=2.0)
    da, db = d(ep, _embed(net, ta, M_B)), d(ep, _embed(net, tb, M_A))
    want = 2.0 * ((1 - alpha) * da + alpha * db) + delta * abs(da - db)
    assert abs(float(out) - want) <= LOSS_TOL * want
    with pytest.raises(_lib.MgfError, match="takes no face crop"):
        BiometricLoss("facenet").set_crop(M_P)


def test_set_crop_and_a_remembered_target(nets):
    """set_crop re-embeds a remembered target only when the new matrices can apply to it, changes nothing when it refuses a matrix, and
    forget_target() spares the re-embedding."""
    from morphganformer_amd import _lib
    from morphganformer_amd.biometric import BiometricLoss
    net = nets["mobilefacenet"]
    t3, pred = _rand((3, 3, 96, 96), 51).cuda(), _rand((2, 3, 96, 96), 52).cuda()
    three, two = torch.stack([M_A, M_B, M_A]), torch.stack([M_B, M_A])
    bio = BiometricLoss(net.clone_for(3))
    bio.set_crop(three)
    bio.set_target(t3)
    kept = bio._target.clone()
    # a refused matrix (target_b is singular) leaves everything as it was
    with pytest.raises(_lib.MgfError, match="singular"):
        bio.set_crop(two, target_b=[[1.0, 2.0, 0.0], [2.0, 4.0, 0.0]])
    assert torch.equal(bio.embedder._crop[0].cpu(), three) and torch.equal(bio._target, kept) and bio._crop["target"] is three
    # two matrices cannot apply to the three remembered targets (the next lockstep group of another size): dropped, not embedded, not an error
    bio.set_crop(two)
    assert bio._target is None and bio._target_src is None
    with pytest.raises(AssertionError, match="set_target"):
        bio.distance_into(torch.zeros(2, device="cuda"), pred)
    bio.set_target(pred)
    assert tuple(bio._target.shape) == (2, 512)
    # one shared target matrix applies to any remembered target
    bio.set_crop(two, target=M_A)
    want = torch.cat([_embed(net, pred[j:j + 1], M_A) for j in range(2)])
    assert float((bio._target.double().cpu() - want).abs().max()) <= ENGINE_TOL * float(want.abs().max())     # (a batch of 2 against 1 + 1)
    # forget_target: the embeddings stay, nothing is embedded again
    before = bio._target.clone()
    bio.forget_target()
    bio.set_crop(two, target=M_B)
    assert torch.equal(bio._target, before)


# ------------------------------------------------------------------------------------------------------------------ engines and drivers
@pytest.fixture(scope="module")
def tiny():
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import TINY, make_state_dict
    return Generator(make_state_dict(TINY, seed=0), TINY, "cuda", max_batch=4), TINY


# the tiny generator draws 64 x 64 images: these crops up-sample (S = 1); the large S is covered by the kernel cases above
T_A, T_B, T_C = similarity(0.45, 3.0, 6.0, 5.0), similarity(0.4, -5.0, 9.0, 8.0), similarity(0.5, 0.0, 4.0, 4.0)


def _setup(G, cfg, steps, targets=1, seed=5):
    torch.manual_seed(seed)
    latent_mean = torch.randn(cfg.k, cfg.z_dim, device="cuda")
    eps = torch.randn(steps, targets, cfg.k, cfg.z_dim, device="cuda")
    target = G(torch.randn(targets, cfg.k, cfg.z_dim, device="cuda"), None, noise_mode="const")[0].clamp(-1, 1).clone()
    return latent_mean, eps, target


def _one_at_a_time(net, imgs, target, pred_m, target_m, gamma):
    from morphganformer_amd.biometric import BiometricLoss
    bio = BiometricLoss(net.clone_for(1))
    bio.set_crop(pred_m, target=target_m)
    bio.set_target(target)
    out = torch.zeros(1, device="cuda")
    return np.array([float(bio.distance_into(out, imgs[i:i + 1].contiguous(), scale=gamma)) for i in range(imgs.shape[0])])


# engine vs one candidate at a time: the same float32 kernels at another batch size; a convolution's sum order may differ with the batch
# (~sqrt(K) 2^-24 per layer over ~50 layers), far below 1e-4 of the loss
ENGINE_TOL = 1e-4


def test_literal_engine_with_a_face_crop(tiny, nets):
    from morphganformer_amd.biometric import BiometricLoss
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine
    G, cfg = tiny
    net = nets["mobilefacenet"]
    steps, gamma = 8, 3.0
    latent_mean, eps, target = _setup(G, cfg, steps)
    args = ProjectionArgs(step=steps, min_loss_init=1e30)
    kw = dict(eps=eps, noise_mode="const", batch=4, gamma=gamma, use_mse=False, use_graph=True)
    eng = ProjectionEngine(G, target, latent_mean, 1.0, args, biometric=BiometricLoss(net.clone_for(4)), face_crop=T_A, face_crop_target=T_B, **kw)
    losses = eng.run().result()[3]
    lats = latent_mean[None] + eps[:, 0] * eng.sigma[:steps].reshape(-1, 1, 1)
    imgs = torch.cat([G(lats[i:i + 4].contiguous(), None, noise_mode="const")[0] for i in range(0, steps, 4)])
    ref = _one_at_a_time(net, imgs, target, T_A, T_B, gamma)
    print("literal", np.abs(losses - ref).max() / np.abs(ref).max())
    assert np.all(np.abs(losses - ref) <= ENGINE_TOL * np.abs(ref))
    plain = ProjectionEngine(G, target, latent_mean, 1.0, args, biometric=BiometricLoss(net.clone_for(4)), **kw).run().result()[3]
    assert np.abs(plain - losses).max() > 1e-2 * np.abs(losses).max()            # the crop is what was scored
    with pytest.raises(ValueError, match="biometric"):
        ProjectionEngine(G, target, latent_mean, 1.0, args, eps=eps, face_crop=T_A)
    with pytest.raises(ValueError, match="need face_crop"):
        ProjectionEngine(G, target, latent_mean, 1.0, args, eps=eps, biometric=BiometricLoss(net.clone_for(1)), face_crop_target=T_A)


def _reset_adam(eng):
    eng.exp_avg.zero_()
    eng.exp_avg_sq.zero_()
    eng.adam_t.zero_()


def test_gradient_engine_with_a_face_crop_and_retarget_under_a_graph(tiny, nets):
    """Step 0 scores the start latent's candidate, and so does step 1 with its own noise: the learning rate is 0 on step 0 of the ramp, so the
    latent has not moved yet.  A captured engine re-targeted to another target with ANOTHER matrix gives
    the bits of a fresh engine: the graph reads the matrices from the buffer set_crop rewrites in place."""
    from morphganformer_amd.biometric import BiometricLoss
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs
    G, cfg = tiny
    net = nets["mobilefacenet"]
    steps, gamma = 5, 10.0
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.25, min_loss_init=1e30)
    m1, e1, t1 = _setup(G, cfg, steps, seed=8)
    m2, e2, t2 = _setup(G, cfg, steps, seed=9)
    make = lambda t, m, e, crop, crop_t: GradientProjectionEngine(G, t, m, 1.0, args, eps=e, noise_mode="const", use_graph=True, use_mse=False,
                                                                  biometric=BiometricLoss(net.clone_for(1)), gamma=gamma, face_crop=crop,
                                                                  face_crop_target=crop_t)
    eng = make(t1, m1, e1, T_A, T_B).run()
    lat1, _, _, losses1 = eng.result()
    assert eng.graph is not None and np.isfinite(losses1).all()
    img0 = G((m1[None] + e1[0] * eng.sigma[0]).contiguous(), None, noise_mode="const")[0]
    ref0 = _one_at_a_time(net, img0, t1, T_A, T_B, gamma)[0]
    print("gradient step 0", losses1[0], ref0)
    assert abs(losses1[0] - ref0) <= ENGINE_TOL * ref0
    assert float(eng.lr_table[0]) == 0.0 and float(eng.lr_table[1]) > 0.0
    img1 = G((m1[None] + e1[1] * eng.sigma[1]).contiguous(), None, noise_mode="const")[0]
    ref1 = _one_at_a_time(net, img1, t1, T_A, T_B, gamma)[0]
    print("gradient step 1", losses1[1], ref1)
    assert abs(losses1[1] - ref1) <= ENGINE_TOL * ref1 and abs(ref1 - ref0) > 1e-3 * ref0
    assert float((eng.latent_in.reshape(-1) - m1.reshape(-1)).abs().max()) > 1e-3           # the identity gradient moved the latent
    plain = GradientProjectionEngine(G, t1, m1, 1.0, args, eps=e1, noise_mode="const", use_graph=True, use_mse=False,
                                     biometric=BiometricLoss(net.clone_for(1)), gamma=gamma).run().result()[3]
    assert abs(plain[0] - losses1[0]) > 1e-2 * abs(losses1[0])
    graph, buf = eng.graph, eng.biometric.embedder._crop[0]
    _reset_adam(eng)                                   # (retarget keeps the Adam moments of the run before; a fresh engine starts from zero)
    eng.retarget(t2, eps=e2, latent_mean=m2, face_crop=T_C, face_crop_target=T_A)
    lat2, step2, loss2, losses2 = eng.run().result()
    assert eng.graph is graph and eng.biometric.embedder._crop[0] is buf and torch.equal(buf.cpu()[0], T_C)
    f_lat, f_step, f_loss, f_losses = make(t2, m2, e2, T_C, T_A).run().result()
    assert np.array_equal(losses2, f_losses) and torch.equal(lat2, f_lat) and step2 == f_step and loss2 == f_loss
    assert not np.array_equal(losses2, losses1)


def _landmarks68(M, seed):
    """A [68,2] set whose five ArcFace points are the template under M (the eye rings average to the eye centres)."""
    from morphganformer_amd.drivers import ARCFACE_TEMPLATE
    M = M.numpy()
    five = ARCFACE_TEMPLATE @ M[:, :2].T + M[:, 2]
    rng = np.random.default_rng(seed)
    lm = rng.uniform(4, 60, (68, 2))
    for rows, centre in ((slice(36, 42), five[0]), (slice(42, 48), five[1])):
        ring = rng.standard_normal((6, 2))
        lm[rows] = centre + ring - ring.mean(0)
    lm[30], lm[48], lm[54] = five[2], five[3], five[4]
    return lm


def test_refine_morph_with_landmark_crops(tiny, nets):
    from morphganformer_amd import drivers
    from morphganformer_amd.biometric import BiometricLoss
    from morphganformer_amd.projection import ProjectionArgs
    G, cfg = tiny
    net = nets["mobilefacenet"]
    steps, alphas = 4, (0.25, 0.5)
    gen = torch.Generator(device="cuda").manual_seed(77)
    z = torch.randn(2, cfg.k, cfg.z_dim, device="cuda", generator=gen)
    img = G(z, None, noise_mode="const")[0].clamp(-1, 1).clone()
    ta, tb = img[0:1].contiguous(), img[1:2].contiguous()
    lm_a, lm_b = _landmarks68(T_A, 1), _landmarks68(T_B, 2)
    assert np.abs(drivers.arcface_crop(lm_a) - T_A.numpy()).max() < 1e-9
    lm_steps = np.stack([0.5 * (lm_a + lm_b)] * steps)
    kw = dict(args=ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.25, min_loss_init=1e30), latent_std=1.0, seed=4, noise_mode="const", gamma=5.0,
              id_balance=0.5, lm_target=lm_a, lm_target_b=lm_b, lm_steps=lm_steps)
    w1, w2 = z[0:1].cpu().numpy(), z[1:2].cpu().numpy()
    plain = drivers.refine_morph(G, w1, w2, ta, tb, alphas, biometric=BiometricLoss(net.clone_for(2)), **kw)
    bio = BiometricLoss(net.clone_for(2))
    res = drivers.refine_morph(G, w1, w2, ta, tb, alphas, biometric=bio, face_crop="landmarks", face_crop_b="landmarks", **kw)
    for r, p in zip(res, plain):
        print(r["alpha"], r["id_distances"], p["id_distances"])
        assert np.isfinite(r["id_distances"]).all() and np.isfinite(r["losses"]).all()
        assert abs(r["id_distances"][0] - p["id_distances"][0]) > 1e-3 * abs(p["id_distances"][0])
    # the candidates' matrices follow the blended landmarks, the targets' their own
    pred = bio.embedder._crop[0].cpu().numpy()
    assert pred.shape == (2, 2, 3)
    for j, a in enumerate(alphas):
        assert np.abs(pred[j] - drivers.arcface_crop((1 - a) * lm_a + a * lm_b)).max() < 1e-12
    assert np.abs(bio._crop["target"] - T_A.numpy()).max() < 1e-9 and np.abs(bio._crop["target_b"] - T_B.numpy()).max() < 1e-9
    with pytest.raises(ValueError, match="biometric"):
        drivers.refine_morph(G, w1, w2, ta, tb, alphas, face_crop=T_A, **{k: v for k, v in kw.items() if k != "id_balance"})


def test_project_many_lockstep_groups_with_face_crops(tiny, nets):
    """project_many(mode='gradient', lockstep=3) over 5 items: a group of three and a group of two share one BiometricLoss, each group gets its
    items' matrices as one stack, and every item's result is that of a single project_image call with its own crop and its column of the
    group's noise.

    The comparison runs at lr = 0: the whole backward pass runs, Adam scales its step by zero, so every step's candidate is known and the two
    sides differ only by the embedder's float32 rounding at batch 3 against batch 1 (ENGINE_TOL; measured 1e-6 on every step).  Once the latent
    moves no bound can be derived: Adam's first steps are lr * sign(g), discontinuous where a gradient entry is near zero, so that rounding sends
    the two runs down different trajectories -- measured 2e-2 of the loss by step 3, with the crop and equally with the plain resize.  The
    descending run is therefore checked for what is determined: it runs, is finite, and leaves the start."""
    from morphganformer_amd import drivers
    from morphganformer_amd.biometric import BiometricLoss
    from morphganformer_amd.projection import ProjectionArgs
    G, cfg = tiny
    net = nets["mobilefacenet"]
    steps, seed = 4, 21
    torch.manual_seed(13)
    targets = [G(torch.randn(1, cfg.k, cfg.z_dim, device="cuda"), None, noise_mode="const")[0].clamp(-1, 1).clone() for _ in range(5)]
    crops = [T_A, T_B.numpy(), T_C, similarity(0.42, 8.0, 7.0, 3.0), similarity(0.48, -2.0, 3.0, 6.0)]
    latent_mean = torch.randn(cfg.k, cfg.z_dim, device="cuda")
    kw = dict(args=ProjectionArgs(step=steps, lr=0.0, min_loss_init=1e30), mode="gradient", noise_mode="const", use_mse=False,
              gamma=2.0, latent_mean=latent_mean, latent_std=1.0)
    bio = BiometricLoss(net.clone_for(3))
    many = drivers.project_many(G, targets, lockstep=3, face_crops=crops, biometric=bio, seed=seed, **kw)
    assert many["items"].tolist() == [0, 1, 2, 3, 4]
    assert tuple(bio.embedder._crop[0].shape) == (2, 2, 3) and torch.equal(bio.embedder._crop[0].cpu()[1], crops[4])     # the last group's stack
    for ids in ([0, 1, 2], [3, 4]):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        eps = torch.randn(steps, len(ids), cfg.k, cfg.z_dim, device="cuda", generator=gen)          # the group engine's own draw
        for col, j in enumerate(ids):
            one = drivers.project_image(G, targets[j], None, None, face_crop=crops[j], biometric=BiometricLoss(net.clone_for(1)),
                                        eps=eps[:, col:col + 1].contiguous(), **kw)
            print("item", j, float(many["losses"][j]), one["loss"], int(many["steps"][j]), one["step"])
            assert int(many["steps"][j]) == one["step"], j
            assert abs(float(many["losses"][j]) - one["loss"]) <= ENGINE_TOL * abs(one["loss"]), j
    assert len({float(v) for v in many["losses"]}) == 5
    moving = drivers.project_many(G, targets, lockstep=3, face_crops=crops, biometric=bio, seed=seed,
                                  **dict(kw, args=ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.25, min_loss_init=1e30)))
    assert np.isfinite(np.asarray(moving["losses"].cpu(), dtype=np.float64)).all() and not torch.equal(moving["latents"], many["latents"])


def test_project_many_with_face_crops(tiny, nets):
    """One re-targeted engine walked over three items, each with its own crop, equals three single project_image calls."""
    from morphganformer_amd import drivers
    from morphganformer_amd.biometric import BiometricLoss
    from morphganformer_amd.projection import ProjectionArgs
    G, cfg = tiny
    net = nets["mobilefacenet"]
    steps = 8
    torch.manual_seed(12)
    targets = [G(torch.randn(1, cfg.k, cfg.z_dim, device="cuda"), None, noise_mode="const")[0].clamp(-1, 1).clone() for _ in range(3)]
    crops = [T_A.numpy(), T_B, T_C]
    latent_mean = torch.randn(cfg.k, cfg.z_dim, device="cuda")
    kw = dict(args=ProjectionArgs(step=steps, min_loss_init=1e30), batch=4, seed=21, noise_mode="const", use_mse=False, gamma=2.0,
              latent_mean=latent_mean, latent_std=1.0)
    many = drivers.project_many(G, targets, face_crops=crops, biometric=BiometricLoss(net.clone_for(4)), **kw)
    for j in range(3):
        one = drivers.project_image(G, targets[j], None, None, face_crop=crops[j], biometric=BiometricLoss(net.clone_for(4)), **kw)
        assert float(many["losses"][j]) == one["loss"] and int(many["steps"][j]) == one["step"], j
        assert torch.equal(many["latents"][j].cpu().float(), one["w"].reshape(many["latents"][j].shape).cpu().float()), j
    assert len({float(v) for v in many["losses"]}) == 3
    with pytest.raises(ValueError, match="face crops"):
        drivers.project_many(G, targets, face_crops=crops[:2], biometric=BiometricLoss(net.clone_for(4)), **kw)
    # an engine built without a crop is not handed one later
    eng = drivers.project_image(G, targets[0], None, None, biometric=BiometricLoss(net.clone_for(4)), return_engine=True, **kw)["engine"]
    with pytest.raises(ValueError, match="face_crop"):
        drivers.project_image(G, targets[1], None, None, biometric=eng.biometric, engine=eng, face_crop=T_A, **kw)
    # pool_above: the driver re-expresses the matrix for the pooled image the losses see
    pooled_target = torch.nn.functional.avg_pool2d(targets[0], 2)
    pk = dict(kw, args=ProjectionArgs(step=steps, min_loss_init=1e30, pool_above=32))
    bio = BiometricLoss(net.clone_for(4))
    drivers.project_image(G, pooled_target, None, None, face_crop=T_A, biometric=bio, **pk)
    assert np.abs(bio.embedder._crop[0].cpu().numpy()[0] - drivers.scale_crop(T_A, 2)).max() == 0.0
