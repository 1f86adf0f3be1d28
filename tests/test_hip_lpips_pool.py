"""PerceptualLoss(pool_above=N): the two kernels of csrc/block_pool.hip against float64 at the bounds their arithmetic
gives (tests/lpips_pool_torch_ref.py), and the LPIPS term with its own block mean -- value, gradient, target pair, region weight, refusals --
against the oracle's LPIPS on the float64-pooled images.  Tolerances of the term are the ones the un-pooled term is held to: 1e-4 for a
value through the backbone and GRAD_TOL for its gradient (tests/test_hip_gradient.py)."""
import os

import numpy as np
import pytest
import torch

from guarded_buffers import Guarded
from lpips_pool_torch_ref import U, block_mean_adjoint_bound, block_mean_adjoint_ref, block_mean_bound, block_mean_ref
from region_weight_torch_ref import lpips_weighted_ref, weights

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-3        # tests/test_hip_gradient.py's gate on gradients

# (planes, h, w, f): the smallest shapes at which the bodies differ -- the smallest input, odd output widths (f = 2 with w % 4 != 0: the scalar
# body), a generic f with an inexact 1 / f^2, the three vector bodies, a 5 x 3 output, more than one workgroup
SHAPES = [(1, 2, 2, 2), (3, 8, 8, 4), (5, 6, 10, 2), (2, 12, 12, 3), (6, 64, 64, 2), (6, 64, 64, 4), (3, 64, 64, 8), (7, 40, 24, 8), (6, 128, 128, 4)]


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _input(kind, planes, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(planes, h, w, generator=g)
    if kind == "cancel":                     # every block holds +m and -m (m around 1000, not a round number) beside small values: the sum
        m = 1000.0 + 500.0 * torch.rand(planes, h, w // 2, generator=g)              # cancels, mean |x| does not
        x = x * 1e-3
        x[:, :, 0::2] += m
        x[:, :, 1::2] -= m
    return x.float()


def _pool(x_guarded, planes, h, w, f, out_offset=0):
    from morphganformer_amd import _lib
    out = Guarded((planes, h // f, w // f), None, offset=out_offset)
    _lib.check(_lib.lib().mgf_block_mean_f32(out.ptr(), x_guarded.ptr(), planes, h, w, f, _lib.stream_ptr()), "block_mean")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("planes,h,w,f", SHAPES)
def test_block_mean_against_float64(planes, h, w, f):
    """|out - exact| <= (f^2 + 1) 2^-24 mean_block |x| per pixel, for an aligned base pointer and for one offset by a float (the 16-byte
    body must fall back) -- and, as include/mgf.h states one summation order, the same bits from both."""
    for kind in ("randn", "cancel"):
        x = _input(kind, planes, h, w, seed=planes * 1000 + h + f)
        exact = block_mean_ref(x[None], f)[0]
        bound = block_mean_bound(x[None], f)[0]
        outs = []
        for x_off, o_off in ((0, 0), (1, 1), (0, 1)):
            xin = Guarded((planes, h, w), x, offset=x_off)
            out = _pool(xin, planes, h, w, f, out_offset=o_off)
            assert out.written() and out.guard_intact() and bool(torch.isnan(out.buf[:o_off]).all())
            err = (out.t.double().cpu() - exact).abs()
            print(f"OBS block_mean {kind} {(planes, h, w, f)} offsets {(x_off, o_off)}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
            assert bool((err <= bound).all())
            outs.append(out.t.clone())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("h,w,f", [(64, 64, 4), (6, 10, 2), (40, 24, 8), (12, 12, 3), (64, 64, 2)])
def test_block_mean_is_batch_invariant(h, w, f):
    """planes = 3 alone and as rows 0-2 of planes = 96: equal bits."""
    x = _input("randn", 96, h, w, seed=h + f)
    alone = _pool(Guarded((3, h, w), x[:3]), 3, h, w, f)
    batch = _pool(Guarded((96, h, w), x), 96, h, w, f)
    assert torch.equal(alone.t, batch.t[:3])


def _crops(h, w, f):
    full = (h // f, w // f)
    return sorted({full, (max(full[0] - 1, 1), max(full[1] - 1, 1)), (1, 1)})


@pytest.mark.parametrize("planes,h,w,f", SHAPES)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_block_mean_adjoint_against_float64(planes, h, w, f, accumulate):
    """dx against P^T dy in float64: |dx - exact| <= 2 2^-24 |dy| / f^2 (+ 2^-24 |result| when accumulating); dy full, cropped by one and
    1 x 1, contiguous and as a view with a larger pitch and plane stride inside a NaN-filled buffer; dx aligned and offset by a float;
    the pixels no dy covers are exactly 0 (accumulate = 0) or exactly the 0.25 they held (accumulate = 1)."""
    from morphganformer_amd import _lib
    L = _lib.lib()
    for gh, gw in _crops(h, w, f):
        for strided in (False, True):
            for off in (0, 1):
                g = torch.Generator().manual_seed(gh * 100 + gw + planes)
                dy = torch.randn(planes, gh, gw, generator=g).float()
                if strided:
                    big = torch.full((planes, gh + 1, gw + 3), float("nan"), device="cuda")
                    view = big[:, :gh, :gw]
                    view.copy_(dy)
                else:
                    view = dy.cuda().contiguous()
                dx = Guarded((planes, h, w), torch.full((planes, h, w), 0.25), offset=off)
                _lib.check(L.mgf_block_mean_adjoint_f32(dx.ptr(), view.data_ptr(), planes, h, w, f, gh, gw, view.stride(1), view.stride(0), accumulate,
                                                        _lib.stream_ptr()), "block_mean_adjoint")
                torch.cuda.synchronize()
                assert dx.written() and dx.guard_intact() and bool(torch.isnan(dx.buf[:off]).all())
                got = dx.t.double().cpu()
                exact = block_mean_adjoint_ref(dy[None], f, h, w)[0] + (0.25 if accumulate else 0.0)
                bound = block_mean_adjoint_bound(dy[None], f, h, w, result=exact[None] if accumulate else None)[0]
                assert bool(((got - exact).abs() <= bound).all()), (gh, gw, strided, off)
                rest = torch.ones(h, w, dtype=torch.bool)
                rest[:gh * f, :gw * f] = False
                assert bool((got[:, rest] == (0.25 if accumulate else 0.0)).all()), (gh, gw, strided, off)


@pytest.mark.parametrize("planes,h,w,f", SHAPES)
def test_dot_product_identity_of_the_two_kernels(planes, h, w, f):
    """|<P x, y> - <x, P^T y>| from the two kernels' outputs, in float64, within what their two bounds allow."""
    from morphganformer_amd import _lib
    x = _input("randn", planes, h, w, seed=7 * h + f)
    g = torch.Generator().manual_seed(h + w + f)
    y = torch.randn(planes, h // f, w // f, generator=g).float()
    px = _pool(Guarded((planes, h, w), x), planes, h, w, f).t.double().cpu()
    dx = Guarded((planes, h, w), None)
    yc = y.cuda()
    _lib.check(_lib.lib().mgf_block_mean_adjoint_f32(dx.ptr(), yc.data_ptr(), planes, h, w, f, h // f, w // f, w // f, (h // f) * (w // f), 0,
                                                     _lib.stream_ptr()), "block_mean_adjoint")
    torch.cuda.synchronize()
    lhs = float((px * y.double()).sum())
    rhs = float((x.double() * dx.t.double().cpu()).sum())
    allowed = float((y.double().abs() * block_mean_bound(x[None], f)[0]).sum() + (x.double().abs() * block_mean_adjoint_bound(y[None], f, h, w)[0]).sum())
    print(f"OBS dot identity {(planes, h, w, f)}: |lhs - rhs| {abs(lhs - rhs):.3e} allowed {allowed:.3e}")
    assert abs(lhs - rhs) <= allowed


def test_bad_arguments_are_refused_and_launch_nothing():
    from morphganformer_amd import _lib
    L = _lib.lib()
    st = _lib.stream_ptr()
    x = Guarded((3, 8, 8), torch.ones(3, 8, 8))
    out = Guarded((3, 8, 8), None)
    dy = torch.ones(3, 4, 4, device="cuda")
    calls = {
        "f = 1": (lambda: L.mgf_block_mean_f32(out.ptr(), x.ptr(), 3, 8, 8, 1, st), "f must be >= 2"),
        "h % f": (lambda: L.mgf_block_mean_f32(out.ptr(), x.ptr(), 4, 6, 8, 4, st), "whole number"),
        "planes": (lambda: L.mgf_block_mean_f32(out.ptr(), x.ptr(), 2 ** 31 // 64 + 1, 8, 8, 2, st), "32-bit index"),
        "adjoint f = 1": (lambda: L.mgf_block_mean_adjoint_f32(out.ptr(), dy.data_ptr(), 3, 8, 8, 1, 4, 4, 4, 16, 0, st), "f must be >= 2"),
        "adjoint w % f": (lambda: L.mgf_block_mean_adjoint_f32(out.ptr(), dy.data_ptr(), 4, 8, 6, 4, 1, 1, 4, 16, 0, st), "whole number"),
        "adjoint gh": (lambda: L.mgf_block_mean_adjoint_f32(out.ptr(), dy.data_ptr(), 3, 8, 8, 2, 5, 4, 4, 16, 0, st), "extent 5 x 4"),
        "adjoint gw": (lambda: L.mgf_block_mean_adjoint_f32(out.ptr(), dy.data_ptr(), 3, 8, 8, 2, 4, 5, 5, 20, 0, st), "extent 4 x 5"),
        "adjoint pitch": (lambda: L.mgf_block_mean_adjoint_f32(out.ptr(), dy.data_ptr(), 3, 8, 8, 2, 4, 4, 3, 16, 0, st), "row pitch"),
        "adjoint planes": (lambda: L.mgf_block_mean_adjoint_f32(out.ptr(), dy.data_ptr(), 2 ** 31 // 64 + 1, 8, 8, 2, 4, 4, 4, 16, 0, st), "32-bit index"),
    }
    for name, (call, message) in calls.items():
        assert call() == _lib.MGF_EINVAL, name
        assert message in L.mgf_last_error().decode(), (name, L.mgf_last_error().decode())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.buf).all())                     # nothing ran: the output is still all NaN


# ------------------------------------------------------------------------------------------------------------------ the term
def _lins(net):
    from morphganformer_amd.lpips import WEIGHTS_DIR
    lin = np.load(os.path.join(WEIGHTS_DIR, f"lpips_lin_{net}.npz"))
    return [torch.from_numpy(lin[f"lin{i}"]).float().reshape(-1) for i in range(len(lin.files))]


def _device_pool(img, f):
    """mgf_block_mean_f32 of a device image [n,3,H,W] -> a new [n,3,H/f,W/f]."""
    from morphganformer_amd import _lib
    n, c, H, W = img.shape
    out = torch.empty(n, c, H // f, W // f, device="cuda")
    _lib.check(_lib.lib().mgf_block_mean_f32(out.data_ptr(), img.contiguous().data_ptr(), n * c, H, W, f, _lib.stream_ptr()), "block_mean")
    return out


@pytest.mark.parametrize("net,size,pool_above", [("squeeze", 64, 32), ("squeeze", 128, 32), ("vgg", 96, 48)])
def test_pooled_term_value_and_gradient(net, size, pool_above):
    """distance_into under pool_above: the bits of a plain PerceptualLoss handed mgf_block_mean_f32's output, and lpips_ref of the
    float64-pooled images within 1e-4; grad_into against autograd through lpips_ref o pool with respect to the FULL-size image at GRAD_TOL,
    scale 0.7, with and without accumulate; the buffers of the pooled images are allocated once."""
    from morphganformer_amd.lpips import PerceptualLoss
    from oracle.loss_ref import backbone_random, lpips_ref
    torch.manual_seed(size)
    n, f = 2, size // pool_above
    pred = (torch.rand(n, 3, size, size) * 2 - 1).requires_grad_(True)
    target = torch.rand(1, 3, size, size) * 2 - 1
    bb, lins = backbone_random(net, 0), _lins(net)
    val = lpips_ref(bb, lins, block_mean_ref(pred, f).float(), block_mean_ref(target, f).float().expand(n, -1, -1, -1), net=net)
    (ref,) = torch.autograd.grad(val.sum() * 0.7, pred)
    pl = PerceptualLoss(net=net, allow_random_backbone=True, pool_above=pool_above)
    plain = PerceptualLoss(net=net, allow_random_backbone=True)
    pc, tc = pred.detach().cuda(), target.cuda()
    pl.set_target(tc)
    plain.set_target(_device_pool(tc, f))
    out, out_plain = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    for keep in (False, True):
        pl.distance_into(out, pc, keep_taps=keep)
        plain.distance_into(out_plain, _device_pool(pc, f), keep_taps=keep)
        assert torch.equal(out, out_plain), keep
        print(f"OBS pooled value {net} {size} keep_taps={keep}: rel {rel(out, val.reshape(n)):.3e}")
        assert rel(out, val.reshape(n)) < 1e-4
    assert torch.equal(pl.distance_per_tap(pc), plain.distance_per_tap(_device_pool(pc, f)))
    single = pl(pc[:1], tc)
    assert tuple(single.shape) == (1, 1, 1, 1) and rel(single.reshape(1), val.reshape(n)[:1]) < 1e-4
    pl.set_target(tc)
    pl.distance_into(out, pc, keep_taps=True)
    buffers = {k: v.data_ptr() for k, v in pl._pooled.items()}
    assert sorted(buffers) == [(1, size, size), (n, size, size)]
    dimg = torch.full((n, 3, size, size), 0.25, device="cuda")
    pl.grad_into(dimg, scale=0.7, accumulate=True)
    print(f"OBS pooled gradient {net} {size}: accumulate rel {rel(dimg - 0.25, ref):.3e}")
    assert rel(dimg - 0.25, ref) < GRAD_TOL
    acc = dimg.clone()
    pl.grad_into(dimg, scale=0.7)
    print(f"OBS pooled gradient {net} {size}: rel {rel(dimg, ref):.3e}")
    assert rel(dimg, ref) < GRAD_TOL
    if net == "squeeze" and size == 64:
        # the stride-2 stem never reads row / column 31 of the 32^2 image: no gradient on rows and columns 62, 63 of the full-size one
        edge = torch.zeros(64, 64, dtype=torch.bool)
        edge[62:], edge[:, 62:] = True, True
        assert float(ref[:, :, edge].abs().max()) == 0.0
        assert bool((dimg[:, :, edge.cuda()] == 0.0).all()) and bool((acc[:, :, edge.cuda()] == 0.25).all())
        for i in (60, 61):
            for grad in (ref, dimg):
                assert float(grad[:, :, i, :].abs().max()) > 0.0 and float(grad[:, :, :, i].abs().max()) > 0.0
    pl.distance_into(out, pc, keep_taps=True)
    assert {k: v.data_ptr() for k, v in pl._pooled.items()} == buffers
    with pytest.raises(AssertionError):
        pl.grad_into(torch.empty(n, 3, size // f, size // f, device="cuda"))           # dimg has the size of the image handed in


def test_pool_above_leaves_small_images_alone():
    """An image at or below pool_above (one ProjectionArgs.pool_above already pooled, say) goes through untouched: the plain term's bits."""
    from morphganformer_amd.lpips import PerceptualLoss
    torch.manual_seed(3)
    pred, target = (torch.rand(2, 3, 64, 64) * 2 - 1).cuda(), (torch.rand(1, 3, 64, 64) * 2 - 1).cuda()
    outs = []
    for pa in (0, 64, 100):
        pl = PerceptualLoss(net="squeeze", allow_random_backbone=True, pool_above=pa)
        pl.set_target(target)
        out = pl.distance_into(torch.empty(2, device="cuda"), pred, keep_taps=True).clone()
        outs.append((out, pl.grad_into(torch.empty(2, 3, 64, 64, device="cuda")).clone()))
        assert not pl._pooled
    assert all(torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs)


def test_pooled_target_pair():
    """set_target_pair at alpha = 0.3 on 64^2 with pool_above = 32: distance_into + pair_offset against the two-target sum on the pooled
    images (1e-4, the gate of test_perceptual_pair_matches_the_explicit_two_target_sum), its gradient at GRAD_TOL."""
    from morphganformer_amd.lpips import PerceptualLoss
    from oracle.loss_ref import backbone_random, lpips_ref
    torch.manual_seed(64)
    n, size, f, alpha = 1, 64, 2, 0.3
    pred = (torch.rand(n, 3, size, size) * 2 - 1).requires_grad_(True)
    ta, tb = torch.rand(n, 3, size, size) * 2 - 1, torch.rand(n, 3, size, size) * 2 - 1
    bb, lins = backbone_random("squeeze", 0), _lins("squeeze")
    pool = lambda t: block_mean_ref(t, f).float()
    val = (1 - alpha) * lpips_ref(bb, lins, pool(pred), pool(ta)).reshape(n) + alpha * lpips_ref(bb, lins, pool(pred), pool(tb)).reshape(n)
    (ref,) = torch.autograd.grad(val.sum() * 0.7, pred)
    pl = PerceptualLoss(net="squeeze", allow_random_backbone=True, pool_above=32)
    pl.set_target_pair(ta.cuda(), tb.cuda(), alpha)
    out = torch.empty(n, device="cuda")
    pl.distance_into(out, pred.detach().cuda(), keep_taps=True)
    print("OBS pooled pair value", rel(out + pl.pair_offset, val))
    assert rel(out + pl.pair_offset, val) < 1e-4
    dimg = pl.grad_into(torch.zeros(n, 3, size, size, device="cuda"), scale=0.7)
    print("OBS pooled pair gradient", rel(dimg, ref))
    assert rel(dimg, ref) < GRAD_TOL


def test_pooled_region_weight():
    """A half-plane weight given at 64^2: the weighted float64 helper on the pooled images with the pooled weight (value 1e-4, gradient GRAD_TOL,
    the gates of test_perceptual_loss_with_a_region_weight); a weight at the pooled size is refused."""
    from morphganformer_amd.lpips import PerceptualLoss
    from oracle.loss_ref import backbone_random
    torch.manual_seed(65)
    n, size, f = 2, 64, 2
    pred = (torch.rand(n, 3, size, size) * 2 - 1).requires_grad_(True)
    target = torch.rand(1, 3, size, size) * 2 - 1
    W = weights("half", size, size)
    Wp = block_mean_ref(W[None, None], f)[0, 0]
    bb, lins = backbone_random("squeeze", 0), _lins("squeeze")
    val = lpips_weighted_ref(bb, lins, block_mean_ref(pred, f), block_mean_ref(target, f), Wp)
    (ref,) = torch.autograd.grad(val.sum() * 0.7, pred)
    pl = PerceptualLoss(net="squeeze", allow_random_backbone=True, pool_above=32)
    pl.set_region_weight(W)
    pl.set_target(target.cuda())
    out = pl.distance_into(torch.empty(n, device="cuda"), pred.detach().cuda(), keep_taps=True)
    print("OBS pooled region value", rel(out, val))
    assert rel(out, val) < 1e-4
    dimg = pl.grad_into(torch.empty(n, 3, size, size, device="cuda"), scale=0.7)
    print("OBS pooled region gradient", rel(dimg, ref))
    assert rel(dimg, ref) < GRAD_TOL
    pl.set_region_weight(Wp)                                    # at the pooled size: not the size of the images handed in
    with pytest.raises(ValueError, match="32x32"):
        pl.distance_into(out, pred.detach().cuda())
    pl.set_region_weight(None)
    plain = PerceptualLoss(net="squeeze", allow_random_backbone=True, pool_above=32)
    plain.set_target(target.cuda())
    assert torch.equal(pl.distance_into(out, pred.detach().cuda()), plain.distance_into(torch.empty(n, device="cuda"), pred.detach().cuda()))


def test_refusals_of_the_pooled_term():
    from morphganformer_amd._lib import MgfError
    from morphganformer_amd.lpips import PerceptualLoss
    with pytest.raises(MgfError, match="the map is defined at the image's own size"):
        PerceptualLoss(net="squeeze", allow_random_backbone=True, spatial=True, pool_above=32)
    pl = PerceptualLoss(net="squeeze", allow_random_backbone=True, pool_above=32)
    pl.set_target(torch.zeros(1, 3, 66, 66, device="cuda"))     # f = 66 // 32 = 2: 33 x 33 at the backbone
    out = pl.distance_into(torch.empty(1, device="cuda"), torch.ones(1, 3, 66, 66, device="cuda") * 0.5)
    assert bool(torch.isfinite(out).all()) and tuple(pl._pooled[(1, 66, 66)].shape) == (1, 3, 33, 33)
    with pytest.raises(MgfError, match="65x65"):
        pl.set_target(torch.zeros(1, 3, 65, 65, device="cuda"))
    with pytest.raises(MgfError, match="64x65"):                # the factor comes from the height; the width must divide too
        pl.set_target(torch.zeros(1, 3, 64, 65, device="cuda"))
