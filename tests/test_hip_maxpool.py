"""The max pools of csrc/maxpool.hip through the C ABI, bit for bit against torch on the CPU: MaxPool2d(3, 2, ceil_mode=True) forward with and
without stored taps, its two backward forms against autograd (torch's first-maximum rule), and the floor-mode pools.

The widths of test_ceil_pool_every_kernel_choice walk the one dispatch of the ceil-mode forward: the generic kernel (3, 63: fewer than 64
columns, a tile row less than half full), the rows kernel with 1..8 slots of 64 columns (64, 65/128, 129/192, 256, 257/320, 384, 448, 449/512, each
slot count at its first and last width where both are listed), the tiled kernel (513, 641; the idx forward has none and takes the generic
kernel there).  Heights 5 and 6: a last window of one row and of two."""
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = [3, 63, 64, 65, 128, 129, 192, 256, 257, 320, 384, 448, 449, 512, 513, 641]
ALL_NEGATIVE = (6, 641)                                                 # this case is shifted below zero: the padding value must never win


def _api():
    from morphganformer_amd import _lib
    return _lib, _lib.lib(), _lib.stream_ptr()


def _ceil_case(x):
    """x [n, c, h, w] on the CPU -> (y, dy, dx) of max_pool2d(x, 3, 2, ceil_mode=True) by torch."""
    x = x.clone().requires_grad_(True)
    y = torch.nn.functional.max_pool2d(x, 3, 2, ceil_mode=True)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(y.numel()))
    (dx,) = torch.autograd.grad(y, x, dy)
    return y.detach(), dy, dx


@pytest.mark.parametrize("in_w", WIDTHS)
@pytest.mark.parametrize("in_h", [5, 6])
def test_ceil_pool_every_kernel_choice(in_h, in_w):
    _lib, L, st = _api()
    x = torch.relu(torch.randn(1, 2, in_h, in_w, generator=torch.Generator().manual_seed(1000 * in_h + in_w)))     # ties: ReLU zeros, also across slot seams
    if (in_h, in_w) == ALL_NEGATIVE:
        x = x - 5.0
    y, dy, ref = _ceil_case(x)
    xd, dyd = x.cuda(), dy.cuda()
    pargs = (2, in_h, in_w, y.shape[2], y.shape[3], st)
    yd, yi = torch.full_like(dyd, float("nan")), torch.full_like(dyd, float("nan"))
    taps = torch.full(dyd.shape, 255, dtype=torch.uint8, device="cuda")
    _lib.check(L.mgf_maxpool3x3s2_ceil_f32(yd.data_ptr(), xd.data_ptr(), *pargs))
    _lib.check(L.mgf_maxpool3x3s2_ceil_idx_f32(yi.data_ptr(), taps.data_ptr(), xd.data_ptr(), *pargs))
    assert torch.equal(yd.cpu(), y)
    assert torch.equal(yi.cpu(), y)
    assert int(taps.max()) <= 8
    dx_idx, dx = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
    _lib.check(L.mgf_maxpool3x3s2_ceil_bwd_idx_f32(dx_idx.data_ptr(), dyd.data_ptr(), taps.data_ptr(), *pargs))
    _lib.check(L.mgf_maxpool3x3s2_ceil_bwd_f32(dx.data_ptr(), dyd.data_ptr(), xd.data_ptr(), *pargs))
    assert torch.equal(dx_idx.cpu(), ref)
    assert torch.equal(dx.cpu(), ref)


@pytest.mark.parametrize("in_w", [65, 257])
@pytest.mark.parametrize("k", [2, 3])
def test_floor_pool_forward_and_backward(k, in_w):
    _lib, L, st = _api()
    for in_h in (5, 6):
        x = torch.relu(torch.randn(1, 2, in_h, in_w, generator=torch.Generator().manual_seed(100 * k + in_h + in_w))).requires_grad_(True)
        y = torch.nn.functional.max_pool2d(x, k, 2)
        dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(7))
        (ref,) = torch.autograd.grad(y, x, dy)
        xd, dyd = x.detach().cuda(), dy.cuda()
        yd, dx = torch.full_like(dyd, float("nan")), torch.full_like(xd, float("nan"))
        _lib.check(L.mgf_maxpool_s2_floor_f32(yd.data_ptr(), xd.data_ptr(), 2, in_h, in_w, k, st))
        _lib.check(L.mgf_maxpool_s2_floor_bwd_f32(dx.data_ptr(), dyd.data_ptr(), xd.data_ptr(), 2, in_h, in_w, k, st))
        assert torch.equal(yd.cpu(), y.detach()), in_h
        assert torch.equal(dx.cpu(), ref), in_h


def test_pool_bwd_ties_and_forward_shapes():
    """Larger planes: several tiles of the backward kernel with ragged edges, several planes, widths past one wave's 128 columns."""
    _lib, L, _ = _api()
    torch.manual_seed(3)
    # ceil-mode pooling with ties (ReLU zeros): the gradient must follow torch's first-maximum rule
    # (one tile; several 64 x 32 tiles with ragged edges, odd and even sides; all-negative inputs: the -inf padding must never win)
    for shape, neg in (((2, 4, 15, 12), False), ((1, 3, 70, 131), False), ((2, 1, 65, 64), False), ((1, 2, 33, 129), True)):
        x = torch.relu(torch.randn(*shape))
        x = (x - 5.0 if neg else x).requires_grad_(True)
        y = torch.nn.functional.max_pool2d(x, 3, 2, ceil_mode=True)
        dy = torch.randn_like(y)
        (ref,) = torch.autograd.grad(y, x, dy)
        xd, dyd = x.detach().cuda(), dy.cuda()
        dx = torch.full_like(xd, float("nan"))
        _lib.check(L.mgf_maxpool3x3s2_ceil_bwd_f32(dx.data_ptr(), dyd.data_ptr(), xd.data_ptr(), shape[0] * shape[1], shape[2], shape[3],
                                                   y.shape[2], y.shape[3], _lib.stream_ptr()))
        assert torch.equal(dx.cpu(), ref), shape
        # the forward that stores each window's winning tap + the backward that reads those: same y as the plain forward, same dx
        yd, yi = torch.empty_like(dyd), torch.empty_like(dyd)
        taps = torch.full(dyd.shape, 255, dtype=torch.uint8, device="cuda")
        pargs = (shape[0] * shape[1], shape[2], shape[3], y.shape[2], y.shape[3], _lib.stream_ptr())
        _lib.check(L.mgf_maxpool3x3s2_ceil_f32(yd.data_ptr(), xd.data_ptr(), *pargs))
        _lib.check(L.mgf_maxpool3x3s2_ceil_idx_f32(yi.data_ptr(), taps.data_ptr(), xd.data_ptr(), *pargs))
        assert torch.equal(yd, yi) and torch.equal(yi.cpu(), y.detach()) and int(taps.max()) <= 8
        dx2 = torch.full_like(xd, float("nan"))
        _lib.check(L.mgf_maxpool3x3s2_ceil_bwd_idx_f32(dx2.data_ptr(), dyd.data_ptr(), taps.data_ptr(), *pargs))
        assert torch.equal(dx2.cpu(), ref), shape
    # forward pooling, both entries, odd and even sides, wider than one wave's 128 columns: bit-exact
    for (c, hh, ww) in ((3, 15, 12), (2, 31, 301), (1, 8, 257), (5, 2, 3)):
        xf = torch.randn(2, c, hh, ww)
        want = torch.nn.functional.max_pool2d(xf, 3, 2, ceil_mode=True)
        got = torch.empty_like(want).cuda()
        _lib.check(L.mgf_maxpool3x3s2_ceil_f32(got.data_ptr(), xf.cuda().data_ptr(), 2 * c, hh, ww, want.shape[2], want.shape[3], _lib.stream_ptr()))
        assert torch.equal(got.cpu(), want)
        for k in (2, 3):
            if hh < k or ww < k:
                continue
            want = torch.nn.functional.max_pool2d(xf, k, 2)
            got = torch.empty_like(want).cuda()
            _lib.check(L.mgf_maxpool_s2_floor_f32(got.data_ptr(), xf.cuda().data_ptr(), 2 * c, hh, ww, k, _lib.stream_ptr()))
            assert torch.equal(got.cpu(), want)
