"""The polyphase Winograd transposed conv (csrc/wino_tconv.hip: mgf_tconv3x3s2_winograd_f32 + mgf_tconv_winograd_weights_f32) against float64
conv_transpose2d, and the dispatch of conv.tconv3x3s2_forward between it and the tap-list kernel."""
import math

import numpy as np
import pytest
import torch


def rel_err(a, b):
    a = a.detach().double().cpu().numpy()
    b = b.detach().double().cpu().numpy()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


T = np.array([[0, 0, 1], [1, 0, 1], [1, 0, 0], [0, 1, 0], [0, 1, 0]], dtype=np.float64)     # weight rows w2, w0 + w2, w0, w1, w1


def _u_ref(w, gain):
    """[25, cin/4, cout, 4] in float64: gain * T w T^T per (co, ci), the chunk's channels in MFMA slot order."""
    cout, cin = w.shape[:2]
    u = np.einsum("rk,oikl,cl->rcoi", T, w.astype(np.float64), T).reshape(25, cout, cin) * gain
    slot_of = [0, 2, 1, 3]                                   # channel c of a chunk sits in slot 2 (c % 2) + c // 2
    out = np.zeros((25, cin // 4, cout, 4))
    for c in range(cin):
        out[:, c // 4, :, slot_of[c % 4]] = u[:, :, c]
    return out


def _launch(x, u, cout, in_scale=None, out_scale=None, fill=float("nan")):
    """The Winograd launch alone (no border kernel, no dispatch predicate) into a NaN-filled workspace."""
    from morphganformer_amd import _lib
    from morphganformer_amd import conv as cv
    n, cin, h, w = x.shape
    oh, pitch = 2 * h + 1, cv.tconv_pitch(w)
    t = torch.full([n, cout, oh, pitch], fill, dtype=torch.float32, device="cuda")
    os_stride = 0 if out_scale is None else out_scale.stride(0)
    rc = _lib.lib().mgf_tconv3x3s2_winograd_f32(t.data_ptr(), x.data_ptr(), u.data_ptr(), _lib.ptr(in_scale), _lib.ptr(out_scale), n, cin, h, w,
                                                cout, pitch, oh * pitch, cout * oh * pitch, os_stride, _lib.stream_ptr())
    _lib.check(rc, "tconv3x3s2_winograd")
    torch.cuda.synchronize()
    return t


def _ref(x, w, s, d):
    xs = x.double() * (s.double()[:, :, None, None] if s is not None else 1.0)
    y = torch.nn.functional.conv_transpose2d(xs, w.double().transpose(0, 1), stride=2)
    return y * (d.double()[:, :, None, None] if d is not None else 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout", [(4, 32), (12, 64), (512, 256)])
def test_weight_transform_vs_float64(cin, cout):
    from morphganformer_amd import conv as cv
    torch.manual_seed(cin + cout)
    w = torch.randn(cout, cin, 3, 3)
    gain = 1.0 / math.sqrt(cin * 9)
    u = cv.tconv_winograd_weights(w.cuda(), gain).cpu().double().numpy()
    ref = _u_ref(w.numpy(), gain)
    assert u.shape == ref.shape
    assert float(np.abs(u - ref).max() / np.abs(ref).max()) < 1e-7


# the five up-sampling layers of the 1024^2 generator (input map, cin -> cout), fewer samples for the deep ones (float64 reference on the CPU)
LAYERS = [(2, 512, 512, 32), (2, 512, 256, 64), (2, 256, 128, 128), (2, 128, 64, 256), (1, 64, 32, 512), (8, 512, 512, 32)]
RAGGED = [(1, 4, 32, 6, 6), (1, 8, 32, 20, 44), (3, 12, 64, 10, 34), (2, 36, 96, 18, 8), (1, 64, 32, 2, 2)]


def _check(n, cin, cout, h, w, styled, seed):
    from morphganformer_amd import conv as cv
    torch.manual_seed(seed)
    x = torch.randn(n, cin, h, w)
    wt = torch.randn(cout, cin, 3, 3) / math.sqrt(cin * 9)
    s = 1 + 0.2 * torch.randn(n, cin) if styled else None
    d = 1 + 0.2 * torch.randn(n, cout) if styled else None
    u = cv.tconv_winograd_weights(wt.cuda())
    t = _launch(x.cuda(), u, cout, s.cuda() if styled else None, d.cuda() if styled else None).cpu()
    ref = _ref(x, wt, s, d)
    got = t[:, :, :2 * h, :2 * w]
    assert not torch.isnan(got).any(), "an output of rows / columns 0 .. 2h-1 / 2w-1 was not written"
    assert rel_err(got, ref[:, :, :2 * h, :2 * w]) < 2e-5
    # row / column 2h / 2w and the padded pitch behind it belong to the border kernel / nobody: untouched
    assert torch.isnan(t[:, :, 2 * h, :]).all() and torch.isnan(t[:, :, :, 2 * w:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n,cin,cout,h", LAYERS)
def test_kernel_layer_shapes_vs_float64(n, cin, cout, h):
    _check(n, cin, cout, h, h, True, cin + cout + h)


@pytest.mark.gpu
@pytest.mark.parametrize("n,cin,cout,h,w", RAGGED)
@pytest.mark.parametrize("styled", [True, False])
def test_kernel_ragged_shapes_vs_float64(n, cin, cout, h, w, styled):
    """Non-square maps, maps that are not a multiple of the 32 x 4 input tile, one to three chunks of channels, one sample."""
    _check(n, cin, cout, h, w, styled, cin + cout + h + w)


@pytest.mark.gpu
@pytest.mark.parametrize("n,cin,cout,h,w", [(32, 128, 64, 32, 32), (4, 64, 32, 64, 40)])
def test_forward_with_border_vs_float64(n, cin, cout, h, w, monkeypatch):
    """conv.tconv3x3s2_forward on the Winograd path: the whole [2h+1, 2w+1] output (row / column 2h from the border kernel), nothing past
    2w in the padded pitch."""
    from morphganformer_amd import conv as cv
    monkeypatch.setattr(cv, "TCONV_WINO_MIN_WGS", 1)
    torch.manual_seed(n + cin + h + w)
    x = torch.randn(n, cin, h, w)
    wt = torch.randn(cout, cin, 3, 3) / math.sqrt(cin * 9)
    s = 1 + 0.2 * torch.randn(n, cin)
    d = 1 + 0.2 * torch.randn(n, cout)
    pc, u = cv.pack_weights(wt.cuda()), cv.tconv_winograd_weights(wt.cuda())
    buf = torch.full([n, cout, 2 * h + 1, cv.tconv_pitch(w)], float("nan"), device="cuda")
    assert cv.tconv_winograd_ok(n, cin, h, w, cout, buf)
    out = cv.tconv3x3s2_forward(x.cuda(), pc, in_scale=s.cuda(), out_scale=d.cuda(), out=buf, wt=u)
    assert rel_err(out, _ref(x, wt, s, d)) < 2e-5
    assert torch.isnan(buf[:, :, :, 2 * w + 1:]).all()


@pytest.mark.gpu
def test_hook_off_is_the_tap_list_path_bit_for_bit(monkeypatch):
    """MGF_TCONV_WINO=0 (conv.TCONV_WINO False): a call that carries Winograd weights computes exactly what the call without them does."""
    from morphganformer_amd import conv as cv
    torch.manual_seed(5)
    n, cin, cout, h = 32, 256, 128, 64
    x = torch.randn(n, cin, h, h).cuda()
    wt = torch.randn(cout, cin, 3, 3).cuda() / math.sqrt(cin * 9)
    s, d = (1 + 0.2 * torch.randn(n, cin)).cuda(), (1 + 0.2 * torch.randn(n, cout)).cuda()
    pc, u = cv.pack_weights(wt), cv.tconv_winograd_weights(wt)
    base = cv.tconv3x3s2_forward(x, pc, in_scale=s, out_scale=d).clone()
    wino = cv.tconv3x3s2_forward(x, pc, in_scale=s, out_scale=d, wt=u).clone()
    assert not torch.equal(base, wino)                      # (the Winograd launch did run: other rounding)
    assert rel_err(wino, base) < 2e-5
    monkeypatch.setattr(cv, "TCONV_WINO", False)
    off = cv.tconv3x3s2_forward(x, pc, in_scale=s, out_scale=d, wt=u)
    assert torch.equal(off, base)


def test_dispatch_predicate_keeps_unsupported_shapes_on_the_tap_list_kernel():
    from morphganformer_amd import conv as cv

    def ok(n, cin, h, w, cout, pitch_extra=0, offset=0, bf=None):
        buf = torch.empty(n * cout * (2 * h + 1) * (cv.tconv_pitch(w) + pitch_extra) + 4)
        out = buf[offset:offset + n * cout * (2 * h + 1) * (cv.tconv_pitch(w) + pitch_extra)].view(n, cout, 2 * h + 1, -1)
        return cv.tconv_winograd_ok(n, cin, h, w, cout, out, bf)

    if not cv.TCONV_WINO:
        pytest.skip("MGF_TCONV_WINO=0 in the environment")
    base_aligned = torch.empty(4).data_ptr() % 16 == 0
    assert ok(32, 512, 32, 32, 512) == base_aligned          # the generator's layers at 32 samples
    assert ok(32, 64, 512, 512, 32) == base_aligned
    assert not ok(32, 512, 33, 33, 512)                      # odd maps
    assert not ok(32, 512, 32, 31, 512)
    assert not ok(1, 512, 32, 32, 512)                       # one image (gradient mode at one target): too few workgroups
    assert not ok(32, 512, 8, 8, 512)                        # tiny maps
    assert not ok(32, 510, 32, 32, 512)                      # ragged channel chunk / tile
    assert not ok(32, 512, 32, 32, 500)
    assert not ok(32, 512, 32, 32, 512, pitch_extra=2)       # pitch not a multiple of 4
    assert not ok(32, 512, 32, 32, 512, offset=1)            # workspace not 16-byte aligned
    assert not ok(32, 512, 32, 32, 512, bf=object())         # the bf16x3 arithmetic keeps its kernel
