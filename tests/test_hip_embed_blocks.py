"""GPU: the IResNet and FaceNet backward passes held to float64 at every block boundary, and the backward kernels of csrc/embed.hip called
directly.

Part 1.  One HIP forward and one backward per case; then every kept gradient buffer is compared on the host with the float64 gradient of the same
tensor through the MASKED restatement (tests/embed_masked_ref.py): float64 autograd through oracle/embed_ref.py with every PReLU / ReLU / max-pool
replaced by the linear branch the HIP run itself took (read off its kept output buffers).  That removes the 1e-2 of kink noise that forced the
bulk gates of test_hip_embed.py, and what is left is gated in the max norm, per boundary b:

    max|got_b - ref64_b| / max|ref64_b|  <=  max(8 r_b, 1e-5)

r_b: the same distance for the float32 restatement on the CPU under the same masks and the same seed gradient (measured here, never taken from the
HIP result).  So that the imposed masks cannot hide a wrong forward pass, they are compared with the free float64 run's (embed_masked_ref.check_masks)
and the embedding with the free float64 embedding, to the bounds of the forward tests (2e-4 IResNet, 1e-3 FaceNet).

Part 2.  mgf_l2_normalize_bwd_f32, mgf_spatial_mean_bwd_f32, mgf_relu_bwd_slice_f32, mgf_prelu_bwd_f32, mgf_linear_bwd_f32 and
mgf_resize_bilinear_bwd_f32 through the C ABI against float64 torch, at the smallest shapes that reach every loop and branch."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import embed_masked_ref as mr
from guarded_buffers import Guarded, g_out

pytestmark = pytest.mark.gpu


def _inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 2 - 1, torch.randn(shape[0], 512, generator=g)


def _loss(scale, target_emb):
    """scale * MSE(embedding, target embedding), summed over the samples: BiometricLoss.distance_into's value, what grad_into differentiates."""
    return lambda emb: scale * ((emb - target_emb.to(emb.dtype)) ** 2).mean(dim=1).sum()


def _references(net, sd, img, seed_grad, masks, pool_idx, emb_bound, emb_hip):
    """The float64 and float32 masked gradients under the HIP run's masks, and the two conditions on those masks."""
    emb64, free64, _ = mr.free_run(net, sd, img, torch.float64)
    flips, total = mr.check_masks(masks, pool_idx, free64)
    print(f"{net} {tuple(img.shape)}: the HIP run and free float64 disagree on {flips} of {total} units ({flips / total:.2e})")
    err = float((emb_hip.cpu().double() - emb64).abs().max()) / float(emb64.abs().max())
    print(f"    embedding against free float64: {err:.3e} (bound {emb_bound:g})")
    assert err <= emb_bound
    _, ref64 = mr.masked_gradients(net, sd, img, seed_grad, masks, pool_idx, torch.float64)
    _, ref32 = mr.masked_gradients(net, sd, img, seed_grad, masks, pool_idx, torch.float32)
    return ref64, ref32


# ---------------------------------------------------------------------------------------------------------------- IResNet-18
def _iresnet_masks(e):
    from morphganformer_amd.iresnet import block_table
    masks = {"prelu": (e.stem_out > 0).cpu()}
    for row, B in zip(block_table(e.depth), e.bufs):
        masks[row[0] + ".prelu"] = (B["h"] > 0).cpu()        # PReLU outputs (slopes > 0: the output's sign is the input's); exactly 0 -> the slope
    return masks


def _iresnet_got(e, dimg):
    from morphganformer_amd.iresnet import block_table
    got = {"top": e._gtop, "x112": e._gx112, "img": dimg}
    for row, gb in zip(block_table(e.depth), e._gb):
        got["in:" + row[0]] = gb["dx"]
    return got


@pytest.mark.parametrize("size,via_loss", [((112, 112), False), ((160, 160), False), ((300, 260), False), ((64, 80), False), ((160, 160), True)],
                         ids=["112", "160", "300x260", "64x80", "160-grad_into"])
def test_iresnet18_gradient_at_every_block_boundary(size, via_loss):
    """112: no resize; 160: shrink < 2x (the atomic scatter adds at shared pixels); 300x260: shrink >= 2x, non-square; 64x80: up-sampling.
    `grad_into`: the seed gradient is mgf_mse_grad_f32's, scale 0.3 (test_biometric_gradient_matches_autograd's)."""
    from morphganformer_amd.iresnet import BiometricLoss, IResNetEmbedder, random_state
    sd = random_state(18, 3)
    img, demb = _inputs((2, 3, *size), size[0] + size[1])
    e = IResNetEmbedder(sd, depth=18, n=2)
    dimg = torch.zeros(2, 3, *size, device="cuda")
    if via_loss:
        target = torch.rand(1, 3, *size, generator=torch.Generator().manual_seed(7)) * 2 - 1
        bio = BiometricLoss(e)
        bio.set_target(target.cuda())
        bio.distance_into(torch.empty(2, device="cuda"), img.cuda())
        bio.grad_into(dimg, scale=0.3)
        seed_grad = _loss(0.3, mr.free_run("iresnet18", sd, target, torch.float64)[0])
    else:
        e.embed_image(img.cuda())
        e.backward(demb.cuda(), dimg)
        seed_grad = demb
    ref64, ref32 = _references("iresnet18", sd, img, seed_grad, _iresnet_masks(e), {}, 2e-4, e.out)
    mr.check_gate(mr.gate_rows("iresnet18", _iresnet_got(e, dimg), ref64, ref32), f"iresnet18 {size}" + (" through grad_into" if via_loss else ""))
    if size == (300, 260):
        # shrinking >= 2x: no two 112x112 pixels share a source pixel, the scatter's atomics never meet (embed.hip, resize_bilinear_bwd_kernel)
        again = torch.zeros_like(dimg)
        e.backward(demb.cuda(), again)
        assert torch.equal(again, dimg)


# ---------------------------------------------------------------------------------------------------------------- FaceNet
_FACENET_STAGES = ["repeat_1", "mixed_6a", "repeat_2", "mixed_7a", "repeat_3"]


def _facenet_block_names(net):
    """[(stage index, block index or None, state_dict prefix)] in execution order."""
    rows = []
    for si, ((kind, c, body), prefix) in enumerate(zip(net.stages, _FACENET_STAGES)):
        if kind == "res":
            rows += [(si, bi, f"{prefix}.{bi}" if bi < 5 or prefix != "repeat_3" else "block8") for bi in range(len(body))]
        else:
            rows.append((si, None, prefix))
    return rows


def _facenet_masks(net):
    """ReLU masks off the kept outputs (output > 0), pool indices off the kept pool inputs by the first-maximum rule."""
    from morphganformer_amd.facenet import _branch_key
    B = net.bufs
    masks, pools = {}, {}
    for i, (name, L) in enumerate(net.stem):
        if L is None:
            pools[name] = mr.first_max_indices(B["stem"][i - 1].cpu())
        else:
            masks[name] = (B["stem"][i] > 0).cpu()
    stage_in = [B["stem"][-1]] + [(S["blocks"][-1]["x"] if "blocks" in S else S["cat"]) for S in B["stages"][:-1]]

    def branches(prefix, brs, inter, cat):
        off = 0
        for b, br in enumerate(brs):
            for li, L in enumerate(br):
                y = inter[(b, li)] if li < len(br) - 1 else cat[:, off:off + L.cout]          # the last layer wrote its slice of the concat buffer
                masks[_branch_key(prefix, b, li, len(br))] = (y > 0).cpu()
            off += br[-1].cout
        return off

    for si, bi, prefix in _facenet_block_names(net):
        kind, c, body = net.stages[si]
        S = B["stages"][si]
        if kind == "res":
            brs, close, relu = body[bi]
            K = S["blocks"][bi]
            branches(prefix, brs, K["t"], K["cat"])
            if relu:
                masks[prefix] = (K["x"] > 0).cpu()                                             # ReLU behind the residual add: the block output
        else:
            off = branches(prefix, body, S["t"], S["cat"])
            assert S["cat"].shape[1] - off == stage_in[si].shape[1]
            pools[prefix + ".pool"] = mr.first_max_indices(stage_in[si].cpu())
    return masks, pools


def _facenet_got(net, dimg):
    g = net._g
    got = {"pre": g[("dpre",)], "mean": g[("dmean",)], "img": dimg}
    for si, bi, prefix in _facenet_block_names(net):
        if prefix != "block8":
            got["in:" + prefix] = g[("dx", si, 0 if bi is None else bi)]
    # ("dx", 5, 0) is allocated for the gradient of block8's OUTPUT (spatial_mean_bwd writes it), but block8 has no ReLU and accumulates its branches'
    # input gradients into that same buffer in place (dxin = dx): after backward() it holds the gradient of block8's INPUT and is compared as that.
    # Block8's output gradient is not read from it; it is determined by ("dmean",), which is compared, through the float64 reference.
    got["in:block8"] = g[("dx", len(net.stages), 0)]
    for i, (name, L) in enumerate(net.stem):
        if i > 0:
            got["in:" + name] = g[("stem", i)]
    assert torch.equal(g[("stem", 0)], dimg) or dimg.data_ptr() == g[("stem", 0)].data_ptr()
    return got


@pytest.mark.parametrize("n,size,via_loss", [(2, (99, 131), False), (1, (160, 160), False), (2, (99, 131), True)],
                         ids=["2x99x131", "1x160x160", "2x99x131-grad_into"])
def test_facenet_gradient_at_every_block_boundary(n, size, via_loss):
    """99x131: odd sides, the stride-2 gradients fill their inputs exactly; 160x160: even sides, the last row / column of the inputs of conv2d_1a,
    conv2d_4b, mixed_6a and mixed_7a receive nothing from the stride-2 layers.  `grad_into`: mgf_mse_grad_f32's seed gradient, scale 3e6."""
    from morphganformer_amd.facenet import InceptionResnetV1Embedder, random_state
    from morphganformer_amd.iresnet import BiometricLoss
    sd = random_state(9)
    img, demb = _inputs((n, 3, *size), size[0] * size[1] + n)
    net = InceptionResnetV1Embedder(sd, n=n)
    net.keep_activations = True
    if via_loss:
        target = torch.rand(1, 3, *size, generator=torch.Generator().manual_seed(8)) * 2 - 1
        bio = BiometricLoss(net)
        bio.set_target(target.cuda())
        bio.distance_into(torch.empty(n, device="cuda"), img.cuda())
        dimg = torch.zeros(n, 3, *size, device="cuda")
        bio.grad_into(dimg, scale=3e6)
        seed_grad = _loss(3e6, mr.free_run("facenet", sd, target, torch.float64)[0])
    else:
        net.embed_image(img.cuda())
        dimg = net.backward(demb.cuda())
        seed_grad = demb
    masks, pools = _facenet_masks(net)
    ref64, ref32 = _references("facenet", sd, img, seed_grad, masks, pools, 1e-3, net.out)
    mr.check_gate(mr.gate_rows("facenet", _facenet_got(net, dimg), ref64, ref32), f"facenet {n}x{size}" + (" through grad_into" if via_loss else ""))


# ================================================================================================================ the kernels, directly
def _lib_():
    from morphganformer_amd import _lib
    return _lib, _lib.lib(), _lib.stream_ptr()


def _gate(got, ref64, ref32, floor=1e-6):
    scale = float(ref64.abs().max())
    r = float((ref32.double() - ref64).abs().max()) / scale
    err = float((got.double().cpu() - ref64).abs().max()) / scale
    return err, max(8 * r, floor)


@pytest.mark.parametrize("d", [1, 255, 512, 700])
@pytest.mark.parametrize("n", [1, 5])
def test_l2_normalize_bwd_vs_float64(n, d):
    """d = 255: lanes with no element; 700: lanes with more than one.  With n = 5, row 1 is zero and row 3 has ||x|| < eps: both take the clamped
    branch dx = dy / eps, like autograd of x / clamp_min(||x||, eps).  Gated ROW BY ROW, max(8 r, 1e-6) of the row's max|ref| (the clamped rows'
    1 / eps would otherwise be the only thing a whole-tensor maximum sees).  At d = 1 the true gradient is zero -- dy / |x| - x <x, dy> / |x|^3
    cancels -- so the measure is the size of the cancelling terms, |dy| / |x|."""
    _lib, L, st = _lib_()
    eps = 1e-12
    g = torch.Generator().manual_seed(100 * n + d)
    x, dy = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
    if n == 5:
        x[1] = 0
        x[3] = torch.randn(d, generator=g) * 1e-14
    refs = []
    for dt in (torch.float64, torch.float32):
        xx = x.clone().to(dt).requires_grad_(True)
        y = xx / xx.norm(dim=1, keepdim=True).clamp_min(eps)
        refs.append(torch.autograd.grad(y, xx, dy.to(dt))[0])
    out = g_out(n, d)
    xd, dyd = x.cuda(), dy.cuda()
    _lib.check(L.mgf_l2_normalize_bwd_f32(out.ptr(), dyd.data_ptr(), xd.data_ptr(), n, d, eps, st))
    assert out.written() and out.guard_intact()
    got = out.t.cpu().double()
    for row in range(n):
        clamped = float(x[row].double().norm()) < eps
        scale = float(refs[0][row].abs().max()) if d > 1 or clamped else float(dy[row].abs().max() / x[row].abs().max())
        r = float((refs[1][row].double() - refs[0][row]).abs().max()) / scale
        err = float((got[row] - refs[0][row]).abs().max()) / scale
        print(f"l2_normalize_bwd n={n} d={d} row {row}{' (clamped)' if clamped else ''}: error {err:.3e}, r {r:.3e}")
        assert err <= max(8 * r, 1e-6), (row, err, r)
        if clamped:
            assert float(refs[0][row].abs().max()) > 1e11                                  # the reference did take dy / eps


@pytest.mark.parametrize("nc,hw", [(1, 1), (1, 9), (1, 870), (5376, 1), (5376, 9), (5376, 870)])
def test_spatial_mean_bwd_is_dy_times_the_float32_reciprocal(nc, hw):
    """dx[p, i] = dy[p] * (1.f / hw), to the bit.  5376 x 870 = 4.7 M elements (19 MB): mgf_stream_grid(total, 256, 4) caps the grid at
    8 * MGF_NUM_CU = 2048 workgroups, which 2.1 M elements reach, so there the stride loop runs nine times at a capped grid."""
    _lib, L, st = _lib_()
    dy = torch.randn(nc, generator=torch.Generator().manual_seed(nc + hw))
    out = g_out(nc, hw)
    dyd = dy.cuda()
    _lib.check(L.mgf_spatial_mean_bwd_f32(out.ptr(), dyd.data_ptr(), nc, hw, st))
    assert out.guard_intact()
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(hw), dtype=torch.float32)
    assert torch.equal(out.t.cpu(), (dy * inv)[:, None].expand(nc, hw))


@pytest.mark.parametrize("c", [1, 33])
@pytest.mark.parametrize("hw", [1, 42])
def test_relu_bwd_slice_bit_for_bit(c, hw):
    """dx = dy[:, dy_off : dy_off + c] where y[:, y_off : y_off + c] > 0 else 0, the two tensors of different widths and offsets; +0.0, -0.0 (both
    "not positive") and denormals of both signs in y; nothing written behind n * c * hw; slices outside their tensor refused."""
    _lib, L, st = _lib_()
    n, dyc, dyo, yc, yo = 2, c + 5, 3, c + 7, 2
    g = torch.Generator().manual_seed(c * 100 + hw)
    dy, y = torch.randn(n, dyc, hw, generator=g), torch.randn(n, yc, hw, generator=g)
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-40], dtype=torch.float32)
    sl = y[:, yo:yo + c].clone().reshape(-1)
    k = min(sl.numel(), 4)
    sl[:k] = special[:k]
    y[:, yo:yo + c] = sl.reshape(n, c, hw)
    dy[:, :dyo], dy[:, dyo + c:], y[:, :yo], y[:, yo + c:] = float("nan"), float("nan"), 1.0, 1.0      # what lies outside the slices must not be read
    out = g_out(n, c, hw)
    dyd, yd = dy.cuda(), y.cuda()
    _lib.check(L.mgf_relu_bwd_slice_f32(out.ptr(), dyd.data_ptr(), dyc, dyo, yd.data_ptr(), yc, yo, n, c, hw, st))
    assert out.written() and out.guard_intact()
    want = torch.where(y[:, yo:yo + c] > 0, dy[:, dyo:dyo + c], torch.zeros(()))
    assert torch.equal(out.t.cpu().view(torch.int32), want.view(torch.int32))
    assert L.mgf_relu_bwd_slice_f32(out.ptr(), dyd.data_ptr(), dyc, dyc - c + 1, yd.data_ptr(), yc, yo, n, c, hw, st) != 0
    assert L.mgf_relu_bwd_slice_f32(out.ptr(), dyd.data_ptr(), dyc, dyo, yd.data_ptr(), yc, yc - c + 1, n, c, hw, st) != 0
    assert L.mgf_relu_bwd_slice_f32(out.ptr(), dyd.data_ptr(), dyc, -1, yd.data_ptr(), yc, yo, n, c, hw, st) != 0
    assert out.guard_intact()


@pytest.mark.parametrize("c", [1, 7])
@pytest.mark.parametrize("hw", [1, 63])
def test_prelu_bwd_bit_for_bit(c, hw):
    """dx = dy * (y > 0 ? 1 : slope[c]) off the OUTPUT y; an output of exactly zero (either sign) takes the slope."""
    _lib, L, st = _lib_()
    n = 3
    g = torch.Generator().manual_seed(c * 100 + hw)
    dy, y, slope = torch.randn(n, c, hw, generator=g), torch.randn(n, c, hw, generator=g), torch.rand(c, generator=g) * 0.3 + 0.1
    y.reshape(-1)[0] = 0.0
    y.reshape(-1)[-1] = -0.0
    out = g_out(n, c, hw)
    dyd, yd, sd = dy.cuda(), y.cuda(), slope.cuda()
    _lib.check(L.mgf_prelu_bwd_f32(out.ptr(), dyd.data_ptr(), yd.data_ptr(), sd.data_ptr(), n, c, hw, st))
    assert out.written() and out.guard_intact()
    want = dy * torch.where(y > 0, torch.ones(()), slope.reshape(1, c, 1).expand(n, c, hw))
    assert torch.equal(out.t.cpu().view(torch.int32), want.view(torch.int32))


def test_linear_bwd_vs_float64():
    """dx = dy w at n in {1, 16}, in_features in {1, 255, 257, 1000} (one lane, a ragged last workgroup on both sides of 256, several workgroups),
    out_features in {1, 512}; n = 16 with out_features = 1024 is exactly 64 KiB of LDS and is accepted; 17 rows and 16 x 1025 are refused."""
    _lib, L, st = _lib_()
    g = torch.Generator().manual_seed(3)
    cases = [(n, i, o) for n in (1, 16) for i in (1, 255, 257, 1000) for o in (1, 512)] + [(16, 257, 1024)]
    for n, in_f, out_f in cases:
        dy, w = torch.randn(n, out_f, generator=g), torch.randn(out_f, in_f, generator=g) / math.sqrt(out_f)
        out = g_out(n, in_f)
        dyd, wd = dy.cuda(), w.cuda()
        _lib.check(L.mgf_linear_bwd_f32(out.ptr(), dyd.data_ptr(), wd.data_ptr(), n, in_f, out_f, st), f"linear_bwd {n} {in_f} {out_f}")
        assert out.written() and out.guard_intact(), (n, in_f, out_f)
        err, bound = _gate(out.t, dy.double() @ w.double(), dy @ w)
        print(f"linear_bwd n={n} in={in_f} out={out_f}: error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (n, in_f, out_f, err, bound)
    big = torch.zeros(17 * 1025, device="cuda")
    assert L.mgf_linear_bwd_f32(big.data_ptr(), big.data_ptr(), big.data_ptr(), 17, 8, 8, st) != 0
    assert L.mgf_linear_bwd_f32(big.data_ptr(), big.data_ptr(), big.data_ptr(), 16, 8, 1025, st) != 0


@pytest.mark.parametrize("n", [17, 33])
def test_the_16_row_split_of_linear_and_linear_bwd_vs_float64(n):
    """FaceEmbedder.linear / linear_bwd launch once per 16 rows with offset pointers: every row against float64, not against another launch."""
    from morphganformer_amd.embedder import FaceEmbedder
    k = 1028
    g = torch.Generator().manual_seed(n)
    x, w, b, dout = torch.randn(n, k, generator=g), torch.randn(512, k, generator=g) / math.sqrt(k), torch.randn(512, generator=g), torch.randn(n, 512, generator=g)
    e = FaceEmbedder()
    e.fc_w, e.fc_b = w.cuda(), b.cuda()
    out, dx = g_out(n, 512), g_out(n, k)
    e.linear(out.t, x.cuda(), n, k)
    e.linear_bwd(dx.t, dout.cuda(), n, k)
    assert out.written() and out.guard_intact() and dx.written() and dx.guard_intact()
    for got, ref64, ref32, what in ((out.t, F.linear(x.double(), w.double(), b.double()), F.linear(x, w, b), "linear"),
                                    (dx.t, dout.double() @ w.double(), dout @ w, "linear_bwd")):
        err, bound = _gate(got, ref64, ref32)
        rows = (got.cpu().double() - ref64).abs().amax(dim=1) / float(ref64.abs().max())
        print(f"{what} n={n}: error {err:.3e}, bound {bound:.3e}, worst row {int(rows.argmax())}")
        assert err <= bound, (what, err, bound)


def _weight_error_bound(side):
    """test_hip_mobilefacenet.py::test_backward_scatters_through_the_resize's W for source coordinates below 2^m >= side: the coordinate
    (dst + 0.5) * scale - 0.5 carries three roundings of 2^(m-25) and the scale's 2^-24 * 2^m, under 4 * 2^(m-24) in all; a weight is a product of
    two such factors: W = 2 * 4 * 2^(m-24)  (m = 6 there: 2 * 4 * 2^-18)."""
    m = max(1, math.ceil(math.log2(side)))
    return 2 * 4 * 2.0 ** (m - 24)


@pytest.mark.parametrize("ih,iw,oh,ow", [(1, 1, 4, 4), (4, 4, 1, 1), (7, 5, 112, 112), (131, 77, 50, 201), (223, 225, 112, 112), (112, 112, 112, 112)])
def test_resize_bilinear_bwd_is_the_adjoint_of_interpolate(ih, iw, oh, ow):
    """Per element |err| <= 4 * 2^-24 * A + W * S (A = sum |weight| |g|, S = sum |g| over the outputs within one pixel of the source pixel's
    support, W as derived for test_backward_scatters_through_the_resize)."""
    _lib, L, st = _lib_()
    nc = 3
    dy = torch.randn(nc, oh, ow, generator=torch.Generator().manual_seed(ih * 1000 + ow))
    out = Guarded((nc, ih, iw), torch.zeros(nc, ih, iw))
    dyd = dy.cuda()
    _lib.check(L.mgf_resize_bilinear_bwd_f32(out.ptr(), dyd.data_ptr(), nc, ih, iw, oh, ow, st))
    assert out.guard_intact()
    z = torch.zeros(1, nc, ih, iw, dtype=torch.float64, requires_grad=True)
    up = F.interpolate(z, size=(oh, ow), mode="bilinear", align_corners=False)
    (adj,) = torch.autograd.grad(up, z, dy.double()[None], retain_graph=True)
    (A,) = torch.autograd.grad(up, z, dy.double().abs()[None])
    sy = np.floor(np.clip((np.arange(oh) + 0.5) * ih / oh - 0.5, 0, None)).astype(np.int64)
    sx = np.floor(np.clip((np.arange(ow) + 0.5) * iw / ow - 0.5, 0, None)).astype(np.int64)
    S, absg = np.zeros((nc, ih, iw)), dy.double().abs().numpy()
    for ddy in (-1, 0, 1, 2):
        for ddx in (-1, 0, 1, 2):
            np.add.at(S, (slice(None), np.clip(sy + ddy, 0, ih - 1)[:, None], np.clip(sx + ddx, 0, iw - 1)[None, :]), absg)
    bound = 4 * 2.0 ** -24 * A[0] + _weight_error_bound(max(ih, iw)) * torch.from_numpy(S)
    d = (out.t.cpu().double() - adj[0]).abs()
    print(f"resize_bwd {ih}x{iw} <- {oh}x{ow}: max |err| / bound {float((d / bound.clamp_min(1e-300)).max()):.3g}, max |err| / max|adj| "
          f"{float(d.max() / adj.abs().max()):.3e}")
    assert float((d - bound).max()) <= 0


def test_resize_bilinear_bwd_is_deterministic_when_shrinking_by_two_or_more():
    """1024x1024 -> 112: no two output pixels share a source pixel, the atomics never meet on an address: two runs agree to the bit."""
    _lib, L, st = _lib_()
    dy = torch.randn(6, 112, 112, generator=torch.Generator().manual_seed(1)).cuda()
    runs = []
    for _ in range(2):
        dx = torch.zeros(6, 1024, 1024, device="cuda")
        _lib.check(L.mgf_resize_bilinear_bwd_f32(dx.data_ptr(), dy.data_ptr(), 6, 1024, 1024, 112, 112, st))
        runs.append(dx)
    assert torch.equal(*runs) and float(runs[0].abs().max()) > 0


def test_forward_edges_of_the_small_ops():
    """mgf_linear_f32 at one float4 per row and at 257 of them (one past a full sweep of the 256 lanes), 16 rows; mgf_channel_affine_prelu_f32 and
    mgf_spatial_mean_f32 at one pixel per plane, the mean also at 63 (less than a wave)."""
    _lib, L, st = _lib_()
    g = torch.Generator().manual_seed(2)
    for in_f in (4, 1028):
        x, w, b = torch.randn(16, in_f, generator=g), torch.randn(37, in_f, generator=g) / math.sqrt(in_f), torch.randn(37, generator=g)
        out = g_out(16, 37)
        xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
        _lib.check(L.mgf_linear_f32(out.ptr(), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 16, in_f, 37, st))
        assert out.written() and out.guard_intact()
        err, bound = _gate(out.t, F.linear(x.double(), w.double(), b.double()), F.linear(x, w, b))
        print(f"linear in={in_f}: error {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    x, sc, sh, sl = torch.randn(3, 5, 1, 1, generator=g), torch.rand(5, generator=g) + 0.5, torch.randn(5, generator=g), torch.rand(5, generator=g) * 0.4
    out = g_out(3, 5, 1, 1)
    xd, scd, shd, sld = x.cuda(), sc.cuda(), sh.cuda(), sl.cuda()
    _lib.check(L.mgf_channel_affine_prelu_f32(out.ptr(), xd.data_ptr(), scd.data_ptr(), shd.data_ptr(), sld.data_ptr(), 3, 5, 1, st))
    assert out.guard_intact()
    assert torch.equal(out.t.cpu(), F.prelu(x * sc.reshape(1, 5, 1, 1) + sh.reshape(1, 5, 1, 1), sl))        # as test_embed_small_ops_vs_torch at hw = 63
    for hw in (1, 63):
        x = torch.randn(21, hw, generator=g)
        out = g_out(21)
        xd = x.cuda()
        _lib.check(L.mgf_spatial_mean_f32(out.ptr(), xd.data_ptr(), 21, hw, st))
        assert out.written() and out.guard_intact()
        if hw == 1:
            assert torch.equal(out.t.cpu(), x[:, 0])
        assert float((out.t.cpu().double() - x.double().mean(1)).abs().max()) < 1e-6
