"""Gradient mode's DSSIM term, the parts that need no GPU: the torch restatement the GPU tests lean on (tests/dssim_torch_ref.py) against
oracle.loss_ref, and the C ABI of the two kernels -- exported, in the ctypes table, arguments refused before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from dssim_torch_ref import dssim_torch

SHAPES = [(2, 3, 7, 7), (1, 3, 9, 40), (2, 3, 64, 64), (1, 3, 70, 45)]


@pytest.mark.parametrize("shape", SHAPES)
def test_torch_restatement_is_ssim_ref_on_float_arrays(shape):
    """dssim_torch == (1 - ssim_ref) / 2 on the same unquantised float HWC arrays to 1e-12, and == dssim_ref to float32 rounding (1e-6) on
    images drawn on the uint8 grid (where the quantisation is the identity)."""
    from oracle.loss_ref import dssim_ref, ssim_ref
    rng = np.random.Generator(np.random.PCG64(shape[2] * 131 + shape[3]))
    img = (rng.standard_normal(shape) * 0.7).astype(np.float32)             # leaves [-1, 1] in places, like the generator's output
    tgt = rng.uniform(-1, 1, shape).astype(np.float32)
    got = dssim_torch(torch.from_numpy(img), torch.from_numpy(tgt)).numpy()
    for i in range(shape[0]):
        p, q = 127.5 * img[i].astype(np.float64) + 127.5, 127.5 * tgt[i].astype(np.float64) + 127.5
        want = (1 - ssim_ref(p.transpose(1, 2, 0), q.transpose(1, 2, 0))) / 2
        assert abs(got[i] - want) <= 1e-12, (got[i], want)
    # on the uint8 grid: x = (k - 127.5) / 127.5 is not exact in float32, but rint(127.5 x + 127.5) == k and the continuous p is within 1e-5 of k
    k_img, k_tgt = rng.integers(0, 256, shape), rng.integers(0, 256, shape)
    gi, gt = ((k_img - 127.5) / 127.5).astype(np.float32), ((k_tgt - 127.5) / 127.5).astype(np.float32)
    got = dssim_torch(torch.from_numpy(gi), torch.from_numpy(gt)).numpy()
    for i in range(shape[0]):
        want = float(dssim_ref(gi[i], gt[i]))
        assert abs(got[i] - want) <= 1e-6 * abs(want), (got[i], want)
    # a shared [c,h,w] target is the per-sample call with that target repeated
    assert torch.equal(dssim_torch(torch.from_numpy(img), torch.from_numpy(tgt[0])),
                       dssim_torch(torch.from_numpy(img), torch.from_numpy(np.broadcast_to(tgt[0], shape).copy())))
    assert float(dssim_torch(torch.from_numpy(img), torch.from_numpy(img))[0]) == 0.0


def test_dssim_entry_points_exported_and_refuse_bad_arguments_before_any_launch():
    """mgf_dssim_f32 / mgf_dssim_grad_f32: in the library and in _lib's table; h = 6, a null img and data_range = 0 return MGF_EINVAL with a
    message.  The pointers are never dereferenced (no device is touched): the checks come first."""
    from morphganformer_amd import _lib
    assert "mgf_dssim_f32" in _lib.EXPORTED_SYMBOLS and "mgf_dssim_grad_f32" in _lib.EXPORTED_SYMBOLS
    L = _lib.lib()
    EINVAL = -1
    buf = ctypes.create_string_buffer(4096)                                 # host memory standing in for every pointer: non-null, 8-byte aligned
    p = (ctypes.addressof(buf) + 7) & ~7

    def value(img=p, h=16, w=16, data_range=255.0, scratch=p, out=p):
        return L.mgf_dssim_f32(out, img, p, 1, 3, h, w, 0, data_range, 1.0, 0, scratch, None)

    def grad(img=p, h=16, w=16, data_range=255.0, scratch=p, dimg=p, out=p):
        return L.mgf_dssim_grad_f32(dimg, out, img, p, 1, 3, h, w, 0, data_range, 1.0, 0, 0, scratch, None)

    for fn in (value, grad):
        for kw in (dict(h=6), dict(w=6), dict(img=None), dict(data_range=0.0), dict(scratch=p + 4), dict(scratch=None)):
            assert fn(**kw) == EINVAL, (fn.__name__, kw)
            assert len(L.mgf_last_error()) > 0
    assert value(out=None) == EINVAL and grad(dimg=None) == EINVAL
    # one scratch buffer serves the quantised and the continuous kernels: one float64 per 16 x 16 pixel tile is the larger need
    assert L.mgf_dssim_scratch_bytes(2, 3, 33, 97) >= 2 * 3 * 3 * 7 * 8 and L.mgf_dssim_scratch_bytes(1, 3, 6, 64) == 0
