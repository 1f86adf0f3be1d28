"""What the three face embedders of the biometric term share: the contract `biometric.BiometricLoss` and both
projection engines rely on (`FaceEmbedder`), the 112x112 front and back of the two ArcFace networks (`ArcFaceEmbedder`: iresnet.py,
mobilefacenet.py; facenet.py scores the un-resized image), eval-mode BatchNorm as an affine map and the seeded BatchNorm of the stand-in weights."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, misc


def np64(v):
    return misc.as_numpy(v).astype(np.float64)


def bn_affine(sd, name, eps):
    """Eval-mode BatchNorm `name` of a state dict (numpy arrays or torch tensors) as float64 (scale, shift): y = x * scale + shift."""
    g = lambda k: np64(sd[f"{name}.{k}"])
    s = g("weight") / np.sqrt(g("running_var") + eps)
    return s, g("bias") - g("running_mean") * s


def seeded_bn(rng, sd, name, c):
    """The four draws of a stand-in BatchNorm, in this order (every `random_state` depends on it): non-trivial affine and running statistics."""
    sd[name + ".weight"] = rng.uniform(0.5, 1.5, c).astype(np.float32)
    sd[name + ".bias"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
    sd[name + ".running_mean"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
    sd[name + ".running_var"] = rng.uniform(0.5, 1.5, c).astype(np.float32)


class FaceEmbedder:
    """The contract of a face embedder.  BiometricLoss and the projection engines use exactly this:

        n, out             the batch size of the workspace and the float32 [n, EMB] buffer the latest embedding was written to
        embed_image(img)   img [n,3,H,W] float32 in [-1,1] -> out (or `out=`); another n re-allocates the workspace; graph-capturable after that
        backward(demb, dimg=None, accumulate=False)
                           demb [n, EMB] -> the gradient wrt the image of the latest embed_image call: returned, or written to / added to dimg
        keep_activations   gradient mode sets it True before the first forward pass (an embedder that re-uses buffers must then keep them)
        clone_for(n)       an instance sharing the weights (fc_w, fc_b, packed taps) but no mutable workspace: `_MUTABLE` names and, unless listed
                           in `_SHARED`, names starting with `_g` (the backward workspace) are left out and `_alloc(n)` rebuilds them
    """
    EMB = 512
    keep_activations = False
    _MUTABLE, _SHARED = (), ()

    def clone_for(self, n):
        other = type(self).__new__(type(self))
        other.__dict__.update({k: v for k, v in self.__dict__.items()
                               if k not in self._MUTABLE and (k in self._SHARED or not k.startswith("_g"))})
        other._alloc(n)
        return other

    def linear(self, out, x, n, k):
        """out [n, EMB] = x [n, k] fc_w^T + fc_b.  The GEMV kernel takes at most 16 rows per launch."""
        for r0 in range(0, n, 16):
            _lib.check(_lib.lib().mgf_linear_f32(out[r0:].data_ptr(), x[r0:].data_ptr(), self.fc_w.data_ptr(), self.fc_b.data_ptr(), min(16, n - r0),
                                                 k, self.EMB, _lib.stream_ptr()), "linear")
        return out

    def linear_bwd(self, dx, dout, n, k):
        for r0 in range(0, n, 16):
            _lib.check(_lib.lib().mgf_linear_bwd_f32(dx[r0:].data_ptr(), dout[r0:].data_ptr(), self.fc_w.data_ptr(), min(16, n - r0), k, self.EMB,
                                                     _lib.stream_ptr()), "linear_bwd")
        return dx

    def __call__(self, img, out=None):
        return self.embed_image(img, out)


class ArcFaceEmbedder(FaceEmbedder):
    """The ArcFace layout: embed(x112 [n,3,112,112] in [-1,1]) -> [n,512]; `embed_image` first resizes any [n,3,H,W] image bilinearly to
    112x112 (into `x112`), `backward` ends by scattering the 112x112 gradient back through that resize.  With `set_crop` the resize becomes
    the aligned, antialiased crop of mgf_face_crop_f32 and the scatter its adjoint."""
    _gp = _gn = None                 # transposed taps / batch size of the backward workspace (`_grad_ws` of the network, on first use)
    _crop = None                     # (float64 [m,2,3] device buffer, filter id) of set_crop; in `_MUTABLE`: a clone starts without one
    CROP_FILTERS = {"area": _lib.MGF_CROP_AREA, "bilinear": _lib.MGF_CROP_BILINEAR}

    def set_crop(self, matrices, filter="area"):
        """matrices [2,3], [1,2,3] (shared) or [n,2,3] (one per image): crop pixel index (u, v) -> source pixel index, (x, y) = M (u, v, 1)
        (cv2.warpAffine's WARP_INVERSE_MAP; drivers.arcface_crop makes one from landmarks); None restores the plain resize.  filter "area":
        S x S bilinear samples per crop pixel, S from the matrix; "bilinear": one.  The values are checked here, once -- the kernels cannot
        return an error -- and live in a device buffer that is rewritten IN PLACE while the shape stays (a captured hipGraph keeps reading it)."""
        if matrices is None:
            self._crop = None
            return
        m, fid = self.check_crop(matrices, filter)
        buf = self._crop[0] if self._crop is not None and self._crop[0].shape == m.shape else torch.empty(m.shape, dtype=torch.float64, device=self.device)
        buf.copy_(torch.from_numpy(m))
        self._crop = (buf, fid)

    @classmethod
    def check_crop(cls, matrices, filter="area"):
        """What set_crop refuses, without setting anything: -> (float64 numpy [m,2,3], filter id).  ValueError for a wrong shape or filter name,
        MgfError for the values mgf_face_crop_check refuses (non-finite, singular, more than 16 sub-samples per side with "area")."""
        if filter not in cls.CROP_FILTERS:
            raise ValueError(f"set_crop: filter must be 'area' or 'bilinear' (got {filter!r})")
        m = np64(matrices)
        if m.shape != (2, 3) and (m.ndim != 3 or m.shape[1:] != (2, 3) or m.shape[0] < 1):
            raise ValueError(f"set_crop: matrices must be [2,3], [1,2,3] or [n,2,3] (got {list(m.shape)})")
        m = np.ascontiguousarray(m.reshape(-1, 2, 3))
        fid = cls.CROP_FILTERS[filter]
        _lib.check(_lib.lib().mgf_face_crop_check(m.ctypes.data, m.shape[0], fid), "set_crop")
        return m, fid

    def _crop_args(self, n):
        mats, fid = self._crop
        if mats.shape[0] not in (1, n):
            raise _lib.MgfError(f"set_crop was given {mats.shape[0]} matrices, the batch has {n} images (one shared matrix, or one per image)")
        return mats.data_ptr(), int(mats.shape[0]), fid

    def embed_image(self, img, out=None):
        """img [n,3,H,W] in [-1,1] -> embedding; bilinear resize (align_corners=False) to the 112x112 ArcFace input, or the crop of set_crop."""
        _lib.require_gpu(img)
        n, c, h, w = img.shape
        if n != self.n:
            self._alloc(n)
        if self._crop is not None:
            mp, mc, fid = self._crop_args(n)
            _lib.check(_lib.lib().mgf_face_crop_f32(self.x112.data_ptr(), img.contiguous().data_ptr(), mp, n, h, w, 112, mc, fid, _lib.stream_ptr()),
                       "face_crop")
            return self.embed(self.x112, out)
        if (h, w) == (112, 112):
            return self.embed(img.contiguous(), out)
        _lib.check(_lib.lib().mgf_resize_bilinear_f32(self.x112.data_ptr(), img.contiguous().data_ptr(), n * c, h, w, 112, 112,
                                                      _lib.stream_ptr()), "resize_bilinear")
        return self.embed(self.x112, out)

    def _image_grad(self, d112, dimg, accumulate):
        """The tail of `backward`: d112 itself, or scattered through the resize into dimg [n,3,H,W] (added when `accumulate`)."""
        if dimg is None:
            return d112
        if self._crop is not None:
            h, w = dimg.shape[2:]
            mp, mc, fid = self._crop_args(self.n)
            _lib.check(_lib.lib().mgf_face_crop_bwd_f32(dimg.data_ptr(), d112.data_ptr(), mp, self.n, h, w, 112, mc, fid, int(bool(accumulate)),
                                                        _lib.stream_ptr()), "face_crop_bwd")
            return dimg
        if not accumulate:
            dimg.zero_()
        h, w = dimg.shape[2:]
        if (h, w) == (112, 112):
            dimg += d112
        else:
            _lib.check(_lib.lib().mgf_resize_bilinear_bwd_f32(dimg.data_ptr(), d112.data_ptr(), self.n * 3, h, w, 112, 112, _lib.stream_ptr()),
                       "resize_bilinear_bwd")
        return dimg

    def _affine(self, y, x, scale=None, shift=None, slope=None):
        """y = PReLU_slope(x * scale + shift) per channel, every part optional, one element-wise pass."""
        n, c = x.shape[:2]
        _lib.check(_lib.lib().mgf_channel_affine_prelu_f32(y.data_ptr(), x.data_ptr(), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(slope),
                                                           n, c, x.shape[2] * x.shape[3], _lib.stream_ptr()), "channel_affine_prelu")
        return y

    def _prelu(self, x, slope):
        return self._affine(x, x, slope=slope)

    @staticmethod
    def _positive_slopes(slopes, text):
        """`backward` reads the sign of a PReLU's input off its output: refuse slopes <= 0 before the first one."""
        if any(bool((s <= 0).any()) for s in slopes):
            raise _lib.MgfError(text)
