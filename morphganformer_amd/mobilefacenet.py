"""The MobileFaceNet embedder of the biometric term: the third face network the reference vendors,
`backbones/mobilefacenet.py` (MobileFaceNet(fp16=False, num_features=512)) -- the ArcFace contract of the IResNets (112x112 input in
[-1,1], 512-d embedding) at ~1.2 M parameters and ~0.45 GFLOP per image.  Built from its state_dict key names:

    layers.0  ConvBlock 3x3 s2 3->64 (112 -> 56)      layers.1  ConvBlock 3x3 s1 depthwise on 64
    layers.2  DepthWise(64->64, g=128, s2) (-> 28)    layers.3  4 x residual DepthWise(64, g=128)
    layers.4  DepthWise(64->128, g=256, s2) (-> 14)   layers.5  6 x residual DepthWise(128, g=256)
    layers.6  DepthWise(128->128, g=512, s2) (-> 7)   layers.7  2 x residual DepthWise(128, g=256)
    conv_sep  ConvBlock 1x1 128->512                  features  GDC: LinearBlock 7x7 depthwise on 512 (7 -> 1) -> flatten
                                                                -> Linear(512->512, no bias) -> BatchNorm1d
    ConvBlock = conv -> BN -> PReLU(c);  LinearBlock = conv -> BN;  DepthWise = ConvBlock 1x1 in->g, ConvBlock 3x3 depthwise on g at
    the stride, LinearBlock 1x1 g->out (+ the block input when residual)                                (mobilefacenet.py:16-125)

Eval-mode BatchNorm is an affine map.  Behind a 1x1 conv its scale is folded into the weights (float64, rounded once) and its shift is
the GEMM epilogue's bias, the residual its residual port (mgf_conv1x1_f32); behind a depthwise conv scale and shift ride on the
kernel's epilogue with the PReLU (mgf_dwconv_f32, csrc/depthwise.hip); the BatchNorm1d is folded into the Linear.  The PReLU behind
an expanding 1x1 is one element-wise pass (mgf_channel_affine_prelu_f32): the input-side fusion into the depthwise load is not built.
Float32 only (the module's fp16 autocast path is refused), num_features 512 only.  No checkpoint exists offline: weights are injectable
(`state`), seeded random by default (`random_state`).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from . import conv as cv
from .embedder import ArcFaceEmbedder, bn_affine, np64 as _np64, seeded_bn

EPS = 1e-5
EMB = ArcFaceEmbedder.EMB
# (layers index, in, out, groups, stride, residual blocks) of the trunk behind layers.0 / layers.1 (mobilefacenet.py:92-101)
TRUNK = [(2, 64, 64, 128, 2, 0), (3, 64, 64, 128, 1, 4), (4, 64, 128, 256, 2, 0), (5, 128, 128, 256, 1, 6), (6, 128, 128, 512, 2, 0),
         (7, 128, 128, 256, 1, 2)]


def block_table():
    """[(prefix, in, out, groups, stride, residual, stage)] of the DepthWise blocks in execution order; `stage` = the index in
    `layers` whose output the block's output is when it is the last block of that entry."""
    rows = []
    for li, cin, cout, g, stride, nres in TRUNK:
        if nres == 0:
            rows.append((f"layers.{li}", cin, cout, g, stride, False, li))
        else:
            rows += [(f"layers.{li}.layers.{j}", cin, cout, g, 1, True, li) for j in range(nres)]
    return rows


def random_state(seed=0):
    """Seeded stand-in weights under the reference's state_dict key names (numpy float32): He-scaled convs, BatchNorm with non-trivial
    affine and running statistics, PReLU slopes in (0.1, 0.4)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}

    def conv_bn(name, co, ci_per_group, k, prelu):
        sd[name + ".layers.0.weight"] = (rng.standard_normal((co, ci_per_group, k, k)) * math.sqrt(2.0 / (ci_per_group * k * k))).astype(np.float32)
        seeded_bn(rng, sd, name + ".layers.1", co)
        if prelu:
            sd[name + ".layers.2.weight"] = rng.uniform(0.1, 0.4, co).astype(np.float32)

    conv_bn("layers.0", 64, 3, 3, True)
    conv_bn("layers.1", 64, 1, 3, True)
    for p, cin, cout, g, stride, res, _ in block_table():
        conv_bn(p + ".layers.0", g, cin, 1, True)
        conv_bn(p + ".layers.1", g, 1, 3, True)
        conv_bn(p + ".layers.2", cout, g, 1, False)
    conv_bn("conv_sep", 512, 128, 1, True)
    conv_bn("features.layers.0", 512, 1, 7, False)
    sd["features.layers.2.weight"] = (rng.standard_normal((EMB, 512)) / math.sqrt(512)).astype(np.float32)
    seeded_bn(rng, sd, "features.layers.3", EMB)
    return sd


class MobileFaceNetEmbedder(ArcFaceEmbedder):
    """embed(x112 [n,3,112,112] in [-1,1]) -> [n,512]; `embed_image` first resizes any [n,3,H,W] image bilinearly to 112x112."""

    _MUTABLE = ("x112", "stem_out", "dw1_out", "bufs", "sep_out", "pool", "out", "stages", "_crop")

    def __init__(self, state=None, n=1, device="cuda", seed=0, fp16=False, num_features=EMB):
        if fp16:
            raise _lib.MgfError("MobileFaceNetEmbedder: the module's fp16 autocast path is not built (float32 only)")
        if num_features != EMB:
            raise _lib.MgfError(f"MobileFaceNetEmbedder: only num_features={EMB} is built (got {num_features})")
        _lib.lib()
        self.device = torch.device(device)
        sd = state if state is not None else random_state(seed)
        if "features.layers.2.weight" not in sd or tuple(np.shape(sd["features.layers.2.weight"])) != (EMB, 512):
            raise _lib.MgfError("MobileFaceNetEmbedder: the state dict is not a MobileFaceNet(num_features=512) one "
                                "(features.layers.2.weight [512, 512] is missing)")
        dev = self.device
        t32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)

        def folded(name):                # conv -> BN with the scale folded into the weights: (packed taps, shift)
            s, t = bn_affine(sd, name + ".layers.1", EPS)
            w = _np64(sd[name + ".layers.0.weight"]) * s[:, None, None, None]
            return cv.pack_weights(t32(w)), t32(t)

        def depthwise(name, prelu):      # (w [c, k*k], scale, shift, slope | None)
            s, t = bn_affine(sd, name + ".layers.1", EPS)
            w = _np64(sd[name + ".layers.0.weight"])
            return t32(w.reshape(w.shape[0], -1)), t32(s), t32(t), t32(_np64(sd[name + ".layers.2.weight"])) if prelu else None

        slope = lambda name: t32(_np64(sd[name + ".layers.2.weight"]))
        self.stem = (*folded("layers.0"), slope("layers.0"))
        self.dw1 = depthwise("layers.1", True)
        self.blocks = []
        for p, cin, cout, g, stride, res, stage in block_table():
            self.blocks.append(dict(expand=(*folded(p + ".layers.0"), slope(p + ".layers.0")), dw=depthwise(p + ".layers.1", True),
                                    project=folded(p + ".layers.2"), cin=cin, cout=cout, g=g, stride=stride, residual=res, stage=stage))
        self.sep = (*folded("conv_sep"), slope("conv_sep"))
        self.gdc = depthwise("features.layers.0", False)
        sf, tf = bn_affine(sd, "features.layers.3", EPS)
        self.fc_w, self.fc_b = t32(_np64(sd["features.layers.2.weight"]) * sf[:, None]), t32(tf)
        self._alloc(n)

    def _alloc(self, n):
        self.n = n
        e = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)
        self.x112 = e(n, 3, 112, 112)
        self.stem_out = e(n, 64, 56, 56)
        self.dw1_out = e(n, 64, 56, 56)
        self.bufs = []
        res = 56
        for b in self.blocks:
            ores = (res + 2 - 3) // b["stride"] + 1
            self.bufs.append(dict(h1=e(n, b["g"], res, res), h2=e(n, b["g"], ores, ores), out=e(n, b["cout"], ores, ores)))
            res = ores
        assert res == 7
        self.sep_out = e(n, 512, 7, 7)
        self.pool = e(n, 512)
        self.out = e(n, EMB)
        # the outputs of layers.0 .. layers.7 and conv_sep (tests, tools)
        last = {b["stage"]: B["out"] for b, B in zip(self.blocks, self.bufs)}
        self.stages = [self.stem_out, self.dw1_out] + [last[i] for i in range(2, 8)] + [self.sep_out]

    def _dw(self, y, x, p, k, stride, pad):
        w, s, t, slope = p
        n, c, h, wd = x.shape
        _lib.check(_lib.lib().mgf_dwconv_f32(y.data_ptr(), x.data_ptr(), w.data_ptr(), s.data_ptr(), t.data_ptr(), _lib.ptr(slope), n, c, h, wd,
                                             k, k, stride, pad, _lib.stream_ptr()), "dwconv")
        return y

    def embed(self, x112, out=None):
        _lib.require_gpu(x112, out)
        n = x112.shape[0]
        if n != self.n:
            self._alloc(n)
        assert tuple(x112.shape) == (n, 3, 112, 112) and x112.dtype == torch.float32 and x112.is_contiguous()
        pc, t, slope = self.stem
        x = self._prelu(cv.conv_forward(x112, pc, stride=2, pad=(1, 1), epilogue=_lib.make_epilogue(bias=t), out=self.stem_out), slope)
        x = self._dw(self.dw1_out, x, self.dw1, 3, 1, 1)
        for b, B in zip(self.blocks, self.bufs):
            pc, t, slope = b["expand"]
            h1 = self._prelu(cv.conv_forward(x, pc, epilogue=_lib.make_epilogue(bias=t), out=B["h1"]), slope)
            h2 = self._dw(B["h2"], h1, b["dw"], 3, b["stride"], 1)
            pc, t = b["project"]
            x = cv.conv_forward(h2, pc, epilogue=_lib.make_epilogue(bias=t, residual=x if b["residual"] else None), out=B["out"])
        pc, t, slope = self.sep
        s = self._prelu(cv.conv_forward(x, pc, epilogue=_lib.make_epilogue(bias=t), out=self.sep_out), slope)
        f = self._dw(self.pool, s, self.gdc, 7, 1, 0)
        return self.linear(self.out if out is None else out, f, n, 512)

    # ------------------------------------------------------------------ gradient mode
    def _grad_ws(self):
        """Transposed 1x1 taps + workspace of `backward` (built on first use)."""
        n = self.n
        if self._gp is None:
            self._positive_slopes([self.stem[2], self.dw1[3], self.sep[2]] + [s for b in self.blocks for s in (b["expand"][2], b["dw"][3])],
                                  "MobileFaceNet backward: PReLU slopes must be positive (the pre-activation sign is read off the output)")
            tp = lambda pc: cv.transpose_packed(pc, flip=False)
            self._gp = dict(stem=cv.transpose_packed(self.stem[0], flip=False),     # stride 2: gradient = transposed conv, same taps
                            blocks=[(tp(b["expand"][0]), tp(b["project"][0])) for b in self.blocks], sep=tp(self.sep[0]))
        if self._gn != n:
            self._gn = n
            e = lambda t: torch.empty_like(t)
            self._gb = [dict(d2=e(B["h2"]), d1=e(B["h1"]), dx=torch.empty([n, b["cin"], B["h1"].shape[2], B["h1"].shape[3]], dtype=torch.float32,
                                                                          device=self.device)) for b, B in zip(self.blocks, self.bufs)]
            self._gpool, self._gsep, self._gtop = e(self.pool), e(self.sep_out), torch.empty([n, 128, 7, 7], dtype=torch.float32, device=self.device)
            self._gdw1, self._gstem = e(self.dw1_out), e(self.stem_out)
            self._gt = torch.empty([n, 3, 113, cv.tconv_pitch(56)], dtype=torch.float32, device=self.device)
            self._gx112 = e(self.x112)

    def _dw_bwd(self, dx, dy, p, y, x_act, x_slope, k, stride, pad):
        w, s, t, slope = p
        n, c, h, wd = dx.shape
        _lib.check(_lib.lib().mgf_dwconv_bwd_data_f32(dx.data_ptr(), dy.data_ptr(), w.data_ptr(), s.data_ptr(), _lib.ptr(y if slope is not None else None),
                                                      _lib.ptr(slope), x_act.data_ptr(), x_slope.data_ptr(), n, c, h, wd, k, k, stride, pad,
                                                      _lib.stream_ptr()), "dwconv_bwd_data")
        return dx

    def backward(self, demb, dimg=None, accumulate=False):
        """demb [n,512] -> gradient wrt the image of the latest embed_image()/embed() call.  With `dimg` [n,3,H,W] the result is
        scattered through the bilinear resize into it (added when `accumulate`); otherwise the [n,3,112,112] gradient is returned."""
        _lib.require_gpu(demb, dimg)
        self._grad_ws()
        n = self.n
        self.linear_bwd(self._gpool, demb, n, 512)
        # every depthwise adjoint also applies the mask of the PReLU in front of its layer: what comes out is the gradient at the
        # preceding 1x1's (BatchNorm-folded) output, ready for that layer's transposed GEMM
        dsep = self._dw_bwd(self._gsep.view(n, 512, 7, 7), self._gpool.view(n, 512, 1, 1), self.gdc, None, self.sep_out, self.sep[2], 7, 1, 0)
        dx = cv.conv_forward(dsep, self._gp["sep"], out=self._gtop)
        for b, B, (ge, gpj), gb in reversed(list(zip(self.blocks, self.bufs, self._gp["blocks"], self._gb))):
            d2 = cv.conv_forward(dx, gpj, out=gb["d2"])
            d1 = self._dw_bwd(gb["d1"], d2, b["dw"], B["h2"], B["h1"], b["expand"][2], 3, b["stride"], 1)
            dx = cv.conv_forward(d1, ge, epilogue=_lib.make_epilogue(residual=dx) if b["residual"] else None, out=gb["dx"])
        dstem = self._dw_bwd(self._gstem, dx, self.dw1, self.dw1_out, self.stem_out, self.stem[2], 3, 1, 1)
        t = cv.tconv3x3s2_forward(dstem, self._gp["stem"], out=self._gt)                       # T[q + 1] = d x[q]: drop row/column 0
        self._gx112.copy_(t[:, :, 1:, 1:])
        return self._image_grad(self._gx112, dimg, accumulate)
