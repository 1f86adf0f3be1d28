"""LPIPS v0.1 perceptual distance on MI355X -- same call contract as the reference's lpips.PerceptualLoss
(lpips/__init__.py:13-41 -> dist_model.py:110-118 -> networks_basic.py:64-92), SqueezeNet1.1 backbone
(lpips/pretrained_networks.py:6-56; topology = torchvision squeezenet1_1.features, a third-party dependency that is not
vendored in the reference and whose ImageNet weights are a remote fetch).

  * Backbone weights are injectable (`backbone_state`: torchvision key names `features.N...`); offline they default to
    seeded He-scaled random tensors -- the same generator the oracle uses (oracle/loss_ref.py).  The learned 1x1 'lin'
    heads are the reference's own vendored data (lpips/weights/v0.1/squeeze.pth), shipped in weights/.
  * ScalingLayer (networks_basic.py:94-101) is folded into the first convolution in float64 (it has no padding, so the
    fold is exact in real arithmetic).
  * All convolutions run on the FP32-MFMA tap kernel with a fused bias+ReLU epilogue; Fire expand branches write their
    halves of the concat buffer directly.
  * The target image's 7 feature maps are computed once (`set_target`) -- the reference recomputes them every iteration.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import _lib
from . import conv as cv

FIRES = {3: (64, 16, 64), 4: (128, 16, 64), 6: (128, 32, 128), 7: (256, 32, 128),
         9: (256, 48, 192), 10: (384, 48, 192), 11: (384, 64, 256), 12: (512, 64, 256)}
TAPS_AFTER = [1, 4, 7, 9, 10, 11, 12]
POOLS = [2, 5, 8]
CHNS = [64, 128, 256, 384, 384, 512, 512]
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
WEIGHTS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "weights")
# The Fire expand3x3 convs (16..64 input channels, 255 / 127 / 63 px maps, output = a channel slice of the concat buffer) run on the form-3
# Winograd kernel: few chunks per tile is exactly where its 32x32-tile shape with four workgroups per CU pays (with form 2 they were
# slower than the tap-list kernel, 481 vs 486 iters/s).  MGF_WINOGRAD_LPIPS=0 (tuning hook) puts them back on the tap-list kernel.
USE_WINOGRAD_LPIPS = os.environ.get("MGF_WINOGRAD_LPIPS", "1") != "0"
# a tap's distance gradient and the backward of the ReLU whose output the tap is, in one pass (mgf_lpips_layer_bwd_relu_f32);
# 0: the two kernels in sequence (experiments / the equivalence test)
FUSE_TAP_RELU = os.environ.get("MGF_FUSE_TAP_RELU", "1") != "0"
# gradient mode: SqueezeNet's pools store their winning taps in the forward and the backward reads those (0: argmax recomputed from the
# input map in the backward; experiments / the equivalence test)
POOL_ARGMAX = os.environ.get("MGF_POOL_ARGMAX", "1") != "0"
# gradient mode: the tap distances also store their per-pixel sums and the tap gradients read them instead of sweeping both maps again
TAP_STATS = os.environ.get("MGF_TAP_STATS", "1") != "0"
# ONE image per forward (gradient mode with a single target): a Fire's two expand branches run as ONE 3x3 launch -- expand1x1's weights sit in
# the centre tap of 2 x ex output channels' worth of 3x3 kernels -- and their data gradients as one 3x3 launch over the concatenated gradient.
# At one image these layers sit on their launch latency (8 - 25 us each), so the extra matrix work of the 1x1 computed as a 3x3 is free and a
# launch per Fire and direction disappears; from two images on the separate launches are kept (0: always separate; the equivalence test)
MERGE_FIRE = os.environ.get("MGF_LPIPS_MERGE_FIRE", "1") != "0"


def random_squeeze_backbone(seed=0):
    """Seeded He-scaled SqueezeNet1.1 feature weights (numpy float32) under torchvision's key names."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}

    def conv(name, co, ci, k):
        sd[name + ".weight"] = (rng.standard_normal((co, ci, k, k)) * math.sqrt(2.0 / (ci * k * k))).astype(np.float32)
        sd[name + ".bias"] = (rng.standard_normal(co) * 0.05).astype(np.float32)

    conv("features.0", 64, 3, 3)
    for idx, (ci, sq, ex) in FIRES.items():
        conv(f"features.{idx}.squeeze", sq, ci, 1)
        conv(f"features.{idx}.expand1x1", ex, sq, 1)
        conv(f"features.{idx}.expand3x3", ex, sq, 3)
    return sd


# torchvision vgg16.features / alexnet.features as (kind, ...) rows; every conv is followed by ReLU; "tap" marks an LPIPS tap
# (lpips/pretrained_networks.py:58-135: alex slices [0:2|2:5|5:8|8:10|10:12], vgg16 slices [0:4|4:9|9:16|16:23|23:30])
VGG_SPEC = ([("conv", 0, 3, 64, 3, 1, 1), ("conv", 2, 64, 64, 3, 1, 1), ("tap",), ("pool", 2),
             ("conv", 5, 64, 128, 3, 1, 1), ("conv", 7, 128, 128, 3, 1, 1), ("tap",), ("pool", 2),
             ("conv", 10, 128, 256, 3, 1, 1), ("conv", 12, 256, 256, 3, 1, 1), ("conv", 14, 256, 256, 3, 1, 1), ("tap",), ("pool", 2),
             ("conv", 17, 256, 512, 3, 1, 1), ("conv", 19, 512, 512, 3, 1, 1), ("conv", 21, 512, 512, 3, 1, 1), ("tap",), ("pool", 2),
             ("conv", 24, 512, 512, 3, 1, 1), ("conv", 26, 512, 512, 3, 1, 1), ("conv", 28, 512, 512, 3, 1, 1), ("tap",)])
ALEX_SPEC = ([("conv", 0, 3, 64, 11, 4, 2), ("tap",), ("pool", 3), ("conv", 3, 64, 192, 5, 1, 2), ("tap",), ("pool", 3),
              ("conv", 6, 192, 384, 3, 1, 1), ("tap",), ("conv", 8, 384, 256, 3, 1, 1), ("tap",), ("conv", 10, 256, 256, 3, 1, 1), ("tap",)])
SPECS = {"vgg": VGG_SPEC, "alex": ALEX_SPEC}
NET_CHNS = {"squeeze": CHNS, "vgg": [64, 128, 256, 512, 512], "alex": [64, 192, 384, 256, 256]}


def random_backbone(net, seed=0):
    """Seeded He-scaled feature weights under torchvision's key names for net in {squeeze, vgg, alex}."""
    if net == "squeeze":
        return random_squeeze_backbone(seed)
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for row in SPECS[net]:
        if row[0] == "conv":
            _, idx, ci, co, k, _, _ = row
            sd[f"features.{idx}.weight"] = (rng.standard_normal((co, ci, k, k)) * math.sqrt(2.0 / (ci * k * k))).astype(np.float32)
            sd[f"features.{idx}.bias"] = (rng.standard_normal(co) * 0.05).astype(np.float32)
    return sd


def load_backbone_state(path):
    """torchvision-keyed feature weights from a state_dict file (.pth/.pt: torch.load with weights_only=True; .npz: numpy).  Accepts a
    whole-model state dict (`features.0.weight`, `classifier...`: the classifier entries are ignored) -> {key: float32 numpy}."""
    if str(path).endswith(".npz"):
        raw = dict(np.load(path))
    else:
        raw = torch.load(path, map_location="cpu", weights_only=True)
        if "state_dict" in raw and not any(k.startswith("features.") for k in raw):
            raw = raw["state_dict"]
    out = {k: np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float32)
           for k, v in raw.items() if k.startswith("features.")}
    if not out:
        raise _lib.MgfError(f"{path}: no `features.*` entries (expected a torchvision squeezenet1_1 / vgg16 / alexnet state dict)")
    return out


class SequentialFeatures:
    """LPIPS taps of a plain conv/ReLU/max-pool stack (VGG16, AlexNet) for a fixed input size, preallocated workspace.
    The ScalingLayer runs as its own element-wise step (these nets zero-pad the SCALED input, so it cannot be folded)."""

    def __init__(self, net, backbone_state, n, h, w, device, share=None):
        self.device = torch.device(device)
        dev = self.device
        self.spec = SPECS[net]
        self.n = n
        t32 = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a), dtype=np.float32), device=dev)
        if share is not None:
            self.convs, self.shift, self.scale, self.gp, self.wino = share.convs, share.shift, share.scale, share.gp, share.wino
        else:
            self.gp = {}                                   # channel-transposed packs of the backward pass, built on first use
            self.convs = {}
            # 3x3 / stride-1 / pad-1 layers with whole 32-channel tiles (every VGG16 layer but the first, AlexNet's last three): Winograd
            # F(2x2,3x3) form 3 when the launch fills the chip -- 4/9 of the matrix work of the tap-list kernel, which runs these layers at
            # 0.80 of the FP32-MFMA peak and cannot get much closer (MGF_WINOGRAD_LPIPS=0: tap-list kernel everywhere)
            self.wino = {}
            for row in self.spec:
                if row[0] == "conv":
                    _, idx, ci, co, k, st_, pd_ = row
                    wt, b = t32(backbone_state[f"features.{idx}.weight"]), t32(backbone_state[f"features.{idx}.bias"])
                    self.convs[idx] = (cv.pack_weights(wt) if k == 3 else wt, b)          # > 9 taps: packed per tap group at run time
                    if USE_WINOGRAD_LPIPS and k == 3 and st_ == 1 and pd_ == 1 and ci % 4 == 0 and co % 32 == 0:
                        self.wino[idx] = cv.winograd2_weights(wt)
                    elif USE_WINOGRAD_LPIPS and k == 3 and st_ == 1 and pd_ == 1 and ci == 3 and co % 32 == 0 and row is self.spec[0]:
                        # VGG16's first layer (3 -> 64 at the full image size: 4.3 GB of output per 16 images, 58 GFLOP): a FOURTH, all-zero
                        # input channel makes it a Winograd launch (the tap-list kernel stages 3 channels synchronously: 2.85 ms per 16 images)
                        self.wino[idx] = cv.winograd2_weights(torch.cat([wt, torch.zeros_like(wt[:, :1])], dim=1).contiguous())
            self.shift, self.scale = t32(SHIFT).reshape(1, 3, 1, 1), t32(SCALE).reshape(1, 3, 1, 1)
        e = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        self.xs = e(n, 3, h, w)
        # the scaled input with a fourth, zero channel: what the first layer's Winograd form reads (see above)
        first = self.spec[0]
        self.xs4 = (torch.zeros(n, 4, h, w, dtype=torch.float32, device=dev)
                    if first[1] in self.wino and first[2] == 3 and min(h, w) > 16 and cv.winograd_fills_chip(n, first[3], h, w) else None)
        self.bufs, self.shapes = [], {}
        c, hh, ww, tap = 3, h, w, 0
        for row in self.spec:
            if row[0] == "conv":
                _, idx, ci, co, k, s, p = row
                assert ci == c
                c, hh, ww = co, (hh + 2 * p - k) // s + 1, (ww + 2 * p - k) // s + 1
                self.bufs.append(e(n, c, hh, ww))
            elif row[0] == "pool":
                k = row[1]
                hh, ww = (hh - k) // 2 + 1, (ww - k) // 2 + 1
                self.bufs.append(e(n, c, hh, ww))
            else:
                self.bufs.append(None)
                self.shapes[tap] = (c, hh, ww)
                tap += 1

    def __call__(self, x, out=None):
        _lib.require_gpu(x)
        L, st = _lib.lib(), _lib.stream_ptr()
        torch.sub(x, self.shift, out=self.xs)
        self.xs.div_(self.scale)
        h, taps = self.xs, []
        for pos, (row, buf) in enumerate(zip(self.spec, self.bufs)):
            if row[0] == "conv":
                _, idx, ci, co, k, s, p = row
                wt, b = self.convs[idx]
                nxt = self.spec[pos + 1]
                dst = out[len(taps)] if (out is not None and nxt[0] == "tap") else buf
                if pos == 0 and self.xs4 is not None:
                    self.xs4[:, :3].copy_(h)                          # channel 3 stays zero
                    h = cv.winograd2_forward(self.xs4, self.wino[idx], epilogue=_lib.make_epilogue(bias=b, act="relu"), out=dst)
                elif idx in self.wino and ci % 4 == 0 and min(h.shape[2:]) > 16 and cv.winograd_fills_chip(h.shape[0], co, h.shape[2], h.shape[3]):
                    h = cv.winograd2_forward(h, self.wino[idx], epilogue=_lib.make_epilogue(bias=b, act="relu"), out=dst)
                elif k == 3:
                    h = cv.conv_forward(h, wt, stride=s, pad=(p, p), epilogue=_lib.make_epilogue(bias=b, act="relu"), out=dst)
                else:
                    h = cv.conv_large_forward(h, wt, b, s, p, act="relu", out=dst)
            elif row[0] == "pool":
                nn, c, ih, iw = h.shape
                _lib.check(L.mgf_maxpool_s2_floor_f32(buf.data_ptr(), h.data_ptr(), nn * c, ih, iw, row[1], st), "maxpool")
                h = buf
            else:
                taps.append(h)
        return taps


    def backward(self, target_taps, lins, scale, per_sample=False, region=None):
        """Gradient of  scale * sum_taps lpips_layer(tap, target_tap)  with respect to the input image of the latest __call__
        (taps in the internal workspace); per_sample: target_taps hold one target per sample instead of one shared target.
        3x3 / stride-1 layers take the tap-list kernel on transposed, flipped taps; AlexNet's 5x5 runs as chained <= 9-tap launches
        (conv.conv_large_dgrad) and its 11x11 / stride-4 stem as 16 phase launches (conv.conv_strided_dgrad).
        region: (per-tap normalised weights [nw, h_l * w_l], nw) -- the gradient of the region-weighted distance (the weighted tap kernels)."""
        L, st = _lib.lib(), _lib.stream_ptr()
        rows = [(row, buf) for row, buf in zip(self.spec, self.bufs)]
        if not self.gp:
            for row in self.spec:
                if row[0] == "conv" and row[4] == 3:
                    self.gp[row[1]] = cv.transpose_packed(self.convs[row[1]][0], flip=True)
        if getattr(self, "gbufs", None) is None:
            self.gbufs = [None if b is None else torch.empty_like(b) for b in self.bufs]
            self.gxs = torch.empty_like(self.xs)
        n = self.n
        nodes = [i for i, (row, _) in enumerate(rows) if row[0] != "tap"]
        tap_of, k = {}, 0
        for i, (row, _) in enumerate(rows):
            if row[0] == "tap":
                tap_of[[j for j in nodes if j < i][-1]] = k          # a tap reads the output of the row in front of it
                k += 1
        for pos in range(len(nodes) - 1, -1, -1):
            i = nodes[pos]
            row, h = rows[i]
            gh = self.gbufs[i]
            c, hh, ww = h.shape[1:]
            behind = pos != len(nodes) - 1                     # a gradient from the rows behind this one is already in gh
            fused = FUSE_TAP_RELU and i in tap_of and row[0] == "conv"
            if i in tap_of and region is not None:
                kk = tap_of[i]
                _tap_bwd_weighted(L, st, fused, gh, None, gh if behind else None, h, target_taps[kk], lins[kk],
                                  getattr(self, "tap_stats", {}).get(kk), region, kk, n, c, c, hh * ww, per_sample, scale, behind)
            elif fused:
                kk = tap_of[i]
                _lib.check(L.mgf_lpips_layer_bwd_relu_stats_f32(gh.data_ptr(), None, gh.data_ptr() if behind else None, h.data_ptr(),
                                                                target_taps[kk].data_ptr(), lins[kk].data_ptr(),
                                                                _lib.ptr(getattr(self, "tap_stats", {}).get(kk)), n, c, c, hh * ww,
                                                                c * hh * ww if per_sample else 0, float(scale), st), "lpips_layer_bwd_relu")
            elif i in tap_of:
                kk = tap_of[i]
                _lib.check(L.mgf_lpips_layer_bwd_f32(gh.data_ptr(), h.data_ptr(), target_taps[kk].data_ptr(), lins[kk].data_ptr(), n, c,
                                                     hh * ww, c * hh * ww if per_sample else 0, float(scale), int(behind), st),
                           "lpips_layer_bwd")
            prev = self.bufs[nodes[pos - 1]] if pos > 0 else self.xs
            gprev = self.gbufs[nodes[pos - 1]] if pos > 0 else self.gxs
            if row[0] == "conv":
                if not fused:
                    _lib.check(L.mgf_relu_bwd_split_f32(gh.data_ptr(), None, gh.data_ptr(), h.data_ptr(), n, c, c, hh * ww, st), "relu_bwd")
                _, idx, _ci, _co, k, stride, pad = row
                if k == 3 and stride == 1:
                    cv.conv_forward(gh, self.gp[idx], pad=(1, 1), out=gprev)
                elif stride == 1:
                    cv.conv_large_dgrad(gh, self.convs[idx][0], pad, out=gprev)
                else:
                    cv.conv_strided_dgrad(gh, self.convs[idx][0], stride, pad, tuple(prev.shape[2:]), out=gprev)
            else:
                _lib.check(L.mgf_maxpool_s2_floor_bwd_f32(gprev.data_ptr(), gh.data_ptr(), prev.data_ptr(), n * c, prev.shape[2],
                                                          prev.shape[3], row[1], st), "maxpool_bwd")
        return self.gxs.div_(self.scale)                   # through the ScalingLayer (x - shift) / scale


def _tap_bwd_weighted(L, st, fused, da, db, din, h, target, lin, stats, region, k, n, c, c_split, hw, per_sample, scale, accumulate):
    """One tap's region-weighted distance gradient: the weighted form of the launch `backward` would issue without a weight (fused with
    the ReLU behind the tap, or the plain form that adds to the gradient already in da)."""
    omegas, nw = region
    wm, ws = omegas[k], (hw if nw > 1 else 0)
    if fused:
        _lib.check(L.mgf_lpips_layer_bwd_relu_stats_weighted_f32(da.data_ptr(), _lib.ptr(db), _lib.ptr(din), h.data_ptr(), target.data_ptr(),
                                                                 lin.data_ptr(), _lib.ptr(stats), wm.data_ptr(), n, c, c_split, hw,
                                                                 c * hw if per_sample else 0, ws, float(scale), st), "lpips_layer_bwd_relu_weighted")
    else:
        _lib.check(L.mgf_lpips_layer_bwd_weighted_f32(da.data_ptr(), h.data_ptr(), target.data_ptr(), lin.data_ptr(), wm.data_ptr(), n, c, hw,
                                                      c * hw if per_sample else 0, ws, float(scale), int(accumulate), st), "lpips_layer_bwd_weighted")


def region_tap_weights(weight, sides):
    """Normalised per-tap region weights.  weight: [..., H, W] >= 0 (any float dtype, CPU or device); sides: the taps' (h_l, w_l).  For every
    tap W_l = adaptive_avg_pool2d(W, (h_l, w_l)) and omega_l = W_l / sum(W_l), both in float64, cast to float32 once -> list of [..., h_l, w_l].
    (Every tap's grid is taken to span the image uniformly: the geometric assumption of the reference's spatial=True up-sampling,
    networks_basic.py:20-24.)  A constant W gives omega_l = 1 / (h_l w_l): the un-weighted spatial mean."""
    w = torch.as_tensor(weight).to(torch.float64)
    lead = w.shape[:-2]
    w4 = w.reshape(-1, 1, *w.shape[-2:])
    out = []
    for hh, ww in sides:
        wl = torch.nn.functional.adaptive_avg_pool2d(w4, (int(hh), int(ww)))
        wl = wl / wl.sum(dim=(2, 3), keepdim=True)
        out.append(wl.to(torch.float32).reshape(*lead, int(hh), int(ww)))
    return out


def check_region_weight(weight, what="region weight"):
    """A region weight as float64 [n, H, W] on the CPU from [H,W], [1,1,H,W] or [n,1,H,W]; ValueError for a negative or non-finite value, an
    all-zero map or another shape."""
    w = torch.as_tensor(weight).detach().to("cpu", torch.float64)
    if w.dim() == 2:
        w = w[None]
    elif w.dim() == 4 and w.shape[1] == 1:
        w = w[:, 0]
    else:
        raise ValueError(f"{what}: expected [H,W], [1,1,H,W] or [n,1,H,W] (got {tuple(w.shape)})")
    if w.numel() == 0 or not bool(torch.isfinite(w).all()):
        raise ValueError(f"{what}: values must be finite")
    if bool((w < 0).any()):
        raise ValueError(f"{what}: values must be >= 0")
    if not bool((w.sum(dim=(1, 2)) > 0).all()):
        raise ValueError(f"{what}: every map needs a positive sum (got an all-zero map)")
    return w.contiguous()


def _pool_out(n):
    o = (n - 3 + 1) // 2 + 1
    if (o - 1) * 2 >= n:
        o -= 1
    return o


class SqueezeFeatures:
    """The 7 LPIPS taps of SqueezeNet1.1 for a fixed input size, with a preallocated workspace."""

    def __init__(self, backbone_state, n, h, w, device, share=None):
        self.device = torch.device(device)
        dev = self.device
        if share is not None:
            self.c0, self.fires, self.wino3 = share.c0, share.fires, share.wino3          # packed weights are size independent
            self.merged, self.wino3m = share.merged, share.wino3m
            self.stem_w, self.stem_b = share.stem_w, share.stem_b
            self.gp, self.gpw, self.gpm, self.gpwm = share.gp, share.gpw, share.gpm, share.gpwm
        else:
            self.gp, self.gpw = {}, {}                            # channel-transposed packs of the backward pass (+ Winograd images), built on first use
            self.gpm, self.gpwm = {}, {}                          # ... of the merged expand launch (one image per forward)
            g = lambda k: np.asarray(backbone_state[k], dtype=np.float64)
            t32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)
            w0, b0 = g("features.0.weight"), g("features.0.bias")
            sc, sh = np.asarray(SCALE), np.asarray(SHIFT)
            w0f = w0 / sc[None, :, None, None]
            b0f = b0 - (w0 * (sh / sc)[None, :, None, None]).sum(axis=(1, 2, 3))
            self.c0 = (cv.pack_weights(t32(w0f)), t32(b0f))
            self.stem_w, self.stem_b = t32(w0f.reshape(64, 27)), t32(b0f)       # operands of the fused stem kernel
            self.fires = {}
            self.wino3 = {}                                       # expand3x3 in Winograd form (csrc/wino.hip form 2: odd maps, concat slice)
            for idx in FIRES:
                p = f"features.{idx}"
                self.fires[idx] = tuple((cv.pack_weights(t32(g(f"{p}.{nm}.weight"))), t32(g(f"{p}.{nm}.bias")))
                                        for nm in ("squeeze", "expand1x1", "expand3x3"))
                if USE_WINOGRAD_LPIPS:
                    self.wino3[idx] = cv.winograd2_weights(t32(g(f"{p}.expand3x3.weight")))
            # the merged expand launch of the one-image path (MERGE_FIRE): [2 ex, sq, 3, 3], expand1x1 in the centre tap of the first ex kernels
            self.merged, self.wino3m = {}, {}
            for idx in FIRES:
                p = f"features.{idx}"
                w1, w3 = g(f"{p}.expand1x1.weight"), g(f"{p}.expand3x3.weight")
                wm = np.zeros((2 * w1.shape[0], w1.shape[1], 3, 3))
                wm[:w1.shape[0], :, 1, 1] = w1[:, :, 0, 0]
                wm[w1.shape[0]:] = w3
                bm = np.concatenate([g(f"{p}.expand1x1.bias"), g(f"{p}.expand3x3.bias")])
                self.merged[idx] = (cv.pack_weights(t32(wm)), t32(bm))
                if USE_WINOGRAD_LPIPS:
                    self.wino3m[idx] = cv.winograd2_weights(t32(wm))
        self.n = n
        self.merge = set()           # Fire modules whose expand branches run merged (filled below: one image, maps the Winograd launch fills the chip with)
        e = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        hh, ww = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        self.shapes = {1: (64, hh, ww)}
        self.buf = {1: e(n, 64, hh, ww)}
        self.sq = {}
        self.pidx, self.have_argmax = {}, False          # winning taps of the pools (uint8), kept by forwards run with argmax=True
        c = 64
        for idx in range(2, 13):
            if idx in POOLS:
                hh, ww = _pool_out(hh), _pool_out(ww)
                self.buf[idx] = e(n, c, hh, ww)
            else:
                ci, sq, ex = FIRES[idx]
                assert ci == c
                self.sq[idx] = e(n, sq, hh, ww)
                # merged only where the merged launch is a Winograd launch (255^2 / 127^2 maps of a 1024^2 image): there both branches sit on
                # their launch latency; on the 63^2 maps the tap-list kernel does real work and twice of it costs more than a launch saves
                if MERGE_FIRE and n == 1 and idx in self.wino3m and min(hh, ww) > 16 and cv.winograd_fills_chip(n, 2 * ex, hh, ww):
                    self.merge.add(idx)
                c = 2 * ex
                self.buf[idx] = e(n, c, hh, ww)
            self.shapes[idx] = (c, hh, ww)

    def _grad_ws(self):
        """Workspace + transposed taps of `backward` (gradient mode only, allocated on first use)."""
        if not self.gp:
            self.gp["c0"] = cv.transpose_packed(self.c0[0], flip=False)       # stride-2 conv -> stride-2 transposed conv, same taps
            for idx, ((ps, _), (p1, _), (p3, _)) in self.fires.items():
                self.gp[idx] = (cv.transpose_packed(ps, False), cv.transpose_packed(p1, False), cv.transpose_packed(p3, True))
                if USE_WINOGRAD_LPIPS and p3.cin % 32 == 0:
                    # the expand-3x3 data gradient (E -> S channels) on the Winograd kernel where S is a multiple of its 32-channel tile
                    w = p3.wp[:, :, :p3.cout].reshape(3, 3, p3.cin, p3.cout).permute(3, 2, 0, 1)        # [E, S, kh, kw]
                    # (the form-3 image whatever this instance's map size: the packs are shared between sizes)
                    self.gpw[idx] = cv.winograd2_weights(w.permute(1, 0, 2, 3).flip(2, 3).contiguous(), 1.0)
            for idx, (pm, _) in self.merged.items():
                # the merged data gradient: one true convolution over the concatenated gradient [d expand1x1 | d expand3x3] (2 ex -> sq channels)
                self.gpm[idx] = cv.transpose_packed(pm, True)
                if USE_WINOGRAD_LPIPS and pm.cin % 32 == 0:
                    w = pm.wp[:, :, :pm.cout].reshape(3, 3, pm.cin, pm.cout).permute(3, 2, 0, 1)        # [2 ex, sq, kh, kw]
                    self.gpwm[idx] = cv.winograd2_weights(w.permute(1, 0, 2, 3).flip(2, 3).contiguous(), 1.0)
        if getattr(self, "gbuf", None) is None:
            e = lambda t: torch.empty_like(t)
            self.gbuf = {idx: e(t) for idx, t in self.buf.items()}
            self.gsq = {idx: e(t) for idx, t in self.sq.items()}
            # merged Fires (one image): the two halves of ONE [1, 2 ex, h, w] tensor are dense blocks, so the kernels that write the split
            # gradient fill the merged launch's input in place
            self.gcat = {idx: e(self.buf[idx]) for idx in self.merge}
            self.gex = {idx: ((self.gcat[idx][:, :FIRES[idx][2]], self.gcat[idx][:, FIRES[idx][2]:]) if idx in self.merge else
                              (e(self.buf[idx][:, :FIRES[idx][2]].contiguous()), e(self.buf[idx][:, FIRES[idx][2]:].contiguous())))
                        for idx in FIRES}
            n, _, h1, w1 = self.buf[1].shape
            self.gimg = torch.empty([n, 3, 2 * h1 + 1, cv.tconv_pitch(w1)], dtype=torch.float32, device=self.device)

    def backward(self, target_taps, lins, scale, per_sample=False, region=None):
        """Gradient of  scale * sum_taps lpips_layer(tap, target_tap)  with respect to the input image of the latest __call__
        (un-fused path: all 7 taps are in the workspace; per_sample: one target per sample instead of one shared target).  Returns a [n,3,2*h1+1,2*w1+1] view (rows/columns beyond it get no
        gradient: the stride-2 stem never reads them).  region: as SequentialFeatures.backward."""
        self._grad_ws()
        L, st = _lib.lib(), _lib.stream_ptr()
        n = self.n
        for idx in range(12, 0, -1):
            h, gh = self.buf[idx], self.gbuf[idx]
            c, hh, ww = h.shape[1:]
            # every tap is a ReLU output (the stem's, or a Fire's concat): its distance gradient and that ReLU's backward (with the
            # Fire's split into the two expand branches) are one pass
            fused = FUSE_TAP_RELU and idx in TAPS_AFTER and idx not in POOLS
            if idx in TAPS_AFTER and region is not None:
                k = TAPS_AFTER.index(idx)
                da, db, ex = (gh, None, c) if (idx == 1 or not fused) else (*self.gex[idx], FIRES[idx][2])
                _tap_bwd_weighted(L, st, fused, da, db, gh if idx != 12 else None, h, target_taps[k], lins[k],
                                  getattr(self, "tap_stats", {}).get(k), region, k, n, c, ex, hh * ww, per_sample, scale, idx != 12)
            elif fused:
                k = TAPS_AFTER.index(idx)
                da, db, ex = (gh, None, c) if idx == 1 else (*self.gex[idx], FIRES[idx][2])
                _lib.check(L.mgf_lpips_layer_bwd_relu_stats_f32(da.data_ptr(), _lib.ptr(db), gh.data_ptr() if idx != 12 else None, h.data_ptr(),
                                                                target_taps[k].data_ptr(), lins[k].data_ptr(),
                                                                _lib.ptr(getattr(self, "tap_stats", {}).get(k)), n, c, ex, hh * ww,
                                                                c * hh * ww if per_sample else 0, float(scale), st), "lpips_layer_bwd_relu")
            elif idx in TAPS_AFTER:
                k = TAPS_AFTER.index(idx)
                _lib.check(L.mgf_lpips_layer_bwd_f32(gh.data_ptr(), h.data_ptr(), target_taps[k].data_ptr(), lins[k].data_ptr(), n, c,
                                                     hh * ww, c * hh * ww if per_sample else 0, float(scale), int(idx != 12), st),
                           "lpips_layer_bwd")
            if idx == 1:
                if not fused:
                    _lib.check(L.mgf_relu_bwd_split_f32(gh.data_ptr(), None, gh.data_ptr(), h.data_ptr(), n, c, c, hh * ww, st), "relu_bwd")
                return cv.tconv3x3s2_forward(gh, self.gp["c0"], out=self.gimg)
            if idx in POOLS:
                x = self.buf[idx - 1]
                if self.have_argmax:
                    _lib.check(L.mgf_maxpool3x3s2_ceil_bwd_idx_f32(self.gbuf[idx - 1].data_ptr(), gh.data_ptr(), self.pidx[idx].data_ptr(), n * c,
                                                                   x.shape[2], x.shape[3], hh, ww, st), "maxpool_bwd_idx")
                else:
                    _lib.check(L.mgf_maxpool3x3s2_ceil_bwd_f32(self.gbuf[idx - 1].data_ptr(), gh.data_ptr(), x.data_ptr(), n * c, x.shape[2],
                                                               x.shape[3], hh, ww, st), "maxpool_bwd")
                continue
            sqT, e1T, e3T = self.gp[idx]
            ex = FIRES[idx][2]
            da, db = self.gex[idx]
            if not fused:
                _lib.check(L.mgf_relu_bwd_split_f32(da.data_ptr(), db.data_ptr(), gh.data_ptr(), h.data_ptr(), n, c, ex, hh * ww, st),
                           "relu_bwd_split")
            s, gs = self.sq[idx], self.gsq[idx]
            merged = idx in self.merge
            if merged:
                gc = self.gcat[idx]
                if idx in self.gpwm and min(hh, ww) > 16 and cv.winograd_fills_chip(n, gs.shape[1], hh, ww):
                    cv.winograd_forward(gc, self.gpwm[idx], out=gs)
                else:
                    cv.conv_forward(gc, self.gpm[idx], pad=(1, 1), out=gs)
            else:
                cv.conv_forward(da, e1T, out=gs)
            if merged:
                pass
            elif idx in self.gpw and cv.winograd_fills_chip(n, gs.shape[1], hh, ww):
                cv.winograd_forward(db, self.gpw[idx], epilogue=_lib.make_epilogue(residual=gs), out=gs)
            else:
                cv.conv_forward(db, e3T, pad=(1, 1), epilogue=_lib.make_epilogue(residual=gs), out=gs)
            _lib.check(L.mgf_relu_bwd_split_f32(gs.data_ptr(), None, gs.data_ptr(), s.data_ptr(), n, s.shape[1], s.shape[1], hh * ww, st),
                       "relu_bwd")
            cv.conv_forward(gs, sqT, out=self.gbuf[idx - 1])
        raise AssertionError("unreachable")

    def stem(self, x, feat_out=None, feat_ref=None, lin=None, dist_out=None, scratch=None):
        """features.0-2 in one kernel (csrc/lpips_stem.hip): writes the pooled map (self.buf[2]) and either the normalised
        tap-0 map (`feat_out`, reference image) or the tap-0 LPIPS distance against `feat_ref` into `dist_out` [n]."""
        _lib.require_gpu(x, feat_out, feat_ref, dist_out)
        n, _, h, w = x.shape
        assert n == self.n and x.is_contiguous() and x.dtype == torch.float32
        _lib.check(_lib.lib().mgf_lpips_stem_f32(self.buf[2].data_ptr(), x.data_ptr(), self.stem_w.data_ptr(), self.stem_b.data_ptr(),
                                                 _lib.ptr(feat_out), _lib.ptr(feat_ref), _lib.ptr(lin), _lib.ptr(dist_out), n, h, w, 0,
                                                 _lib.ptr(scratch), _lib.stream_ptr()), "lpips_stem")
        return self.buf[2]

    def __call__(self, x, out=None, from_pooled=False, argmax=False):
        """x: [n,3,h,w] in [-1,1] (un-scaled; ScalingLayer is folded).  Returns the list of 7 tap tensors
        (views of the internal workspace unless `out` -- a list of 7 preallocated tensors -- is given).
        from_pooled=True: `stem()` already produced the first pooled map; tap 0 is not materialised (entry 0 is None)."""
        _lib.require_gpu(x)
        L = _lib.lib()
        st = _lib.stream_ptr()
        taps = []
        k = 0
        self.have_argmax = bool(argmax) and not from_pooled and POOL_ARGMAX

        def dest(idx):
            nonlocal k
            if idx in TAPS_AFTER and out is not None:
                return out[TAPS_AFTER.index(idx)]
            return self.buf[idx]

        if from_pooled:
            h = self.buf[2]
            taps.append(None)
        else:
            pc, b = self.c0
            if cv.NARROW_CONV:
                h = cv.conv3x3s2_few_inputs(x.contiguous(), self.stem_w.view(64, 3, 3, 3), bias=b, relu=True, out=dest(1))
            else:
                h = cv.conv_forward(x.contiguous(), pc, stride=2, pad=(0, 0), epilogue=_lib.make_epilogue(bias=b, act="relu"), out=dest(1))
            taps.append(h)
        for idx in range(3 if from_pooled else 2, 13):
            if idx in POOLS:
                y = self.buf[idx]
                n, c, ih, iw = h.shape
                if self.have_argmax:
                    # gradient mode: the pool also stores each window's winning tap (one byte per output), so that its backward reads
                    # neither the input map nor scans the windows again
                    if idx not in self.pidx:
                        self.pidx[idx] = torch.empty(y.shape, dtype=torch.uint8, device=y.device)
                    _lib.check(L.mgf_maxpool3x3s2_ceil_idx_f32(y.data_ptr(), self.pidx[idx].data_ptr(), h.data_ptr(), n * c, ih, iw, y.shape[2],
                                                               y.shape[3], st), "maxpool_idx")
                else:
                    _lib.check(L.mgf_maxpool3x3s2_ceil_f32(y.data_ptr(), h.data_ptr(), n * c, ih, iw, y.shape[2], y.shape[3], st), "maxpool")
                h = y
            else:
                (ps, bs), (p1, b1), (p3, b3) = self.fires[idx]
                s = cv.conv_forward(h, ps, epilogue=_lib.make_epilogue(bias=bs, act="relu"), out=self.sq[idx])
                y = dest(idx)
                ex = p1.cout
                if idx in self.merge:
                    cv.winograd2_forward(s, self.wino3m[idx], epilogue=_lib.make_epilogue(bias=self.merged[idx][1], act="relu"), out=y)
                    h = y
                    if idx in TAPS_AFTER:
                        taps.append(h)
                    continue
                cv.conv_forward(s, p1, epilogue=_lib.make_epilogue(bias=b1, act="relu"), out=y, out_choff=0)
                # Winograd when its grid (no split-K) fills the chip: the 25-candidate literal iteration, not a single small image
                if idx in self.wino3 and min(s.shape[2:]) > 16 and cv.winograd_fills_chip(s.shape[0], ex, s.shape[2], s.shape[3]):
                    cv.winograd2_forward(s, self.wino3[idx], epilogue=_lib.make_epilogue(bias=b3, act="relu"), out=y, out_choff=ex)
                else:
                    cv.conv_forward(s, p3, pad=(1, 1), epilogue=_lib.make_epilogue(bias=b3, act="relu"), out=y, out_choff=ex)
                h = y
            if idx in TAPS_AFTER:
                taps.append(h)
        return taps


def spatial_tap_output_side(h, H):
    """Side of a tap map of side h after the reference's `upsample(..., out_H=H)` (networks_basic.py:20-24): it hands torch the scale factor
    1. * H / h, and torch sizes the output floor(h * scale) in double -- which is not always H (47 * (96 / 47) floors to 95)."""
    return int(math.floor(float(h) * (1.0 * H / h)))


class PerceptualLoss(torch.nn.Module):
    """lpips.PerceptualLoss(model='net-lin', net='squeeze', use_gpu=True)(pred, target, normalize=False) -> [N,1,1,1];
    with spatial=True -> the [N,1,H,W] map of PNetLin(spatial=True) (networks_basic.py:75-76,85-92; `distance_map_into`)."""

    def __init__(self, model="net-lin", net="squeeze", colorspace="rgb", spatial=False, use_gpu=True, gpu_ids=(0,),
                 backbone_state=None, backbone_seed=None, allow_random_backbone=False, device="cuda"):
        """backbone_state: the torchvision feature weights (`features.N...` keys, tensors or arrays; `load_backbone_state` reads a
        .pth / .npz) -- what the reference obtains with tv.<net>(pretrained=True) (pretrained_networks.py:9,60,100).  Without it
        the distance would be computed on meaningless features, so that is an ERROR unless the caller opts in to the seeded random
        backbone (allow_random_backbone=True or an explicit backbone_seed: benchmarks and parity tests, where only the arithmetic
        matters)."""
        super().__init__()
        if model != "net-lin" or colorspace != "rgb":
            raise NotImplementedError("the MI355X path implements model='net-lin', colorspace='rgb'")
        self.spatial = bool(spatial)
        if net not in NET_CHNS:
            raise NotImplementedError(f"unknown LPIPS backbone {net!r} (squeeze, vgg, alex)")
        if not use_gpu:
            raise _lib.MgfError("PerceptualLoss(use_gpu=False): the MI355X package has no CPU path")
        if backbone_state is None:
            if not allow_random_backbone and backbone_seed is None:
                raise _lib.MgfError(
                    f"PerceptualLoss(net={net!r}): no backbone weights.  Pass backbone_state= (torchvision `{net}` feature weights, see "
                    "lpips.load_backbone_state) or opt in to seeded random features with allow_random_backbone=True / backbone_seed=")
            backbone_state = random_backbone(net, 0 if backbone_seed is None else backbone_seed)
            self.random_backbone = True
        else:
            self.random_backbone = False
        self.backbone_state = backbone_state
        _lib.lib()
        self.device_ = torch.device(device)
        self.net = net
        self.chns = NET_CHNS[net]
        lin = np.load(os.path.join(WEIGHTS_DIR, f"lpips_lin_{net}.npz"))
        self.lins = [torch.as_tensor(lin[f"lin{i}"], dtype=torch.float32, device=self.device_) for i in range(len(self.chns))]
        self._feats = {}
        self._stats = {}
        self._map_ws = {}                 # (n, H) -> per-tap maps of distance_map_into (spatial=True)
        self._map_taps = None             # spatial=True beside the fused stem: the target's unit taps through the un-fused path
        self._target_taps = None
        self._target_n = 1
        self.pair_offset = None           # [B] float32 = alpha (1 - alpha) LPIPS(Ta, Tb) while a target pair is set (set_target_pair)
        self._last, self._last_hw = None, None
        self._region = None               # float64 [nw, H, W] on the CPU while a region weight is set (set_region_weight)
        self._region_taps = {}            # (nw, H, W) -> per-tap normalised weights [nw, h_l * w_l], rewritten in place per weight
        # the one-pass stem exists for SqueezeNet's first three layers; MGF_LPIPS_STEM=0 (tuning hook) keeps them separate
        self.fused_stem = net == "squeeze" and os.environ.get("MGF_LPIPS_STEM", "1") != "0"
        self._scratch = torch.empty(int(_lib.lib().mgf_reduce_scratch_floats()), dtype=torch.float32, device=self.device_)
        self._val = torch.zeros(1, dtype=torch.float32, device=self.device_)

    def _features(self, n, h, w):
        """Feature extractor (workspace) for a batch/input size; packed weights are shared between instances."""
        key = (n, h, w)
        f = self._feats.get(key)
        if f is None:
            share = next(iter(self._feats.values()), None)
            if self.net == "squeeze":
                f = SqueezeFeatures(self.backbone_state, n, h, w, self.device_, share=share)
            else:
                f = SequentialFeatures(self.net, self.backbone_state, n, h, w, self.device_, share=share)
            self._feats[key] = f
        return f

    def set_region_weight(self, weight):
        """Weight the distance by region: weight [H,W], [1,1,H,W] (one map for every candidate) or [n,1,H,W] (one per candidate) >= 0 at the
        image size; None: the uniform spatial mean again, with today's dispatch (fused stem included).  Per tap the weight is pooled to the
        tap's grid and normalised (`region_tap_weights`), and `distance_into`, `grad_into`, `distance_per_tap` and the scalar module call
        compute sum_l sum_p omega_l[p] m_l[p] on the un-fused path (the fused stem consumes tap 0 with a uniform mean).  `distance_map_into`
        is unaffected.  The per-tap weights live in buffers that are rewritten in place while the geometry stays (captured graphs read
        them).  With a target pair set, call `set_target_pair` again afterwards: its constant depends on the weight."""
        if weight is None:
            self._region = None
            return
        w = check_region_weight(weight, "set_region_weight")
        nw, H, W = w.shape
        f = self._features(nw, H, W)
        keys = TAPS_AFTER if self.net == "squeeze" else range(len(self.chns))
        om = region_tap_weights(w, [f.shapes[idx][1:] for idx in keys])
        bufs = self._region_taps.get((nw, H, W))
        if bufs is None:
            bufs = self._region_taps[(nw, H, W)] = [torch.empty(nw, o.shape[1] * o.shape[2], dtype=torch.float32, device=self.device_) for o in om]
        for b, o in zip(bufs, om):
            b.copy_(o.reshape(nw, -1))
        self._region = w
        self.pair_offset = None

    def _region_for(self, n, h, w):
        """(per-tap weight buffers, nw) of the weight that is set, checked against n candidates of size h x w; None without a weight."""
        if self._region is None:
            return None
        nw, H, W = self._region.shape
        if (H, W) != (h, w):
            raise ValueError(f"region weight is {H}x{W} but the images are {h}x{w}")
        if nw not in (1, n):
            raise ValueError(f"{nw} region weights cannot pair with {n} candidates")
        return self._region_taps[(nw, H, W)], nw

    def set_target(self, target):
        """Cache the target's feature maps, unit-normalised over channels (they do not change across projection iterations; the
        reference recomputes and re-normalises them every step).  One target [1,3,H,W] is shared by every candidate of
        `distance_into`; n targets pair up with n candidates (independent projections advanced in lockstep)."""
        n, _, h, w = target.shape
        self._target_n = n
        f = self._features(n, h, w)
        keys = TAPS_AFTER if self.net == "squeeze" else range(len(self.chns))
        shapes = [(n, c, *f.shapes[idx][1:]) for c, idx in zip(self.chns, keys)]
        old = getattr(self, "_target_taps", None)
        if old is not None and [tuple(t.shape) for t in old] == shapes:
            outs = old                # same geometry: rewrite the cached taps IN PLACE -- a captured hipGraph of the projection engine reads
        else:                         # these buffers (ProjectionEngine.retarget); every element is overwritten below
            outs = [torch.empty(sh, dtype=torch.float32, device=self.device_) for sh in shapes]
        if self.fused_stem and n == 1:
            # outs[0] holds the NORMALISED tap 0 (what the stem's distance mode compares against); the same kernel arithmetic
            # runs on both images, so identical images still give exactly zero
            f.stem(target.float().contiguous(), feat_out=outs[0])
            f(target.float(), out=outs, from_pooled=True)
        else:
            f(target.float(), out=outs)
        L, st = _lib.lib(), _lib.stream_ptr()
        for i, t in enumerate(outs):
            if i == 0 and self.fused_stem and n == 1:
                continue                            # the stem already wrote tap 0 normalised
            _lib.check(L.mgf_lpips_unit_f32(t.data_ptr(), t.data_ptr(), n, t.shape[1], t.shape[2] * t.shape[3], st), "lpips_unit")
        if self.spatial and self.fused_stem and n == 1:
            # the map takes the un-fused path (the stem never writes tap 0), so its target taps come from the un-fused path too: the SAME
            # kernels run on both images and identical images give an all-zero map exactly (outs, behind the stem, stay what distance_into reads)
            mt = self._map_taps
            if mt is None or [t.shape for t in mt] != [t.shape for t in outs]:
                mt = self._map_taps = [torch.empty_like(t) for t in outs]
            f(target.float(), out=mt)
            for t in mt:
                _lib.check(L.mgf_lpips_unit_f32(t.data_ptr(), t.data_ptr(), n, t.shape[1], t.shape[2] * t.shape[3], st), "lpips_unit")
        else:
            self._map_taps = None
        self._target_taps = outs
        self.pair_offset = None                     # a single target again: no constant to add (set_target_pair sets it afterwards)

    def set_target_pair(self, target_a, target_b, alpha):
        """Two targets per candidate, target_b weighted by alpha and target_a by 1 - alpha (drivers.merge_morph's convention).  With unit taps
        u_a, u_b every tap's term is quadratic in the candidate's unit tap u_x, so for weights that sum to one
            (1 - alpha) LPIPS(x, Ta) + alpha LPIPS(x, Tb) = sum_taps mean_hw sum_c lin_c (u_x - u)^2 + alpha (1 - alpha) LPIPS(Ta, Tb),
        u = (1 - alpha) u_a + alpha u_b: the cached taps become u (the tap kernels take the target map as data; nothing in them needs it to
        have unit norm) and `pair_offset` [B] holds the constant.  `distance_into` / `grad_into` then run exactly as for one target -- the caller
        adds pair_offset.  targets: [1,3,H,W], or [B,...] for B lockstep pairs; alpha: a float or B of them.  alpha exactly 0 or 1 keeps that
        target's taps as they are (a copy, no arithmetic).  Same geometry as before: taps and offset are rewritten in place (a captured
        hipGraph keeps reading them)."""
        _lib.require_gpu(target_a, target_b)
        if tuple(target_a.shape) != tuple(target_b.shape):
            raise ValueError(f"set_target_pair: the two targets differ in shape: {tuple(target_a.shape)} vs {tuple(target_b.shape)}")
        n = int(target_a.shape[0])
        al = np.asarray(alpha.detach().cpu() if isinstance(alpha, torch.Tensor) else alpha, dtype=np.float64).reshape(-1)
        if al.size not in (1, n) or not np.all((al >= 0.0) & (al <= 1.0)):
            raise ValueError(f"set_target_pair: alpha must be one value or {n} values in [0, 1] (got {alpha!r})")
        al = np.array(np.broadcast_to(al, (n,)))
        buf = getattr(self, "_pair_offset_buf", None)
        if buf is None or buf.numel() != n:
            buf = self._pair_offset_buf = torch.zeros(n, dtype=torch.float32, device=self.device_)
        self.set_target(target_b)
        ub = [t.clone() for t in self._target_taps]
        self.distance_into(buf, target_a.float().contiguous())                  # LPIPS(Ta, Tb), per pair, through the distance kernels
        buf.mul_(torch.as_tensor(al * (1.0 - al), dtype=torch.float32, device=self.device_))
        self.set_target(target_a)                                               # in place when the geometry is unchanged
        for t, b in zip(self._target_taps, ub):
            for i in range(n):
                a = float(al[i])
                if a == 1.0:
                    t[i].copy_(b[i])
                elif a != 0.0:
                    t[i].mul_(1.0 - a).add_(b[i], alpha=a)
        self.pair_offset = buf

    def grad_into(self, dimg, scale=1.0, accumulate=False):
        """dimg (+)= d(scale * distance)/d(pred) for the pred of the latest `distance_into(..., keep_taps=True)` call
        (what autograd computes through networks_basic.py:64-92 and the backbone).  SqueezeNet and VGG16 backbones."""
        f = self._last
        assert f is not None and tuple(dimg.shape) == (f.n, 3, *self._last_hw), "call distance_into(..., keep_taps=True) first"
        region = self._region_for(f.n, *self._last_hw)
        if region is None:
            g = f.backward(self._target_taps, self.lins, scale, per_sample=self._target_n > 1)
        else:
            g = f.backward(self._target_taps, self.lins, scale, per_sample=self._target_n > 1, region=region)
        if not accumulate:
            dimg.zero_()
        dimg[:, :, :g.shape[2], :g.shape[3]].add_(g)
        return dimg

    def distance_into(self, out, pred, keep_taps=False):
        """out[i] = sum over taps of the spatial-mean weighted distance between pred[i] and the cached (single) target.
        pred: [n,3,H,W]; out: float32 [n].  keep_taps=True takes the un-fused path so that every tap stays in the workspace
        for `grad_into`."""
        n = pred.shape[0]
        f = self._features(n, pred.shape[2], pred.shape[3])
        assert self._target_taps is not None, "call set_target first"
        per_sample = self._target_n > 1
        assert not per_sample or self._target_n == n, f"{self._target_n} targets cannot pair with {n} candidates"
        need = n * int(_lib.lib().mgf_reduce_scratch_floats())
        if self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.float32, device=self.device_)
        self._last, self._last_hw = (f, tuple(pred.shape[2:])) if keep_taps else (None, None)
        f.tap_stats = {}                            # tap index -> per-pixel sums of this forward (keep_taps only)
        region = self._region_for(n, pred.shape[2], pred.shape[3])
        if self.fused_stem and not keep_taps and not per_sample and region is None:
            f.stem(pred.contiguous(), feat_ref=self._target_taps[0], lin=self.lins[0], dist_out=out, scratch=self._scratch)
            taps = f(pred, from_pooled=True)
        else:
            taps = f(pred, argmax=True) if (keep_taps and self.net == "squeeze") else f(pred)
        L, st = _lib.lib(), _lib.stream_ptr()
        # every tap leaves its partial sums in a scratch set of its own; ONE finish launch adds them to `out` in tap order (the same sums
        # in the same order as a finish per tap: the value is a by-product nothing waits for)
        red = int(L.mgf_reduce_scratch_floats())
        ntaps = len(self.lins)
        if self._scratch.numel() < ntaps * n * red:
            self._scratch = torch.empty(ntaps * n * red, dtype=torch.float32, device=self.device_)
        import ctypes as C
        nparts, scales, k, first_done = (C.c_int32 * 8)(), (C.c_float * 8)(), 0, False
        for i, (a, b, lin) in enumerate(zip(taps, self._target_taps, self.lins)):
            if a is None:
                first_done = True                   # tap 0 was consumed inside the stem kernel, which wrote out itself
                continue
            _, c, hh, ww = a.shape
            stats = None
            if keep_taps and TAP_STATS:
                key = (i, n, hh * ww)
                stats = self._stats.get(key)
                if stats is None:
                    stats = self._stats[key] = torch.empty(n, 3, hh * ww, dtype=torch.float32, device=self.device_)
                f.tap_stats[i] = stats
            got = C.c_int32(0)
            if region is not None:                  # the partials are of omega[p] d[p] with omega normalised: no 1 / hw
                _lib.check(L.mgf_lpips_layer_defer_weighted_f32(self._scratch[k * n * red:].data_ptr(), _lib.ptr(stats), a.data_ptr(), b.data_ptr(),
                                                                lin.data_ptr(), region[0][i].data_ptr(), n, c, hh * ww,
                                                                c * hh * ww if per_sample else 0, hh * ww if region[1] > 1 else 0, C.byref(got), st),
                           "lpips_layer_weighted")
                nparts[k], scales[k] = got.value, 1.0
                k += 1
                continue
            _lib.check(L.mgf_lpips_layer_defer_f32(self._scratch[k * n * red:].data_ptr(), _lib.ptr(stats), a.data_ptr(), b.data_ptr(), lin.data_ptr(),
                                                   n, c, hh * ww, c * hh * ww if per_sample else 0, C.byref(got), st), "lpips_layer")
            nparts[k], scales[k] = got.value, 1.0 / float(hh * ww)
            k += 1
        _lib.check(L.mgf_lpips_finish_taps_f32(out.data_ptr(), self._scratch.data_ptr(), n * red, k, nparts, scales, n, int(first_done), st),
                   "lpips_finish_taps")
        return out

    def distance_per_tap(self, pred):
        """[taps, n]: every tap's own contribution to `distance_into`'s sum -- PNetLin.forward(retPerLayer=True)'s `res` list
        (networks_basic.py:85-92) -- through the SAME kernel dispatch as distance_into (fused stem included), each tap written to its
        own row instead of accumulated."""
        n = pred.shape[0]
        f = self._features(n, pred.shape[2], pred.shape[3])
        assert self._target_taps is not None, "call set_target first"
        per_sample = self._target_n > 1
        assert not per_sample or self._target_n == n
        need = n * int(_lib.lib().mgf_reduce_scratch_floats())
        if self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.float32, device=self.device_)
        out = torch.zeros(len(self.chns), n, dtype=torch.float32, device=self.device_)
        f.tap_stats = {}
        region = self._region_for(n, pred.shape[2], pred.shape[3])
        if self.fused_stem and not per_sample and region is None:
            f.stem(pred.contiguous(), feat_ref=self._target_taps[0], lin=self.lins[0], dist_out=out[0], scratch=self._scratch)
            taps = f(pred, from_pooled=True)
        else:
            taps = f(pred)
        L, st = _lib.lib(), _lib.stream_ptr()
        for i, (a, b, lin) in enumerate(zip(taps, self._target_taps, self.lins)):
            if a is None:
                continue
            _, c, hh, ww = a.shape
            if region is not None:
                import ctypes as C
                got, one = C.c_int32(0), (C.c_float * 8)(1.0)
                _lib.check(L.mgf_lpips_layer_defer_weighted_f32(self._scratch.data_ptr(), None, a.data_ptr(), b.data_ptr(), lin.data_ptr(),
                                                                region[0][i].data_ptr(), n, c, hh * ww, c * hh * ww if per_sample else 0,
                                                                hh * ww if region[1] > 1 else 0, C.byref(got), st), "lpips_layer_weighted")
                _lib.check(L.mgf_lpips_finish_taps_f32(out[i].data_ptr(), self._scratch.data_ptr(), n * int(L.mgf_reduce_scratch_floats()), 1,
                                                       (C.c_int32 * 8)(got.value), one, n, 0, st), "lpips_finish_taps")
                continue
            _lib.check(L.mgf_lpips_layer_stats_f32(out[i].data_ptr(), None, a.data_ptr(), b.data_ptr(), lin.data_ptr(), n, c, hh * ww,
                                                   c * hh * ww if per_sample else 0, 0, self._scratch.data_ptr(), st), "lpips_layer")
        return out

    @staticmethod
    def _require_square(H, W):
        if H != W:
            raise _lib.MgfError(f"PerceptualLoss(spatial=True): the image must be square (got {H}x{W}): the reference derives ONE scale factor from "
                                "the height and its tap maps then disagree in width")

    def _map_workspace(self, n, H, f):
        """Per-tap maps [n, h_l, h_l] for n images of side H (cached like `_stats`), after the size checks of spatial mode."""
        ws = self._map_ws.get((n, H))
        if ws is None:
            keys = TAPS_AFTER if self.net == "squeeze" else range(len(self.chns))
            sides = []
            for l, idx in enumerate(keys):
                _, hh, ww = f.shapes[idx]
                got = spatial_tap_output_side(hh, H)
                if hh != ww or got != H:
                    raise _lib.MgfError(f"PerceptualLoss(spatial=True, net={self.net!r}): tap {l} ({hh}x{ww}) up-samples to side {got}, not to the "
                                        f"image's {H} (the reference's own sum of the tap maps fails at this size)")
                sides.append(hh)
            ws = self._map_ws[(n, H)] = [torch.empty(n, s, s, dtype=torch.float32, device=self.device_) for s in sides]
        return ws

    def _upsample_sum(self, out, maps, accumulate=False):
        import ctypes as C
        n, H = out.shape[0], out.shape[-1]
        ptrs = (C.c_void_p * 8)(*[m.data_ptr() for m in maps])
        sides = (C.c_int32 * 8)(*[m.shape[-1] for m in maps])
        _lib.check(_lib.lib().mgf_lpips_upsample_sum_f32(out.data_ptr(), ptrs, sides, len(maps), n, H, int(accumulate), _lib.stream_ptr()),
                   "lpips_upsample_sum")
        return out

    def distance_map_into(self, out, pred, per_tap=None):
        """out[i,0,y,x] = sum over taps of the tap's per-pixel weighted distance between pred[i] and the cached target (`set_target`: one
        target for every candidate, or n targets for n candidates, as in `distance_into`), up-sampled bilinearly to the image size -- what
        PNetLin.forward returns with spatial=True (networks_basic.py:20-24,75-76,85-87).  pred: [n,3,H,H]; out: float32 [n,1,H,H].
        per_tap: a list of [n,1,H,H] tensors, one per tap, that receive every tap's own up-sampled map.  The un-fused path: every tap is in the
        workspace, as with keep_taps=True; the per-tap maps are cached per (n, H), nothing is allocated per call."""
        if not self.spatial:
            raise _lib.MgfError("distance_map_into: this PerceptualLoss was built with spatial=False")
        _lib.require_gpu(out, pred)
        n, _, H, W = pred.shape
        self._require_square(H, W)
        assert self._target_taps is not None, "call set_target first"
        if self.pair_offset is not None:
            raise _lib.MgfError("distance_map_into: a target pair is set (set_target_pair); the map is defined against one target")
        per_sample = self._target_n > 1
        assert not per_sample or self._target_n == n, f"{self._target_n} targets cannot pair with {n} candidates"
        assert tuple(out.shape) == (n, 1, H, H) and out.dtype == torch.float32 and out.is_contiguous(), "out: contiguous float32 [n,1,H,H]"
        f = self._features(n, H, W)
        maps = self._map_workspace(n, H, f)
        self._last, self._last_hw = None, None
        f.tap_stats = {}
        taps = f(pred.float())
        L, st = _lib.lib(), _lib.stream_ptr()
        targets = self._target_taps if self._map_taps is None else self._map_taps
        for a, b, lin, m in zip(taps, targets, self.lins, maps):
            _, c, hh, ww = a.shape
            _lib.check(L.mgf_lpips_layer_map_f32(m.data_ptr(), a.data_ptr(), b.data_ptr(), lin.data_ptr(), n, c, hh * ww,
                                                 c * hh * ww if per_sample else 0, st), "lpips_layer_map")
        self._upsample_sum(out, maps)
        if per_tap is not None:
            assert len(per_tap) == len(maps)
            for o, m in zip(per_tap, maps):
                assert tuple(o.shape) == (n, 1, H, H) and o.dtype == torch.float32 and o.is_contiguous()
                self._upsample_sum(o, [m])
        return out

    def forward(self, pred, target, normalize=False, retPerLayer=False):
        """spatial=False: [N,1,1,1].  spatial=True: the float32 [N,1,H,W] map, and with retPerLayer=True (val, [per-tap up-sampled maps]).
        The list is un-aliased: every entry is a tap's own map.  In the reference, `val = res[0]` followed by the in-place `val += res[l]`
        (networks_basic.py:85-87) makes res[0] the running total, not tap 0's map."""
        _lib.require_gpu(pred, target)
        if normalize:
            target, pred = 2 * target - 1, 2 * pred - 1
        n = pred.shape[0]
        if self.spatial:
            H, W = pred.shape[2:]
            self._require_square(H, W)
            self.set_target(target.float().contiguous())          # n targets for n images, or one for all of them
            val = torch.empty(n, 1, H, W, dtype=torch.float32, device=self.device_)
            res = [torch.empty_like(val) for _ in self.lins] if retPerLayer else None
            self.distance_map_into(val, pred.float().contiguous(), per_tap=res)
            return (val, res) if retPerLayer else val
        if retPerLayer:
            raise NotImplementedError("retPerLayer=True is implemented for spatial=True; `distance_per_tap` returns the per-tap values otherwise")
        if self._region is not None and self._region.shape[0] > 1:
            # one region weight per image: n targets pair up with n images and n weights in one evaluation
            self.set_target(target.float().contiguous())
            vals = torch.empty(n, dtype=torch.float32, device=self.device_)
            self.distance_into(vals, pred.float().contiguous())
            return vals.reshape(n, 1, 1, 1)
        vals = []
        for i in range(n):      # per-sample values like the reference's [N,1,1,1]; the loop only ever uses N == 1
            # like the reference, the module-call form recomputes the target features on every call; the projection
            # engine uses set_target() once + distance_into() per step instead
            self.set_target(target[i:i + 1].contiguous())
            self.distance_into(self._val, pred[i:i + 1].contiguous().float())
            vals.append(self._val.clone())
        return torch.stack(vals).reshape(n, 1, 1, 1)
