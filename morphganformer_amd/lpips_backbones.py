"""The LPIPS backbones: layer specs, seeded weights and the tap extractors (forward and backward) of SqueezeNet1.1 (`SqueezeFeatures`) and
of the plain conv / ReLU / max-pool stacks VGG16 and AlexNet (`SequentialFeatures`) for a fixed input size.  `TapFeatures` is what the two
share: the state `PerceptualLoss` (lpips.py) reads and writes, the tap's distance-gradient dispatch, the ReLU backward and the hand-over of
size-independent packs between instances."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import _lib, misc
from . import conv as cv

FIRES = {3: (64, 16, 64), 4: (128, 16, 64), 6: (128, 32, 128), 7: (256, 32, 128),
         9: (256, 48, 192), 10: (384, 48, 192), 11: (384, 64, 256), 12: (512, 64, 256)}
TAPS_AFTER = [1, 4, 7, 9, 10, 11, 12]
POOLS = [2, 5, 8]
CHNS = [64, 128, 256, 384, 384, 512, 512]
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# The Fire expand3x3 convs (16..64 input channels, 255 / 127 / 63 px maps, output = a channel slice of the concat buffer) run on the form-3
# Winograd kernel: few chunks per tile is exactly where its 32x32-tile shape with four workgroups per CU pays (with form 2 they were
# slower than the tap-list kernel, 481 vs 486 iters/s).  MGF_WINOGRAD_LPIPS=0 (tuning hook) puts them back on the tap-list kernel.
USE_WINOGRAD_LPIPS = os.environ.get("MGF_WINOGRAD_LPIPS", "1") != "0"
# a tap's distance gradient and the backward of the ReLU whose output the tap is, in one pass (mgf_lpips_layer_bwd_relu_f32);
# 0: the two kernels in sequence (experiments / test_lpips_switches_equal_the_default_dispatch, as for the next two)
FUSE_TAP_RELU = os.environ.get("MGF_FUSE_TAP_RELU", "1") != "0"
# gradient mode: SqueezeNet's pools store their winning taps in the forward and the backward reads those (0: argmax recomputed from the
# input map in the backward)
POOL_ARGMAX = os.environ.get("MGF_POOL_ARGMAX", "1") != "0"
# gradient mode: the tap distances also store their per-pixel sums and the tap gradients read them instead of sweeping both maps again
TAP_STATS = os.environ.get("MGF_TAP_STATS", "1") != "0"
# ONE image per forward (gradient mode with a single target): a Fire's two expand branches run as ONE 3x3 launch -- expand1x1's weights sit in
# the centre tap of 2 x ex output channels' worth of 3x3 kernels -- and their data gradients as one 3x3 launch over the concatenated gradient.
# At one image these layers sit on their launch latency (8 - 25 us each), so the extra matrix work of the 1x1 computed as a 3x3 is free and a
# launch per Fire and direction disappears; from two images on the separate launches are kept (0: always separate;
# test_lpips_merged_fire_launches_equal_the_separate_ones)
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
    out = {k: misc.as_numpy(v, np.float32) for k, v in raw.items() if k.startswith("features.")}
    if not out:
        raise _lib.MgfError(f"{path}: no `features.*` entries (expected a torchvision squeezenet1_1 / vgg16 / alexnet state dict)")
    return out


class TapFeatures:
    """What the two backbones share.  `tap_shapes`: (c, h, w) of every LPIPS tap, in tap order; `tap_stats`: tap index -> per-pixel sums of
    the latest forward (`PerceptualLoss.distance_into(keep_taps=True)` fills it, the tap gradients read it); `_SHARED`: the attributes that
    do not depend on the input size and that a new instance takes over from `share` -- the dictionaries by identity, the lazily filled
    packs of the backward pass among them."""
    _SHARED = ()

    def __init__(self, n, device, share):
        self.device, self.n = torch.device(device), n
        self.tap_shapes, self.tap_stats = [], {}
        self.gbufs = None                                  # the gradient workspace: allocated by the first `backward`
        for name in self._SHARED if share is not None else ():
            setattr(self, name, getattr(share, name))

    def _tap_grad(self, k, h, da, db, split, din, fused, target_taps, lins, per_sample, region, scale):
        """Tap k's distance gradient, scale * d lpips_layer(h, target_taps[k]) / dh.  fused: in one pass with the backward of the ReLU whose
        output h is, on top of the gradient from behind `din` (None: there is none), into da -- or split at channel `split` into da | db.
        Otherwise the plain form: written to da, or added to it where a gradient from behind is in it (din, then da itself).
        region: (per-tap normalised weights, nw) -- the weighted forms."""
        L, st = _lib.lib(), _lib.stream_ptr()
        n, c, hh, ww = h.shape
        hw, maps = hh * ww, (h.data_ptr(), target_taps[k].data_ptr(), lins[k].data_ptr())
        tstride, stats = (c * hw if per_sample else 0), _lib.ptr(self.tap_stats.get(k))
        wm, ws = (None, 0) if region is None else (region[0][k].data_ptr(), hw if region[1] > 1 else 0)
        if fused and region is not None:
            rc, what = L.mgf_lpips_layer_bwd_relu_stats_weighted_f32(da.data_ptr(), _lib.ptr(db), _lib.ptr(din), *maps, stats, wm, n, c, split, hw,
                                                                     tstride, ws, float(scale), st), "lpips_layer_bwd_relu_weighted"
        elif fused:
            rc, what = L.mgf_lpips_layer_bwd_relu_stats_f32(da.data_ptr(), _lib.ptr(db), _lib.ptr(din), *maps, stats, n, c, split, hw, tstride,
                                                            float(scale), st), "lpips_layer_bwd_relu"
        elif region is not None:
            rc, what = L.mgf_lpips_layer_bwd_weighted_f32(da.data_ptr(), *maps, wm, n, c, hw, tstride, ws, float(scale), int(din is not None),
                                                          st), "lpips_layer_bwd_weighted"
        else:
            rc, what = L.mgf_lpips_layer_bwd_f32(da.data_ptr(), *maps, n, c, hw, tstride, float(scale), int(din is not None), st), "lpips_layer_bwd"
        _lib.check(rc, what)

    @staticmethod
    def _relu_bwd(g, y, da=None, db=None):
        """g through the ReLU whose output is y: in place, or (a Fire's concat) split into the two expand gradients da | db."""
        n, c, hh, ww = y.shape
        a = g if da is None else da
        _lib.check(_lib.lib().mgf_relu_bwd_split_f32(a.data_ptr(), _lib.ptr(db), g.data_ptr(), y.data_ptr(), n, c, a.shape[1], hh * ww,
                                                     _lib.stream_ptr()), "relu_bwd" if db is None else "relu_bwd_split")


class SequentialFeatures(TapFeatures):
    """LPIPS taps of a plain conv/ReLU/max-pool stack (VGG16, AlexNet) for a fixed input size, preallocated workspace.
    The ScalingLayer runs as its own element-wise step (these nets zero-pad the SCALED input, so it cannot be folded)."""
    _SHARED = ("convs", "first4", "shift", "scale", "gp")

    def __init__(self, net, backbone_state, n, h, w, device, share=None):
        super().__init__(n, device, share)
        dev = self.device
        self.spec = SPECS[net]
        t32 = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a), dtype=np.float32), device=dev)
        if share is None:
            self.gp = {}                                   # channel-transposed packs of the backward pass, built on first use
            # (Conv3x3 | [cout, cin, k, k] weights of the layers with > 9 taps: packed per tap group at run time, bias) of every conv.
            # 3x3 / stride-1 / pad-1 layers with whole 32-channel tiles (every VGG16 layer but the first, AlexNet's last three): Winograd
            # F(2x2,3x3) form 3 when the launch fills the chip -- 4/9 of the matrix work of the tap-list kernel, which runs these layers at
            # 0.80 of the FP32-MFMA peak and cannot get much closer (MGF_WINOGRAD_LPIPS=0: tap-list kernel everywhere)
            self.convs, self.first4 = {}, None
            for row in self.spec:
                if row[0] == "conv":
                    _, idx, ci, co, k, st_, pd_ = row
                    assert k != 3 or (st_, pd_) == (1, 1)
                    wt, b = t32(backbone_state[f"features.{idx}.weight"]), t32(backbone_state[f"features.{idx}.bias"])
                    self.convs[idx] = (cv.pack_conv3x3(wt, winograd=USE_WINOGRAD_LPIPS and ci % 4 == 0 and co % 32 == 0) if k == 3 else wt, b)
                    if USE_WINOGRAD_LPIPS and k == 3 and ci == 3 and co % 32 == 0 and row is self.spec[0]:
                        # VGG16's first layer (3 -> 64 at the full image size: 4.3 GB of output per 16 images, 58 GFLOP): a FOURTH, all-zero
                        # input channel makes it a Winograd launch (the tap-list kernel stages 3 channels synchronously: 2.85 ms per 16 images)
                        self.first4 = cv.pack_conv3x3(torch.cat([wt, torch.zeros_like(wt[:, :1])], dim=1).contiguous(), winograd=True)
            self.shift, self.scale = t32(SHIFT).reshape(1, 3, 1, 1), t32(SCALE).reshape(1, 3, 1, 1)
        e = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        self.xs = e(n, 3, h, w)
        # the scaled input with a fourth, zero channel: what the first layer's Winograd form reads (see above)
        self.xs4 = (torch.zeros(n, 4, h, w, dtype=torch.float32, device=dev)
                    if self.first4 is not None and cv.conv3x3_takes_winograd(self.first4, n, h, w) else None)
        self.bufs, self.shapes = [], {}
        c, hh, ww = 3, h, w
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
                self.shapes[len(self.tap_shapes)] = (c, hh, ww)
                self.tap_shapes.append((c, hh, ww))

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
                    h = cv.winograd2_forward(self.xs4, self.first4.u, epilogue=_lib.make_epilogue(bias=b, act="relu"), out=dst)
                elif k == 3:
                    h = cv.conv3x3_forward(h, wt, epilogue=_lib.make_epilogue(bias=b, act="relu"), out=dst)
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
                    self.gp[row[1]] = cv.transpose_packed(self.convs[row[1]][0].pc, flip=True)
        if self.gbufs is None:
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
            c = h.shape[1]
            behind = pos != len(nodes) - 1                     # a gradient from the rows behind this one is already in gh
            fused = FUSE_TAP_RELU and i in tap_of and row[0] == "conv"
            if i in tap_of:
                self._tap_grad(tap_of[i], h, gh, None, c, gh if behind else None, fused, target_taps, lins, per_sample, region, scale)
            prev = self.bufs[nodes[pos - 1]] if pos > 0 else self.xs
            gprev = self.gbufs[nodes[pos - 1]] if pos > 0 else self.gxs
            if row[0] == "conv":
                if not fused:
                    self._relu_bwd(gh, h)
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


def _pool_out(n):
    o = (n - 3 + 1) // 2 + 1
    if (o - 1) * 2 >= n:
        o -= 1
    return o


class SqueezeFeatures(TapFeatures):
    """The 7 LPIPS taps of SqueezeNet1.1 for a fixed input size, with a preallocated workspace."""
    _SHARED = ("c0", "fires", "merged", "stem_w", "stem_b", "gp", "gpm")   # packed weights are size independent

    def __init__(self, backbone_state, n, h, w, device, share=None):
        super().__init__(n, device, share)
        dev = self.device
        if share is None:
            self.gp = {}                                          # channel-transposed packs of the backward pass (+ Winograd images), built on first use
            self.gpm = {}                                         # ... of the merged expand launch (one image per forward)
            g = lambda k: np.asarray(backbone_state[k], dtype=np.float64)
            t32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)
            w0, b0 = g("features.0.weight"), g("features.0.bias")
            sc, sh = np.asarray(SCALE), np.asarray(SHIFT)
            w0f = w0 / sc[None, :, None, None]
            b0f = b0 - (w0 * (sh / sc)[None, :, None, None]).sum(axis=(1, 2, 3))
            self.c0 = (cv.pack_weights(t32(w0f)), t32(b0f))
            self.stem_w, self.stem_b = t32(w0f.reshape(64, 27)), t32(b0f)       # operands of the fused stem kernel
            # (squeeze, expand1x1: PackedConv; expand3x3: Conv3x3 with its Winograd planes -- odd maps, concat slice), each with its bias
            self.fires = {}
            for idx in FIRES:
                p = f"features.{idx}"
                wt, bs = (lambda nm: t32(g(f"{p}.{nm}.weight"))), (lambda nm: t32(g(f"{p}.{nm}.bias")))
                self.fires[idx] = ((cv.pack_weights(wt("squeeze")), bs("squeeze")), (cv.pack_weights(wt("expand1x1")), bs("expand1x1")),
                                   (cv.pack_conv3x3(wt("expand3x3"), winograd=USE_WINOGRAD_LPIPS), bs("expand3x3")))
            # the merged expand launch of the one-image path (MERGE_FIRE): [2 ex, sq, 3, 3], expand1x1 in the centre tap of the first ex kernels
            self.merged = {}
            for idx in FIRES:
                p = f"features.{idx}"
                w1, w3 = g(f"{p}.expand1x1.weight"), g(f"{p}.expand3x3.weight")
                wm = np.zeros((2 * w1.shape[0], w1.shape[1], 3, 3))
                wm[:w1.shape[0], :, 1, 1] = w1[:, :, 0, 0]
                wm[w1.shape[0]:] = w3
                bm = np.concatenate([g(f"{p}.expand1x1.bias"), g(f"{p}.expand3x3.bias")])
                self.merged[idx] = (cv.pack_conv3x3(t32(wm), winograd=USE_WINOGRAD_LPIPS), t32(bm))
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
                if MERGE_FIRE and n == 1 and cv.conv3x3_takes_winograd(self.merged[idx][0], n, hh, ww):
                    self.merge.add(idx)
                c = 2 * ex
                self.buf[idx] = e(n, c, hh, ww)
            self.shapes[idx] = (c, hh, ww)
        self.tap_shapes = [self.shapes[idx] for idx in TAPS_AFTER]

    def _grad_ws(self):
        """Workspace + transposed taps of `backward` (gradient mode only, allocated on first use)."""
        if not self.gp:
            self.gp["c0"] = cv.transpose_packed(self.c0[0], flip=False)       # stride-2 conv -> stride-2 transposed conv, same taps
            for idx, ((ps, _), (p1, _), (p3, _)) in self.fires.items():
                # the expand-3x3 data gradient (E -> S channels) on the Winograd kernel where S is a multiple of its 32-channel tile
                # (the forms-2/3 planes whatever this instance's map size: the packs are shared between sizes)
                self.gp[idx] = (cv.transpose_packed(ps, False), cv.transpose_packed(p1, False),
                                cv.transpose_conv3x3(p3, winograd=USE_WINOGRAD_LPIPS and p3.cin % 32 == 0))
            for idx, (pm, _) in self.merged.items():
                # the merged data gradient: one true convolution over the concatenated gradient [d expand1x1 | d expand3x3] (2 ex -> sq channels)
                self.gpm[idx] = cv.transpose_conv3x3(pm, winograd=USE_WINOGRAD_LPIPS and pm.cin % 32 == 0)
        if self.gbufs is None:
            e = lambda t: torch.empty_like(t)
            self.gbufs = {idx: e(t) for idx, t in self.buf.items()}
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
            h, gh = self.buf[idx], self.gbufs[idx]
            c, hh, ww = h.shape[1:]
            # every tap is a ReLU output (the stem's, or a Fire's concat): its distance gradient and that ReLU's backward (with the
            # Fire's split into the two expand branches) are one pass
            fused = FUSE_TAP_RELU and idx in TAPS_AFTER and idx not in POOLS
            if idx in TAPS_AFTER:
                da, db, ex = (gh, None, c) if (idx == 1 or not fused) else (*self.gex[idx], FIRES[idx][2])
                self._tap_grad(TAPS_AFTER.index(idx), h, da, db, ex, gh if idx != 12 else None, fused, target_taps, lins, per_sample, region, scale)
            if idx == 1:
                if not fused:
                    self._relu_bwd(gh, h)
                return cv.tconv3x3s2_forward(gh, self.gp["c0"], out=self.gimg)
            if idx in POOLS:
                x = self.buf[idx - 1]
                if self.have_argmax:
                    _lib.check(L.mgf_maxpool3x3s2_ceil_bwd_idx_f32(self.gbufs[idx - 1].data_ptr(), gh.data_ptr(), self.pidx[idx].data_ptr(), n * c,
                                                                   x.shape[2], x.shape[3], hh, ww, st), "maxpool_bwd_idx")
                else:
                    _lib.check(L.mgf_maxpool3x3s2_ceil_bwd_f32(self.gbufs[idx - 1].data_ptr(), gh.data_ptr(), x.data_ptr(), n * c, x.shape[2],
                                                               x.shape[3], hh, ww, st), "maxpool_bwd")
                continue
            sqT, e1T, e3T = self.gp[idx]
            da, db = self.gex[idx]
            if not fused:
                self._relu_bwd(gh, h, da, db)
            s, gs = self.sq[idx], self.gsq[idx]
            if idx in self.merge:
                cv.conv3x3_forward(self.gcat[idx], self.gpm[idx], out=gs)
            else:
                cv.conv_forward(da, e1T, out=gs)
                cv.conv3x3_forward(db, e3T, epilogue=_lib.make_epilogue(residual=gs), out=gs)
            self._relu_bwd(gs, s)
            cv.conv_forward(gs, sqT, out=self.gbufs[idx - 1])
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
        self.have_argmax = bool(argmax) and not from_pooled and POOL_ARGMAX

        def dest(idx):
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
                    pm, bm = self.merged[idx]
                    cv.conv3x3_forward(s, pm, epilogue=_lib.make_epilogue(bias=bm, act="relu"), out=y)
                    h = y
                    if idx in TAPS_AFTER:
                        taps.append(h)
                    continue
                cv.conv_forward(s, p1, epilogue=_lib.make_epilogue(bias=b1, act="relu"), out=y, out_choff=0)
                # Winograd when its grid (no split-K) fills the chip: the 25-candidate literal iteration, not a single small image
                cv.conv3x3_forward(s, p3, epilogue=_lib.make_epilogue(bias=b3, act="relu"), out=y, out_choff=ex)
                h = y
            if idx in TAPS_AFTER:
                taps.append(h)
        return taps
