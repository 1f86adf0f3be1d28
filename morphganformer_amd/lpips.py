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
  * `pool_above=N` block-averages every image taller than N by height // N in front of the backbone (projection_example_v1.py:148-155, for
    this term only) and `grad_into` applies the adjoint: callers hand in and get back full-size tensors (csrc/block_pool.hip).
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib, misc
from . import lpips_backbones as backbones          # the switches are read through the module (tests and tools set them there)
from .lpips_backbones import (ALEX_SPEC, CHNS, FIRES, NET_CHNS, POOLS, SCALE, SHIFT, SPECS, TAPS_AFTER, VGG_SPEC,  # noqa: F401 (re-exported)
                              SequentialFeatures, SqueezeFeatures, _pool_out, load_backbone_state, random_backbone, random_squeeze_backbone)

WEIGHTS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "weights")


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

def spatial_tap_output_side(h, H):
    """Side of a tap map of side h after the reference's `upsample(..., out_H=H)` (networks_basic.py:20-24): it hands torch the scale factor
    1. * H / h, and torch sizes the output floor(h * scale) in double -- which is not always H (47 * (96 / 47) floors to 95)."""
    return int(math.floor(float(h) * (1.0 * H / h)))


class PerceptualLoss(torch.nn.Module):
    """lpips.PerceptualLoss(model='net-lin', net='squeeze', use_gpu=True)(pred, target, normalize=False) -> [N,1,1,1];
    with spatial=True -> the [N,1,H,W] map of PNetLin(spatial=True) (networks_basic.py:75-76,85-92; `distance_map_into`)."""

    def __init__(self, model="net-lin", net="squeeze", colorspace="rgb", spatial=False, use_gpu=True, gpu_ids=(0,),
                 backbone_state=None, backbone_seed=None, allow_random_backbone=False, device="cuda", pool_above=0):
        """backbone_state: the torchvision feature weights (`features.N...` keys, tensors or arrays; `load_backbone_state` reads a
        .pth / .npz) -- what the reference obtains with tv.<net>(pretrained=True) (pretrained_networks.py:9,60,100).  Without it
        the distance would be computed on meaningless features, so that is an ERROR unless the caller opts in to the seeded random
        backbone (allow_random_backbone=True or an explicit backbone_seed: benchmarks and parity tests, where only the arithmetic
        matters).
        pool_above: an image [n,3,H,W] with H > pool_above is block-averaged by f = H // pool_above in front of the backbone (0 = off; the
        rule of ProjectionArgs.pool_above, misc.pool_factor, for this term alone): targets, candidates and region weights are given at
        their full size, `grad_into` fills a full-size gradient.  An image at or below pool_above goes through untouched."""
        super().__init__()
        if model != "net-lin" or colorspace != "rgb":
            raise NotImplementedError("the MI355X path implements model='net-lin', colorspace='rgb'")
        self.spatial = bool(spatial)
        self.pool_above = int(pool_above)
        if self.pool_above < 0:
            raise _lib.MgfError(f"PerceptualLoss(pool_above={pool_above!r}): a size in pixels, or 0 for no pooling")
        if self.spatial and self.pool_above:
            raise _lib.MgfError("PerceptualLoss(spatial=True, pool_above=...): the map is defined at the image's own size; a map of the "
                                "pooled image is not built")
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
        self._pooled = {}                 # (n, H, W) -> the block-averaged image [n,3,H/f,W/f] (pool_above); allocated on first use
        self._stats = {}
        self._map_ws = {}                 # (n, H) -> per-tap maps of distance_map_into (spatial=True)
        self._map_taps = None             # spatial=True beside the fused stem: the target's unit taps through the un-fused path
        self._target_taps = None
        self._target_n = 1
        self.pair_offset = None           # [B] float32 = alpha (1 - alpha) LPIPS(Ta, Tb) while a target pair is set (set_target_pair)
        self._pair_offset_buf = None      # ... its buffer, kept across pairs of the same count (a captured graph reads it)
        self._last, self._last_hw = None, None
        self._region = None               # float64 [nw, H, W] on the CPU while a region weight is set (set_region_weight), at the backbone's size
        self._region_given = None         # ... and the (H, W) it was handed in at (the images' own size; differs under pool_above)
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

    def _pool_factor(self, H, W):
        """Block side for H x W images (1: not pooled); MgfError when the image is not a whole number of blocks."""
        f = misc.pool_factor(H, self.pool_above)
        if f > 1 and (H % f or W % f):
            raise _lib.MgfError(f"PerceptualLoss(pool_above={self.pool_above}): a {H}x{W} image is not a whole number of {f}x{f} blocks "
                                f"(f = {H} // {self.pool_above})")
        return f

    def _pool(self, img):
        """img [n,3,H,W] as the backbone sees it: itself, or under pool_above its block mean in the buffer cached for (n, H, W)."""
        if not self.pool_above:
            return img
        n, c, H, W = img.shape
        f = self._pool_factor(H, W)
        if f == 1:
            return img
        _lib.require_gpu(img)
        x = img.float().contiguous()
        out = self._pooled.get((n, H, W))
        if out is None:
            out = self._pooled[(n, H, W)] = torch.empty(n, c, H // f, W // f, dtype=torch.float32, device=self.device_)
        _lib.check(_lib.lib().mgf_block_mean_f32(out.data_ptr(), x.data_ptr(), n * c, H, W, f, _lib.stream_ptr()), "block_mean")
        return out

    def set_region_weight(self, weight):
        """Weight the distance by region: weight [H,W], [1,1,H,W] (one map for every candidate) or [n,1,H,W] (one per candidate) >= 0 at the
        image size (the full size under pool_above: the weight is block-averaged like the images, in float64 on the host); None: the uniform
        spatial mean again, with today's dispatch (fused stem included).  Per tap the weight is pooled to the tap's grid and normalised (`region_tap_weights`), and `distance_into`, `grad_into`, `distance_per_tap` and the scalar module call
        compute sum_l sum_p omega_l[p] m_l[p] on the un-fused path (the fused stem consumes tap 0 with a uniform mean).  `distance_map_into`
        is unaffected.  The per-tap weights live in buffers that are rewritten in place while the geometry stays (captured graphs read
        them).  With a target pair set, call `set_target_pair` again afterwards: its constant depends on the weight."""
        if weight is None:
            self._region = self._region_given = None
            return
        w = check_region_weight(weight, "set_region_weight")
        given = tuple(w.shape[1:])
        f = self._pool_factor(*given)
        if f > 1:
            w = w.reshape(w.shape[0], given[0] // f, f, given[1] // f, f).mean(dim=(2, 4)).contiguous()
        nw, H, W = w.shape
        om = region_tap_weights(w, [s[1:] for s in self._features(nw, H, W).tap_shapes])
        bufs = self._region_taps.get((nw, H, W))
        if bufs is None:
            bufs = self._region_taps[(nw, H, W)] = [torch.empty(nw, o.shape[1] * o.shape[2], dtype=torch.float32, device=self.device_) for o in om]
        for b, o in zip(bufs, om):
            b.copy_(o.reshape(nw, -1))
        self._region, self._region_given = w, given
        self.pair_offset = None

    def _region_for(self, n, h, w, full=None):
        """(per-tap weight buffers, nw) of the weight that is set, checked against n candidates of size h x w at the backbone (the pooled
        size under pool_above; full: the size they were handed in at); None without a weight."""
        if self._region is None:
            return None
        nw, H, W = self._region.shape
        if (H, W) != (h, w):
            raise ValueError(f"region weight is {H}x{W} but the images are {h}x{w}")
        if full is not None and tuple(full) != self._region_given:          # (pool_above: a weight handed in at the pooled size)
            raise ValueError(f"region weight was given at {self._region_given[0]}x{self._region_given[1]} but the images are {full[0]}x{full[1]}")
        if nw not in (1, n):
            raise ValueError(f"{nw} region weights cannot pair with {n} candidates")
        return self._region_taps[(nw, H, W)], nw

    def set_target(self, target):
        """Cache the target's feature maps, unit-normalised over channels (they do not change across projection iterations; the
        reference recomputes and re-normalises them every step).  One target [1,3,H,W] is shared by every candidate of
        `distance_into`; n targets pair up with n candidates (independent projections advanced in lockstep)."""
        target = self._pool(target)
        n, _, h, w = target.shape
        self._target_n = n
        f = self._features(n, h, w)
        shapes = [(n, c, *s[1:]) for c, s in zip(self.chns, f.tap_shapes)]
        old = self._target_taps
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
        self._unit(outs, skip_first=self.fused_stem and n == 1)          # (the stem already wrote tap 0 normalised)
        if self.spatial and self.fused_stem and n == 1:
            # the map takes the un-fused path (the stem never writes tap 0), so its target taps come from the un-fused path too: the SAME
            # kernels run on both images and identical images give an all-zero map exactly (outs, behind the stem, stay what distance_into reads)
            mt = self._map_taps
            if mt is None or [t.shape for t in mt] != [t.shape for t in outs]:
                mt = self._map_taps = [torch.empty_like(t) for t in outs]
            f(target.float(), out=mt)
            self._unit(mt)
        else:
            self._map_taps = None
        self._target_taps = outs
        self.pair_offset = None                     # a single target again: no constant to add (set_target_pair sets it afterwards)

    @staticmethod
    def _unit(taps, skip_first=False):
        """Normalise every tap map over its channels, in place."""
        for t in taps[1:] if skip_first else taps:
            _lib.check(_lib.lib().mgf_lpips_unit_f32(t.data_ptr(), t.data_ptr(), t.shape[0], t.shape[1], t.shape[2] * t.shape[3], _lib.stream_ptr()),
                       "lpips_unit")

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
        al = misc.as_numpy(alpha, np.float64).reshape(-1)
        if al.size not in (1, n) or not np.all((al >= 0.0) & (al <= 1.0)):
            raise ValueError(f"set_target_pair: alpha must be one value or {n} values in [0, 1] (got {alpha!r})")
        al = np.array(np.broadcast_to(al, (n,)))
        buf = self._pair_offset_buf
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
        (what autograd computes through networks_basic.py:64-92 and the backbone).  SqueezeNet and VGG16 backbones.  dimg has that pred's
        own size: under pool_above the backward pass runs at the pooled size and the block mean's adjoint spreads it over dimg."""
        f = self._last
        assert f is not None and tuple(dimg.shape) == (f.n, 3, *self._last_hw[0]), "call distance_into(..., keep_taps=True) first"
        full, pooled = self._last_hw
        g = f.backward(self._target_taps, self.lins, scale, per_sample=self._target_n > 1, region=self._region_for(f.n, *pooled, full=full))
        if full != pooled:
            # g is a view of the backbone's input gradient (it may stop short of the pooled image): its own extent, pitch and plane stride
            assert dimg.dtype == torch.float32 and dimg.is_contiguous() and g.stride(3) == 1 and g.stride(0) == 3 * g.stride(1)
            _lib.check(_lib.lib().mgf_block_mean_adjoint_f32(dimg.data_ptr(), g.data_ptr(), f.n * 3, full[0], full[1], full[0] // pooled[0],
                                                             g.shape[2], g.shape[3], g.stride(2), g.stride(1), int(bool(accumulate)),
                                                             _lib.stream_ptr()), "block_mean_adjoint")
            return dimg
        if not accumulate:
            dimg.zero_()
        dimg[:, :, :g.shape[2], :g.shape[3]].add_(g)
        return dimg

    def _forward_taps(self, pred, keep_taps=False, out=None, scalar=True):
        """The shared head of the distance methods -> (f, taps, per_sample, region, out): the workspace of pred's size, the target count
        checked against pred's, the reduce scratch, `tap_stats` reset, the region weight that is set, and the forward -- the fused stem
        (which adds tap 0 to out [n], or writes row 0 of out [taps, n]; entry 0 of taps is then None) where nothing needs tap 0 itself.
        keep_taps: None leaves what `grad_into` reads alone.  out=None: the [taps, n] rows of `distance_per_tap` are allocated here.
        scalar=False (the map): no scratch, no region weight, every tap in the workspace.  Under pool_above pred is block-averaged first."""
        full = tuple(pred.shape[2:])
        pred = self._pool(pred)
        n, _, h, w = pred.shape
        f = self._features(n, h, w)
        assert self._target_taps is not None, "call set_target first"
        per_sample = self._target_n > 1
        assert not per_sample or self._target_n == n, f"{self._target_n} targets cannot pair with {n} candidates"
        if scalar:
            need = n * int(_lib.lib().mgf_reduce_scratch_floats())
            if self._scratch.numel() < need:
                self._scratch = torch.empty(need, dtype=torch.float32, device=self.device_)
            if out is None:
                out = torch.zeros(len(self.chns), n, dtype=torch.float32, device=self.device_)
        if keep_taps is not None:
            self._last, self._last_hw = (f, (full, (h, w))) if keep_taps else (None, None)      # (the size handed in, the backbone's)
        f.tap_stats = {}                            # tap index -> per-pixel sums of this forward (keep_taps only)
        region = self._region_for(n, h, w, full=full) if scalar else None
        if scalar and self.fused_stem and not keep_taps and not per_sample and region is None:
            f.stem(pred.contiguous(), feat_ref=self._target_taps[0], lin=self.lins[0], dist_out=out if out.dim() == 1 else out[0],
                   scratch=self._scratch)
            taps = f(pred, from_pooled=True)
        else:
            taps = f(pred, argmax=True) if (keep_taps and self.net == "squeeze") else f(pred)
        return f, taps, per_sample, region, out

    def _defer_tap(self, i, a, scratch, stats, per_sample, region):
        """Launch tap i's distance of the map a against the cached target: partial sums into scratch (the finish launch adds them up), the
        per-pixel sums into stats where given -> (number of partials, the factor the finish launch applies to them)."""
        n, c, hh, ww = a.shape
        L, st, hw, got = _lib.lib(), _lib.stream_ptr(), hh * ww, C.c_int32(0)
        maps = (a.data_ptr(), self._target_taps[i].data_ptr(), self.lins[i].data_ptr())
        if region is not None:                      # the partials are of omega[p] d[p] with omega normalised: no 1 / hw
            _lib.check(L.mgf_lpips_layer_defer_weighted_f32(scratch.data_ptr(), _lib.ptr(stats), *maps, region[0][i].data_ptr(), n, c, hw,
                                                            c * hw if per_sample else 0, hw if region[1] > 1 else 0, C.byref(got), st),
                       "lpips_layer_weighted")
            return got.value, 1.0
        _lib.check(L.mgf_lpips_layer_defer_f32(scratch.data_ptr(), _lib.ptr(stats), *maps, n, c, hw, c * hw if per_sample else 0, C.byref(got), st),
                   "lpips_layer")
        return got.value, 1.0 / float(hw)

    def distance_into(self, out, pred, keep_taps=False):
        """out[i] = sum over taps of the spatial-mean weighted distance between pred[i] and the cached (single) target.
        pred: [n,3,H,W]; out: float32 [n].  keep_taps=True takes the un-fused path so that every tap stays in the workspace
        for `grad_into`."""
        f, taps, per_sample, region, _ = self._forward_taps(pred, bool(keep_taps), out)
        n = pred.shape[0]
        L, st = _lib.lib(), _lib.stream_ptr()
        # every tap leaves its partial sums in a scratch set of its own; ONE finish launch adds them to `out` in tap order (the same sums
        # in the same order as a finish per tap: the value is a by-product nothing waits for)
        red = int(L.mgf_reduce_scratch_floats())
        ntaps = len(self.lins)
        if self._scratch.numel() < ntaps * n * red:
            self._scratch = torch.empty(ntaps * n * red, dtype=torch.float32, device=self.device_)
        nparts, scales, k, first_done = (C.c_int32 * 8)(), (C.c_float * 8)(), 0, False
        for i, a in enumerate(taps):
            if a is None:
                first_done = True                   # tap 0 was consumed inside the stem kernel, which wrote out itself
                continue
            hw = a.shape[2] * a.shape[3]
            stats = None
            if keep_taps and backbones.TAP_STATS:
                key = (i, n, hw)
                stats = self._stats.get(key)
                if stats is None:
                    stats = self._stats[key] = torch.empty(n, 3, hw, dtype=torch.float32, device=self.device_)
                f.tap_stats[i] = stats
            nparts[k], scales[k] = self._defer_tap(i, a, self._scratch[k * n * red:], stats, per_sample, region)
            k += 1
        _lib.check(L.mgf_lpips_finish_taps_f32(out.data_ptr(), self._scratch.data_ptr(), n * red, k, nparts, scales, n, int(first_done), st),
                   "lpips_finish_taps")
        return out

    def distance_per_tap(self, pred):
        """[taps, n]: every tap's own contribution to `distance_into`'s sum -- PNetLin.forward(retPerLayer=True)'s `res` list
        (networks_basic.py:85-92) -- through the SAME kernel dispatch as distance_into (fused stem included), each tap written to its
        own row instead of accumulated."""
        f, taps, per_sample, region, out = self._forward_taps(pred, None)
        n = pred.shape[0]
        L, st = _lib.lib(), _lib.stream_ptr()
        for i, (a, b, lin) in enumerate(zip(taps, self._target_taps, self.lins)):
            if a is None:
                continue
            _, c, hh, ww = a.shape
            if region is not None:
                nparts, scale = self._defer_tap(i, a, self._scratch, None, per_sample, region)
                _lib.check(L.mgf_lpips_finish_taps_f32(out[i].data_ptr(), self._scratch.data_ptr(), n * int(L.mgf_reduce_scratch_floats()), 1,
                                                       (C.c_int32 * 8)(nparts), (C.c_float * 8)(scale), n, 0, st), "lpips_finish_taps")
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
            sides = []
            for l, (_, hh, ww) in enumerate(f.tap_shapes):
                got = spatial_tap_output_side(hh, H)
                if hh != ww or got != H:
                    raise _lib.MgfError(f"PerceptualLoss(spatial=True, net={self.net!r}): tap {l} ({hh}x{ww}) up-samples to side {got}, not to the "
                                        f"image's {H} (the reference's own sum of the tap maps fails at this size)")
                sides.append(hh)
            ws = self._map_ws[(n, H)] = [torch.empty(n, s, s, dtype=torch.float32, device=self.device_) for s in sides]
        return ws

    def _upsample_sum(self, out, maps, accumulate=False):
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
        if self.pair_offset is not None:
            raise _lib.MgfError("distance_map_into: a target pair is set (set_target_pair); the map is defined against one target")
        assert tuple(out.shape) == (n, 1, H, H) and out.dtype == torch.float32 and out.is_contiguous(), "out: contiguous float32 [n,1,H,H]"
        maps = self._map_workspace(n, H, self._features(n, H, W))
        _, taps, per_sample, _, _ = self._forward_taps(pred.float(), False, scalar=False)
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
