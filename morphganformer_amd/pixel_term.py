"""The pixel term of both projection loops: which entry points score it, which descend it, and the buffers they need.  The engines of
projection.py hold one `PixelTerm` and call it; what each term computes is written at ProjectionArgs.pixel_term."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)       # Wang, Simoncelli, Bovik 2003, finest level first


def msssim_weights(levels):
    """The level weights of pixel_term="msssim": the first `levels` of the paper's five, renormalised to sum 1 (one level: plain Gaussian SSIM)."""
    if not (isinstance(levels, int) and 1 <= levels <= len(MSSSIM_WEIGHTS)):
        raise _lib.MgfError(f"projection: msssim_levels must be an integer in 1..{len(MSSSIM_WEIGHTS)} (got {levels!r})")
    w = np.asarray(MSSSIM_WEIGHTS[:levels], dtype=np.float64)
    return (w / w.sum()).tolist()


def msssim_max_levels(h, w):
    """How many MS-SSIM levels an h x w image allows (every level's sides >= 11; a side s becomes (s + 1) // 2), at most 5."""
    n = 0
    while n < len(MSSSIM_WEIGHTS) and min(h, w) >= 11:
        n, h, w = n + 1, (h + 1) // 2, (w + 1) // 2
    return n


class PixelTerm:
    """The pixel term for `n` images per call of `shape` = [targets, C, H, W], the size the image-space losses see.  kind: args.pixel_term, or
    None without a pixel term (use_mse=False).  window: DSSIM or MS-SSIM, whose gradient kernels write the value too.  region_weighted: built
    with a region weight (set_region_weight fills it).  full_res: the generator's resolution, which the LBP distance scores (never pooled)."""

    def __init__(self, args, use_mse, shape, n, device, region_weighted=False, full_res=None):
        a, L = args, _lib.lib()
        assert a.pixel_term in ("mse", "psnr", "dssim", "lbp", "msssim"), a.pixel_term
        assert a.psnr_layout in ("script", "aligned"), a.psnr_layout
        self.args, self.device, self.shape = a, device, tuple(shape)
        self.kind = a.pixel_term if (use_mse or a.pixel_term == "lbp") else None
        self.window = self.kind in ("dssim", "msssim")
        self.region_weighted, self.pix_w = bool(region_weighted), None
        self.pair = self.pair_offset = self.script_target = None
        c, h, w = self.shape[1:]
        if self.kind in ("mse", "psnr"):
            self.scratch = torch.empty(n * int(L.mgf_reduce_scratch_floats()), dtype=torch.float32, device=device)
        if self.kind == "psnr" and a.psnr_layout == "script":
            # the script's element order: the target's H-W-C stream under the candidate's C-H-W indexing (a permuted copy, see refresh_target)
            self.script_target = torch.empty(self.shape, dtype=torch.float32, device=device)
        if self.kind == "lbp":
            from . import lbp
            self.lbp_ws = lbp.LbpWorkspace(n, full_res, full_res, device)
            self.lbp_codes = torch.empty(lbp.SIDE * lbp.SIDE, dtype=torch.uint8, device=device)
        if self.kind == "dssim":
            nbytes = int(L.mgf_dssim_scratch_bytes(n, c, h, w))
            if nbytes <= 0:
                raise _lib.MgfError(f"projection: pixel_term='dssim' needs images of at least 7x7 pixels, got {h}x{w}")
            self.win_scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
        if self.kind == "msssim":
            # the level weights as the float64 host array the entry points read at call time; the scratch holds the float64 pyramids
            weights = msssim_weights(a.msssim_levels)
            if msssim_max_levels(h, w) < a.msssim_levels:
                raise _lib.MgfError(f"projection: pixel_term='msssim' with msssim_levels={a.msssim_levels} needs every level's sides to be at least 11 "
                                    f"pixels; a {h}x{w} image allows {msssim_max_levels(h, w)} level(s)")
            self.msssim_w = (ctypes.c_double * len(weights))(*weights)
            self.msssim_w_ptr = ctypes.addressof(self.msssim_w)
            nbytes = int(L.mgf_msssim_scratch_bytes(n, c, h, w, a.msssim_levels))
            assert nbytes > 0, (n, c, h, w, a.msssim_levels)
            self.win_scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
        if self.region_weighted:
            if a.pixel_term != "mse":
                raise _lib.MgfError(f"projection: pixel_term={a.pixel_term!r} does not take a region_weight: the weighted window forms (DSSIM's 7x7 "
                                    "windows, MS-SSIM's Gaussian windows, the PSNR script's element order, the LBP histogram) are not built; "
                                    "use pixel_term='mse'")
            if int(a.latent_copies) > 1:
                raise _lib.MgfError("projection: latent_copies > 1 (the v2 driver's averaged latent) does not take a region_weight")

    # ------------------------------------------------------------------ what retarget() rewrites
    def set_region_weight(self, region_weight):
        """Write W / (C sum W), what the weighted kernels multiply by, into pix_w [nw, H W] (in place: captured graphs read it); returns the
        checked maps [nw, H, W] for the LPIPS module."""
        from .lpips import check_region_weight
        if not self.region_weighted:
            raise _lib.MgfError("retarget: this engine was built without a region_weight (its launch sequence holds the un-weighted kernels); "
                                "build a fresh one")
        w = check_region_weight(region_weight, "region_weight")
        nt, C, H, W = self.shape
        if tuple(w.shape[1:]) != (H, W):
            raise ValueError(f"region_weight is {tuple(w.shape[1:])}, the image-space losses see {(H, W)}")
        if w.shape[0] not in (1, nt):
            raise ValueError(f"{w.shape[0]} region weights for {nt} target(s): pass one map, or one per target")
        pix = (w / (C * w.sum(dim=(1, 2), keepdim=True))).to(torch.float32).reshape(w.shape[0], H * W)
        if self.pix_w is None:
            self.pix_w = pix.to(self.device).contiguous()
        elif tuple(self.pix_w.shape) != tuple(pix.shape):
            raise ValueError(f"retarget: {w.shape[0]} region weight map(s) where the engine was built with {self.pix_w.shape[0]}")
        else:
            self.pix_w.copy_(pix)
        return w

    def refresh_target(self, target, lbp_target=None):
        """The copies of the target this term keeps: the PSNR script-order stream (`tensor2np(imgs).flatten()`, 1024_example_PSNR.py:122,153,158)
        and the LBP code map of the target FILE, which the caller hands over."""
        if self.script_target is not None:
            self.script_target.copy_(target.permute(0, 2, 3, 1).contiguous().view(target.shape))
        if self.kind == "lbp":
            assert lbp_target is not None, "this engine scores the LBP distance: pass the new target's code map (lbp.target_feature)"
            codes = torch.as_tensor(lbp_target, dtype=torch.uint8).reshape(-1)
            assert codes.numel() == self.lbp_codes.numel(), "lbp_target: the 224 x 224 code map of lbp.target_feature"
            self.lbp_codes.copy_(codes)

    def set_pair(self, ta, tb, alpha):
        """A target pair, alpha [B] float64 on the host.  The MSE runs against the blended target and differs from the pair objective by the
        constant alpha (1 - alpha) P(Ta, Tb), computed here once; the window terms are not quadratic: both targets, every step (grad_into)."""
        B = len(alpha)
        self.pair = (ta, tb, alpha)
        if self.kind == "mse":
            self.pair_offset = torch.zeros(B, dtype=torch.float32, device=self.device)
            self._quadratic_into(self.pair_offset, ta, tb, B, ta.numel() // B)
            self.pair_offset.mul_(torch.as_tensor(alpha * (1.0 - alpha), dtype=torch.float32, device=self.device))
        elif self.window:
            self.pair_vals = torch.zeros(2, B, dtype=torch.float32, device=self.device)
            self.pair_w = torch.as_tensor(np.stack([1.0 - alpha, alpha]), dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ launches
    def _quadratic_into(self, out, img, target, n, tstride):
        L, st = _lib.lib(), _lib.stream_ptr()
        if self.pix_w is not None:
            c, hw = img.shape[1], img.shape[2] * img.shape[3]
            _lib.check(L.mgf_mse_weighted_f32(out.data_ptr(), img.data_ptr(), target.data_ptr(), self.pix_w.data_ptr(), n, c, hw, tstride,
                                              hw if self.pix_w.shape[0] > 1 else 0, 1.0, 0, self.scratch.data_ptr(), st), "mse_weighted")
        else:
            _lib.check(L.mgf_mse_f32(out.data_ptr(), img.data_ptr(), target.data_ptr(), n, img.numel() // n, tstride, 1.0, 0,
                                     self.scratch.data_ptr(), st), "mse")

    def value_into(self, out, img, target, n, tstride):
        """out[n] = the term as the literal loop scores it (DSSIM on the uint8 images); image j reads the target at j * tstride.  Nothing
        without a pixel term, and nothing for "lbp", which rides in the float64 slot (lbp_into)."""
        L, st, a = _lib.lib(), _lib.stream_ptr(), self.args
        c, h, w = img.shape[1:]
        if self.kind == "dssim":
            _lib.check(L.mgf_dssim_u8_f32(out.data_ptr(), img.data_ptr(), target.data_ptr(), n, c, h, w, tstride, 255.0, 1.0, 0,
                                          self.win_scratch.data_ptr(), st), "dssim")
        elif self.kind == "msssim":         # the continuous form; candidates that share a target share its pyramid
            _lib.check(L.mgf_msssim_f32(out.data_ptr(), img.data_ptr(), target.data_ptr(), n, c, h, w, tstride, self.msssim_w_ptr,
                                        a.msssim_levels, 255.0, 1.0, 0, self.win_scratch.data_ptr(), st), "msssim")
        elif self.kind in ("mse", "psnr"):
            self._quadratic_into(out, img, target if self.script_target is None else self.script_target, n, tstride)
            if self.kind == "psnr":
                # 10 * np.log10(peak ** 2 / np.mean(d ** 2)) with peak = 255., in float32 like the script's numpy (1024_example_PSNR.py:113-114)
                out.reciprocal_().mul_(65025.0).log10_().mul_(10.0)

    def lbp_into(self, out, full_img):
        """out[n] (float64) = the LBP matching distance of the images as generated (the script compares float64 distances, :166-172)."""
        self.lbp_ws.distance_into(out, full_img, self.lbp_codes)

    def _window_grad(self, dimg, out, img, tgt, n, tstride, scale, accumulate):
        L, st, a = _lib.lib(), _lib.stream_ptr(), self.args
        c, h, w = img.shape[-3:]
        if self.kind == "msssim":
            _lib.check(L.mgf_msssim_grad_f32(dimg.data_ptr(), out.data_ptr(), img.data_ptr(), tgt.data_ptr(), n, c, h, w, tstride, self.msssim_w_ptr,
                                             a.msssim_levels, 255.0, scale, accumulate, 0, self.win_scratch.data_ptr(), st), "msssim_grad")
        else:
            _lib.check(L.mgf_dssim_grad_f32(dimg.data_ptr(), out.data_ptr(), img.data_ptr(), tgt.data_ptr(), n, c, h, w, tstride, 255.0, scale,
                                            accumulate, 0, self.win_scratch.data_ptr(), st), "dssim_grad")

    def grad_into(self, dimg, out, img, target, n, tstride, scale, accumulate):
        """dimg (+)= scale * d term / d img (zero without a pixel term).  The window terms (their continuous forms) also write the unscaled
        value into out[n]; the MSE value is a launch of its own (value_after_grad_into)."""
        L, st = _lib.lib(), _lib.stream_ptr()
        if self.window and self.pair is not None:
            # both targets, sample by sample (the weight is the sample's own), gradients accumulated
            ta, tb, alpha = self.pair
            for t, tgt in enumerate((ta, tb)):
                for j in range(n):
                    wt = float(alpha[j]) if t else 1.0 - float(alpha[j])
                    self._window_grad(dimg[j:], self.pair_vals[t, j:], img[j:], tgt[j:], 1, 0, scale * wt, t)
            torch.sum(self.pair_vals * self.pair_w, 0, out=out)
        elif self.window:
            self._window_grad(dimg, out, img, target, n, tstride, scale, accumulate)
        elif self.kind == "mse" and self.pix_w is not None:
            c, hw = img.shape[1], img.shape[2] * img.shape[3]
            _lib.check(L.mgf_mse_weighted_grad_f32(dimg.data_ptr(), img.data_ptr(), target.data_ptr(), self.pix_w.data_ptr(), n, c, hw, tstride,
                                                   hw if self.pix_w.shape[0] > 1 else 0, scale, accumulate, st), "mse_weighted_grad")
        elif self.kind == "mse":
            _lib.check(L.mgf_mse_grad_f32(dimg.data_ptr(), img.data_ptr(), target.data_ptr(), n, img.numel() // n, tstride, scale, accumulate,
                                          st), "mse_grad")
        elif not accumulate:
            dimg.zero_()

    def value_after_grad_into(self, out, img, target, n, tstride):
        """The value where grad_into has not written it: the MSE, plus a target pair's constant (gradient mode, after the other terms)."""
        if self.kind == "mse":
            self._quadratic_into(out, img, target, n, tstride)
            if self.pair_offset is not None:
                out.add_(self.pair_offset)
