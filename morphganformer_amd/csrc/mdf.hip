// The MDF (multi-scale discriminative feature) objective: SinGAN WDiscriminators as loss networks (SinGAN/models.py:7-35,
// mdfloss.py:16-47).  Each discriminator is five VALID (padding 0) 3x3 / stride-1 convolutions -- head 3 -> N, three body blocks
// N -> N, tail N -> 1 -- with eval-mode BatchNorm folded into the weights on the host and LeakyReLU(0.2) behind every layer but the
// tail; the loss sums, per candidate, mean((D(x)_t - D(y)_t)^2) over the three taps x1 (head out), x2 (body out), x3 (tail out).
//
// Frames.  Every map of one discriminator lives in an h x w FRAME of the input image's size; a map of ring depth r holds its valid
// values at rows / columns [r, h - r) of the frame (the image: r = 0, x1: 1, after body block k: 1 + k, x3: 5).  A valid 3x3
// convolution of a ring-r map is then the frame's pad-1 convolution read on ring r + 1: an output at p reads p - 1 .. p + 1, inside
// ring r.  The body blocks run as such pad-1 launches of the form-3 Winograd kernel (wino3.hip, even 1024^2 frames, 32 / 64 / 128
// channels) over the whole frame: the valid outputs are exact valid convolutions up to float32 rounding, the ring outside them holds
// finite values of the same magnitude that nothing compares (a Winograd tile that straddles the ring boundary mixes them into its
// transform, which is why the head writes the whole frame -- zero-padded -- rather than leaving its ring unset).  The frames cost
// (h^2 - (h - 2r)^2) / h^2 extra work: 0.4-1.6 % at 1024^2.
//
// Partial sums.  The head and the tail reduce their squared differences per workgroup (64 x 4 frame pixels) in a fixed order into
// one float64 per (candidate, workgroup): slabs part[slot][candidate][workgroup], slot = 3 * (discriminator position) + tap.  The
// finish kernel adds the slabs of a candidate in index order, divides each tap's sum by its element count and sums the taps in the
// reference's order.  No atomics anywhere, and a candidate's workgroups do not depend on the batch: its loss is the same bits in any
// batch.
// Contracts: include/mgf.h (mgf_mdf_*).
#include <algorithm>

#include "mgf_common.h"

namespace {

constexpr int MDF_BX = 64, MDF_BY = 4;           // frame pixels per workgroup (one per lane)
constexpr int MDF_MAX_C = 128;                    // discriminator width N
constexpr int MDF_MAX_SLOTS = 27;                 // 9 discriminators x 3 taps
typedef const float __attribute__((address_space(4)))* mdf_cfp;   // weights through the scalar cache: every lane reads the same value

// the workgroup's 64 x 4 lanes as the thread index 0..255 of mgf_block_tree_sum_256 (mgf_common.h)
static_assert(MDF_BX * MDF_BY == 256, "mgf_block_tree_sum_256");
__device__ __forceinline__ int mdf_lane() { return (int)(threadIdx.y * MDF_BX + threadIdx.x); }

// x1[n, co] = lrelu(b[co] + sum_{ci,kh,kw} w[co, ci, kh, kw] img[n, ci, y + kh - 1, x + kw - 1]) on the whole frame (zero padding);
// part[n][blk] = sum over the ring-1 pixels of the workgroup and the channels of (x1 - x1_target)^2
__global__ __launch_bounds__(256) void mdf_head_kernel(float* __restrict__ x1, double* __restrict__ part, const float* __restrict__ img,
                                                       const float* w, const float* bias, const float* __restrict__ x1t, int c, int h,
                                                       int wd, float slope) {
    __shared__ double red[MDF_BX * MDF_BY];
    const int x = blockIdx.x * MDF_BX + threadIdx.x, y = blockIdx.y * MDF_BY + threadIdx.y, n = blockIdx.z;
    const bool in = x < wd && y < h;
    const int64_t plane = (int64_t)h * wd;
    float v[27];
    const float* ib = img + (int64_t)n * 3 * plane;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        const int yy = y + (k % 9) / 3 - 1, xx = x + k % 3 - 1;
        v[k] = (in && yy >= 0 && yy < h && xx >= 0 && xx < wd) ? ib[(k / 9) * plane + (int64_t)yy * wd + xx] : 0.f;
    }
    const bool inner = in && y >= 1 && y < h - 1 && x >= 1 && x < wd - 1;
    const mdf_cfp ws = (mdf_cfp)w, bs = (mdf_cfp)bias;
    float* yb = x1 + (int64_t)n * c * plane + (int64_t)y * wd + x;
    const float* tb = x1t ? x1t + (int64_t)y * wd + x : nullptr;
    double acc = 0.0;
    for (int co = 0; co < c; ++co) {
        const mdf_cfp wr = ws + co * 27;
        float a = bs[co];
#pragma unroll
        for (int k = 0; k < 27; ++k) a = fmaf(wr[k], v[k], a);
        a = a > 0.f ? a : a * slope;                          // LeakyReLU: x if x > 0 else slope x (torch)
        if (in) yb[co * plane] = a;
        if (tb && inner) {
            const double d = (double)a - (double)tb[co * plane];
            acc += d * d;
        }
    }
    if (part) {
        const double s = mgf_block_tree_sum_256(acc, red, mdf_lane());
        if (threadIdx.x == 0 && threadIdx.y == 0) part[(int64_t)n * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// x2: ring-r frames [n, c, h, w].  On ring r: part2 += sum_c (x2 - x2_target)^2.  On ring r + 1: x3 = b + sum_{c,kh,kw} w[c, kh, kw]
// x2[c, y + kh - 1, x + kw - 1] (the tail conv N -> 1, no activation), written to x3 if given, part3 += (x3 - x3_target)^2.
__global__ __launch_bounds__(256) void mdf_tail_kernel(float* __restrict__ x3, double* __restrict__ part2, double* __restrict__ part3,
                                                       const float* __restrict__ x2, const float* w, float bias,
                                                       const float* __restrict__ x2t, const float* __restrict__ x3t, int c, int h, int wd,
                                                       int r) {
    __shared__ double red[MDF_BX * MDF_BY];
    const int x = blockIdx.x * MDF_BX + threadIdx.x, y = blockIdx.y * MDF_BY + threadIdx.y, n = blockIdx.z;
    const bool v2 = x >= r && x < wd - r && y >= r && y < h - r;
    const bool v3 = x >= r + 1 && x < wd - r - 1 && y >= r + 1 && y < h - r - 1;
    const int64_t plane = (int64_t)h * wd, pix = (int64_t)y * wd + x;
    const float* xb = x2 + (int64_t)n * c * plane + pix;
    const mdf_cfp ws = (mdf_cfp)w;
    double s2 = 0.0, s3 = 0.0;
    float a = bias;
    if (v2) {
        for (int ci = 0; ci < c; ++ci) {
            const float* xc = xb + ci * plane;
            if (x2t) {
                const double d = (double)xc[0] - (double)x2t[ci * plane + pix];
                s2 += d * d;
            }
            if (v3) {
                const mdf_cfp wr = ws + ci * 9;
#pragma unroll
                for (int k = 0; k < 9; ++k) a = fmaf(wr[k], xc[(k / 3 - 1) * wd + (k % 3 - 1)], a);
            }
        }
    }
    if (v3) {
        if (x3) x3[(int64_t)n * plane + pix] = a;
        if (x3t) {
            const double d = (double)a - (double)x3t[pix];
            s3 = d * d;
        }
    }
    const int64_t slot = (int64_t)n * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x;
    if (part2) {
        const double s = mgf_block_tree_sum_256(s2, red, mdf_lane());
        if (threadIdx.x == 0 && threadIdx.y == 0) part2[slot] = s;
    }
    if (part3) {
        const double s = mgf_block_tree_sum_256(s3, red, mdf_lane());
        if (threadIdx.x == 0 && threadIdx.y == 0) part3[slot] = s;
    }
}

struct MdfFinishArgs {
    double count[MDF_MAX_SLOTS];      // elements of each slot's tap
};

// grid = n, 256 lanes: out[b] = (accumulate ? out[b] : 0) + float(scale * sum_slot (sum_k part[slot][b][k]) / count[slot])
__global__ __launch_bounds__(256) void mdf_finish_kernel(float* out, const double* __restrict__ part, int nslots, int64_t nblk, int n,
                                                         MdfFinishArgs args, float scale, int accumulate) {
    __shared__ double red[256];
    const int t = threadIdx.x, b = blockIdx.x;
    double loss = 0.0;
    for (int s = 0; s < nslots; ++s) {
        const double* p = part + ((int64_t)s * n + b) * nblk;
        double v = 0.0;
        for (int64_t k = t; k < nblk; k += 256) v += p[k];
        loss += mgf_block_tree_sum_256(v, red) / args.count[s];      // mean over the tap, taps in the reference's order (mdfloss.py:34-43)
    }
    if (t == 0) {
        const float v = (float)((double)scale * loss);
        out[b] = accumulate ? out[b] + v : v;
    }
}


// ---- backward (dimg (+)= s * d loss / d img).  Frames as in the forward; phi'(a) = a > 0 ? 1 : slope of the stored POST-activation (torch's
// in-place LeakyReLU backward).  Every gradient frame is written whole, 0 outside its ring: the adjoint Winograd launches read it zero-padded.

// d3 [n,c,h,w] = (sum_{kh,kw} w[c,kh,kw] g3[y - kh + 1, x - kw + 1] + coef2 (x2 - x2_target)) * phi'(x2) on ring r, 0 elsewhere, with
// g3 = coef3 (x3 - x3_target) on ring r + 1 and 0 elsewhere, formed on the fly from x3 (no g3 buffer)
__global__ __launch_bounds__(256) void mdf_tail_bwd_kernel(float* __restrict__ d3, const float* __restrict__ x2, const float* __restrict__ x2t,
                                                           const float* __restrict__ x3, const float* __restrict__ x3t, const float* w,
                                                           int c, int h, int wd, int r, float coef2, float coef3, float slope) {
    const int x = blockIdx.x * MDF_BX + threadIdx.x, y = blockIdx.y * MDF_BY + threadIdx.y, n = blockIdx.z;
    if (x >= wd || y >= h) return;
    const bool v2 = x >= r && x < wd - r && y >= r && y < h - r;
    const int64_t plane = (int64_t)h * wd, pix = (int64_t)y * wd + x;
    float* db = d3 + (int64_t)n * c * plane + pix;
    if (!v2) {
        for (int ci = 0; ci < c; ++ci) db[ci * plane] = 0.f;
        return;
    }
    float g[9];                                           // g[k]: g3 at (y - kh + 1, x - kw + 1), k = 3 kh + kw
    const float* x3b = x3 + (int64_t)n * plane;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = y - k / 3 + 1, xx = x - k % 3 + 1;
        const bool v3 = xx >= r + 1 && xx < wd - r - 1 && yy >= r + 1 && yy < h - r - 1;
        const int64_t q = (int64_t)yy * wd + xx;
        g[k] = v3 ? coef3 * (x3b[q] - x3t[q]) : 0.f;
    }
    const float* xb = x2 + (int64_t)n * c * plane + pix;
    const mdf_cfp ws = (mdf_cfp)w;
    for (int ci = 0; ci < c; ++ci) {
        const mdf_cfp wr = ws + ci * 9;
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) a = fmaf(wr[k], g[k], a);
        const float xv = xb[ci * plane];
        a = fmaf(coef2, xv - x2t[ci * plane + pix], a);
        db[ci * plane] = xv > 0.f ? a : a * slope;
    }
}

// dimg [n,3,h,w] (+)= sum_{co,kh,kw} w[co,ci,kh,kw] d0[co, y - kh + 1, x - kw + 1] on the whole frame (the head's adjoint: pad 1), with
// d0 = d0m + coef1 (x1 - x1_target) phi'(x1) on ring 1 and 0 elsewhere -- d0m is the masked adjoint of the first body block, the tap-0
// term joins here
__global__ __launch_bounds__(256) void mdf_head_bwd_kernel(float* __restrict__ dimg, const float* __restrict__ d0m, const float* __restrict__ x1,
                                                           const float* __restrict__ x1t, const float* w, int c, int h, int wd, float coef1,
                                                           float slope, int accumulate) {
    const int x = blockIdx.x * MDF_BX + threadIdx.x, y = blockIdx.y * MDF_BY + threadIdx.y, n = blockIdx.z;
    if (x >= wd || y >= h) return;
    const int64_t plane = (int64_t)h * wd;
    int64_t off[9];
    bool ok[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = y - k / 3 + 1, xx = x - k % 3 + 1;
        ok[k] = xx >= 1 && xx < wd - 1 && yy >= 1 && yy < h - 1;
        off[k] = ok[k] ? (int64_t)yy * wd + xx : 0;
    }
    const float* db = d0m + (int64_t)n * c * plane;
    const float* xb = x1 + (int64_t)n * c * plane;
    const mdf_cfp ws = (mdf_cfp)w;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int co = 0; co < c; ++co) {
        const int64_t cp = co * plane;
        const mdf_cfp wr = ws + co * 27;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            float d = 0.f;
            if (ok[k]) {
                const float xv = xb[cp + off[k]], t = coef1 * (xv - x1t[cp + off[k]]);
                d = db[cp + off[k]] + (xv > 0.f ? t : t * slope);
            }
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) acc[ci] = fmaf(wr[ci * 9 + k], d, acc[ci]);
        }
    }
    float* ob = dimg + (int64_t)n * 3 * plane + (int64_t)y * wd + x;
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) ob[ci * plane] = accumulate ? ob[ci * plane] + acc[ci] : acc[ci];
}

}  // namespace

extern "C" int64_t mgf_mdf_partials(int32_t h, int32_t w) {
    if (h < 1 || w < 1) return 0;
    return mgf_cdiv(w, MDF_BX) * mgf_cdiv(h, MDF_BY);
}

extern "C" int mgf_mdf_head_f32(float* x1, double* part, const float* img, const float* w, const float* bias, const float* x1_target,
                                int32_t n, int32_t c, int32_t h, int32_t wd, float slope, mgf_stream_t stream) {
    MGF_REQUIRE(x1 && img && w && bias && n >= 1 && n <= 65535 && h >= 3 && wd >= 3 && h <= 65535 * MDF_BY, MGF_EINVAL, "mdf_head: bad arguments");
    MGF_REQUIRE(c >= 1 && c <= MDF_MAX_C, MGF_EUNSUPPORTED, "mdf_head: 1 .. %d output channels (got %d)", MDF_MAX_C, c);
    MGF_REQUIRE(!x1_target == !part, MGF_EINVAL, "mdf_head: the target tap and the partial sums come together");
    const dim3 grid((unsigned)mgf_cdiv(wd, MDF_BX), (unsigned)mgf_cdiv(h, MDF_BY), (unsigned)n), blk(MDF_BX, MDF_BY);
    mgf_prof_external_begin((hipStream_t)stream, "mdf_head_kernel", 2.0 * 27 * c * (double)h * wd * n,
                            4.0 * (double)n * h * wd * (3 + c + (x1_target ? c : 0)));
    hipLaunchKernelGGL(mdf_head_kernel, grid, blk, 0, (hipStream_t)stream, x1, part, img, w, bias, x1_target, c, h, wd, slope);
    mgf_prof_external_end((hipStream_t)stream);
    MGF_CHECK_LAUNCH("mdf_head");
    return MGF_OK;
}

extern "C" int mgf_mdf_body_f32(float* y, const float* x, const float* u, const float* bias, int32_t n, int32_t c, int32_t h, int32_t wd,
                                float slope, mgf_stream_t stream) {
    MGF_REQUIRE(y && x && u && bias && n >= 1 && h >= 3 && wd >= 3, MGF_EINVAL, "mdf_body: bad arguments");
    MGF_REQUIRE(c == 32 || c == 64 || c == 128, MGF_EUNSUPPORTED, "mdf_body: 32, 64 or 128 channels (got %d)", c);
    mgf_epilogue ep{};
    ep.bias = bias;
    ep.act = MGF_ACT_LRELU;
    ep.alpha = slope;
    ep.gain = 1.f;
    return mgf_wino3_batch_invariant_f32(y, x, u, n, c, h, wd, c, &ep, stream);
}

extern "C" int mgf_mdf_tail_f32(float* x3, double* part2, double* part3, const float* x2, const float* w, float bias, const float* x2_target,
                                const float* x3_target, int32_t n, int32_t c, int32_t h, int32_t wd, int32_t ring, mgf_stream_t stream) {
    MGF_REQUIRE(x2 && w && n >= 1 && n <= 65535 && ring >= 0 && h - 2 * ring >= 3 && wd - 2 * ring >= 3 && h <= 65535 * MDF_BY, MGF_EINVAL,
                "mdf_tail: bad arguments");
    MGF_REQUIRE(c >= 1 && c <= MDF_MAX_C, MGF_EUNSUPPORTED, "mdf_tail: 1 .. %d input channels (got %d)", MDF_MAX_C, c);
    MGF_REQUIRE(!x2_target == !part2 && !x3_target == !part3, MGF_EINVAL, "mdf_tail: each target tap comes with its partial sums");
    MGF_REQUIRE(x3 || part2 || part3, MGF_EINVAL, "mdf_tail: nothing to compute");
    const dim3 grid((unsigned)mgf_cdiv(wd, MDF_BX), (unsigned)mgf_cdiv(h, MDF_BY), (unsigned)n), blk(MDF_BX, MDF_BY);
    mgf_prof_external_begin((hipStream_t)stream, "mdf_tail_kernel", 2.0 * 9 * c * (double)h * wd * n,
                            4.0 * (double)n * h * wd * (c + (x2_target ? c : 0) + 1));
    hipLaunchKernelGGL(mdf_tail_kernel, grid, blk, 0, (hipStream_t)stream, x3, part2, part3, x2, w, bias, x2_target, x3_target, c, h, wd, ring);
    mgf_prof_external_end((hipStream_t)stream);
    MGF_CHECK_LAUNCH("mdf_tail");
    return MGF_OK;
}

extern "C" int mgf_mdf_finish_f32(float* out, const double* part, int32_t nslots, int64_t nblk, const double* counts, int32_t n, float scale,
                                  int32_t accumulate, mgf_stream_t stream) {
    MGF_REQUIRE(out && part && counts && n >= 1 && nblk >= 1, MGF_EINVAL, "mdf_finish: bad arguments");
    MGF_REQUIRE(nslots >= 1 && nslots <= MDF_MAX_SLOTS, MGF_EUNSUPPORTED, "mdf_finish: 1 .. %d taps (got %d)", MDF_MAX_SLOTS, nslots);
    MdfFinishArgs a{};
    for (int s = 0; s < nslots; ++s) {
        MGF_REQUIRE(counts[s] > 0, MGF_EINVAL, "mdf_finish: tap %d has no elements", s);
        a.count[s] = counts[s];
    }
    hipLaunchKernelGGL(mdf_finish_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, out, part, nslots, nblk, n, a, scale, accumulate);
    MGF_CHECK_LAUNCH("mdf_finish");
    return MGF_OK;
}

extern "C" int mgf_mdf_tail_backward_f32(float* d3, const float* x2, const float* x2_target, const float* x3, const float* x3_target, const float* w,
                                         int32_t n, int32_t c, int32_t h, int32_t wd, int32_t ring, float coef2, float coef3, float slope,
                                         mgf_stream_t stream) {
    MGF_REQUIRE(d3 && x2 && x2_target && x3 && x3_target && w && n >= 1 && n <= 65535 && ring >= 0 && h - 2 * ring >= 3 && wd - 2 * ring >= 3 &&
                h <= 65535 * MDF_BY, MGF_EINVAL, "mdf_tail_backward: bad arguments");
    MGF_REQUIRE(c >= 1 && c <= MDF_MAX_C, MGF_EUNSUPPORTED, "mdf_tail_backward: 1 .. %d channels (got %d)", MDF_MAX_C, c);
    const dim3 grid((unsigned)mgf_cdiv(wd, MDF_BX), (unsigned)mgf_cdiv(h, MDF_BY), (unsigned)n), blk(MDF_BX, MDF_BY);
    mgf_prof_external_begin((hipStream_t)stream, "mdf_tail_bwd_kernel", 2.0 * 10 * c * (double)h * wd * n,
                            4.0 * (double)h * wd * (n * (2.0 * c + 1) + c + 1));
    hipLaunchKernelGGL(mdf_tail_bwd_kernel, grid, blk, 0, (hipStream_t)stream, d3, x2, x2_target, x3, x3_target, w, c, h, wd, ring, coef2, coef3, slope);
    mgf_prof_external_end((hipStream_t)stream);
    MGF_CHECK_LAUNCH("mdf_tail_backward");
    return MGF_OK;
}

extern "C" int mgf_mdf_body_backward_f32(float* d, const float* g, const float* u_adj, const float* a_prev, int32_t n, int32_t c, int32_t h,
                                         int32_t wd, int32_t ring, float slope, mgf_stream_t stream) {
    MGF_REQUIRE(d && g && u_adj && a_prev && n >= 1 && h >= 3 && wd >= 3 && ring >= 1, MGF_EINVAL, "mdf_body_backward: bad arguments");
    MGF_REQUIRE(c == 32 || c == 64 || c == 128, MGF_EUNSUPPORTED, "mdf_body_backward: 32, 64 or 128 channels (got %d)", c);
    return mgf_wino3_batch_invariant_masked_f32(d, g, u_adj, a_prev, n, c, h, wd, ring, slope, stream);
}

extern "C" int mgf_mdf_head_backward_f32(float* dimg, const float* d0, const float* x1, const float* x1_target, const float* w, int32_t n,
                                         int32_t c, int32_t h, int32_t wd, float coef1, float slope, int32_t accumulate, mgf_stream_t stream) {
    MGF_REQUIRE(dimg && d0 && x1 && x1_target && w && n >= 1 && n <= 65535 && h >= 3 && wd >= 3 && h <= 65535 * MDF_BY, MGF_EINVAL,
                "mdf_head_backward: bad arguments");
    MGF_REQUIRE(c >= 1 && c <= MDF_MAX_C, MGF_EUNSUPPORTED, "mdf_head_backward: 1 .. %d channels (got %d)", MDF_MAX_C, c);
    const dim3 grid((unsigned)mgf_cdiv(wd, MDF_BX), (unsigned)mgf_cdiv(h, MDF_BY), (unsigned)n), blk(MDF_BX, MDF_BY);
    mgf_prof_external_begin((hipStream_t)stream, "mdf_head_bwd_kernel", 2.0 * 27 * c * (double)h * wd * n,
                            4.0 * (double)h * wd * (n * (2.0 * c + 3 * (accumulate ? 2 : 1)) + c));
    hipLaunchKernelGGL(mdf_head_bwd_kernel, grid, blk, 0, (hipStream_t)stream, dimg, d0, x1, x1_target, w, c, h, wd, coef1, slope, accumulate);
    mgf_prof_external_end((hipStream_t)stream);
    MGF_CHECK_LAUNCH("mdf_head_backward");
    return MGF_OK;
}
