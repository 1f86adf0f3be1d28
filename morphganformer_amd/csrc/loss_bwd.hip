// Gradient mode, loss side: dLoss/dimage of the terms the synthesis network's pass (backward.hip) starts from -- what torch autograd does
// for the reference through the LPIPS taps (lpips/networks_basic.py:64-92), the backbones' ReLU layers (lpips/pretrained_networks.py) and
// torch.nn.MSELoss.  The convolutions' data gradients are the forward kernels on transposed taps and live with them, the max-pool gradients
// with the pools (maxpool.hip); here are the element-wise kernels:
//   mgf_lpips_layer_bwd*              one tap's gradient, alone or fused with the tap's ReLU backward, plain / from stored stats / weighted
//   mgf_relu_bwd_split_f32            ReLU backward into the two halves of a Fire concat
//   mgf_mse_grad_f32                  gradient of the per-sample mean squared error
// No reduction across lanes beyond a workgroup's own pixels: every output element is written by one lane, bit-reproducible.
// Contract: include/mgf.h ("Loss side of gradient mode").
#include "mgf_common.h"

namespace {

// LPIPS tap (networks_basic.py:70-87): l = (scale / hw) * sum_p sum_c lin[c] (f0[c] q - u1[c])^2 with q = 1 / (|f0| + 1e-10).
// One lane per pixel, two sweeps over the channels:  A = sum f0^2, B = sum lin f0^2, Cc = sum lin u1 f0  give
//   <du0, f0> = k (q B - Cc),   df0[c] = q k lin[c] (f0[c] q - u1[c]) - <du0, f0> q^2 / |f0| * f0[c],   k = 2 scale / hw.
// An all-zero pixel (|f0| = 0) gets a zero gradient (torch autograd yields NaN there: sqrt'(0) * 0).
// RELU: the tap is a ReLU output (all of them are) and the ReLU's backward rides along: dz = f0 > 0 ? din + df0 : 0 (din may be
// null), channels [0, c_split) to oa [n, c_split, hw], the rest to ob [n, c - c_split, hw] (mgf_relu_bwd_split_f32's layout); without
// RELU oa is df0 [n, c, hw] and `accumulate` adds to it.
// CPT > 0: c <= CPT * (256 / PXB), and the lane keeps its CPT channels of f0 and f1 in registers between the two sweeps: 629 -> 588 us
// at 8 x 64 x 511^2 with 16 channels per lane; with 32 (128 channels) the registers cost more residency than the second sweep's
// mostly cache-resident reads (321 -> 435 us), so only CPT = 16 is built.  Wider pixel blocks (128, 256) measured no faster than 64.
// WEIGHTED (region weights): l = scale * sum_p omega[p] sum_c ..., so k = 2 scale omega[p] per pixel -- the host passes 2 scale and every lane
// multiplies by its pixel's weight (one more buffer load); omega = 0 gives g = 0 exactly, i.e. din through the ReLU mask.
template <int PXB, bool RELU, int CPT, bool WEIGHTED = false>
__global__ __launch_bounds__(256) void lpips_layer_bwd_kernel(float* oa, float* ob, const float* din, const float* f0, const float* f1u,
                                                              const float* lin, int c, int c_split, int64_t hw, int64_t f1_bs, float k,
                                                              int accumulate, const float* stats, const float* wmap, int64_t w_bs) {
    // a workgroup owns PXB consecutive pixels; its G = 256 / PXB lane groups split the channels and meet in LDS
    constexpr int G = 256 / PXB;
    constexpr int NV = CPT > 0 ? CPT : 1;
    __shared__ float part[3][G][PXB];
    const int n = blockIdx.y, px = threadIdx.x % PXB, grp = threadIdx.x / PXB;
    const int64_t p = (int64_t)blockIdx.x * PXB + px;
    const bool valid = p < hw;
    const int64_t pc = valid ? p : hw - 1;
    // Buffer addressing (round 3, like the forward kernel): a thread's channels are G planes apart, so the channel part of every address is
    // a scalar offset (j G hw) on one per-lane offset (grp hw + pixel); the range check covers both, so a channel past c -- or past
    // c_split in the first output, before it in the second -- reads 0 / is not stored, without a per-lane test.  Host: c * hw * 4 < 2^32.
    const unsigned plane_b = 4u * (unsigned)hw;
    const unsigned vo = (unsigned)grp * plane_b + 4u * (unsigned)pc;
    const unsigned cbytes = (unsigned)c * plane_b;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)(f0 + (int64_t)n * c * hw), 0, (int)cbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(f1u + (int64_t)n * f1_bs), 0, (int)cbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc((void*)lin, 0, 4 * c, 0x00020000);
    auto ld = [&](const __amdgpu_buffer_rsrc_t& r, int j) {
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, vo, (int)((unsigned)(j * G) * plane_b), 0));
    };
    auto ldlin = [&](int j) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rl, 4u * (unsigned)grp, 4 * j * G, 0)); };
    const int nj = (c + G - 1) / G;                   // channel steps (a lane whose channel of the last step is past c reads zeros)
    if (WEIGHTED) {
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(wmap + (int64_t)n * w_bs), 0, (int)plane_b, 0x00020000);
        k *= __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rw, 4u * (unsigned)pc, 0, 0));
    }
    float va[NV], vb[NV];
    float A = 0.f, B = 0.f, Cc = 0.f;
    // stats: the per-pixel sums A, B, C of the forward (mgf_lpips_layer_stats_f32, [n][3][hw]) -- no first sweep, no meeting in LDS
    if (CPT == 0 && stats) {
        const float* sp = stats + (int64_t)n * 3 * hw + pc;
        A = sp[0]; B = sp[hw]; Cc = sp[2 * hw];
    } else {
    if (CPT > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) { va[j] = ld(ra, j); vb[j] = ld(rb, j); }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float l = ldlin(j);
            A += va[j] * va[j];
            B += l * va[j] * va[j];
            Cc += l * vb[j] * va[j];
        }
    } else {
#pragma unroll 4
        for (int j = 0; j < nj; ++j) {
            const float v = ld(ra, j), l = ldlin(j);
            A += v * v;
            B += l * v * v;
            Cc += l * ld(rb, j) * v;
        }
    }
    part[0][grp][px] = A; part[1][grp][px] = B; part[2][grp][px] = Cc;
    __syncthreads();
    A = B = Cc = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) { A += part[0][g][px]; B += part[1][g][px]; Cc += part[2][g][px]; }
    }
    const float nrm = sqrtf(A);
    const float q = 1.f / (nrm + 1e-10f);
    const float dot = k * (q * B - Cc);
    const float coef = nrm > 0.f ? dot * q * q / nrm : 0.f;
    // outputs: RELU -> channels [0, c_split) to oa, the rest to ob; else oa holds all c channels
    const unsigned vst = valid ? vo : 0xFFFFFFF0u;
    const int ca = RELU ? c_split : c;
    const __amdgpu_buffer_rsrc_t rda = __builtin_amdgcn_make_buffer_rsrc((void*)(oa + (int64_t)n * ca * hw), 0, (int)((unsigned)ca * plane_b), 0x00020000);
    const bool has_b = RELU && ob != nullptr && c > c_split;
    const __amdgpu_buffer_rsrc_t rdb = __builtin_amdgcn_make_buffer_rsrc((void*)(has_b ? ob + (int64_t)n * (c - c_split) * hw : oa), 0,
                                                                         has_b ? (int)((unsigned)(c - c_split) * plane_b) : 0, 0x00020000);
    const bool has_di = RELU && din != nullptr;
    const __amdgpu_buffer_rsrc_t rdi = __builtin_amdgcn_make_buffer_rsrc((void*)(has_di ? din + (int64_t)n * c * hw : f0), 0, has_di ? (int)cbytes : 0, 0x00020000);
    auto one = [&](int j, float v, float u) {
        const int so = (int)((unsigned)(j * G) * plane_b);
        float g = q * k * ldlin(j) * (v * q - u) - coef * v;
        if (RELU) {
            g = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rdi, vo, so, 0)) + g;       // (no din: zero-size descriptor, reads 0)
            g = v > 0.f ? g : 0.f;
            const int ch = grp + j * G, cb = j * G - c_split;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, g), rda, vst, so, 0);       // ch >= c_split: past rda's end
            // second output: channel ch - c_split.  With c_split a multiple of G the step's channel base j G - c_split is wave-uniform (a
            // negative one means this step lies in the first output); otherwise the whole offset is per lane.  (The range check adds
            // vector and scalar offset WITHOUT 32-bit wrap: an offset that "wraps back" into range is still out of range.)
            const bool even = c_split % G == 0;
            const unsigned vsb = !valid ? 0xFFFFFFF0u
                               : even ? (cb >= 0 ? vo : 0xFFFFFFF0u)
                                      : (ch >= c_split ? (unsigned)(ch - c_split) * plane_b + 4u * (unsigned)pc : 0xFFFFFFF0u);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, g), rdb, vsb, (even && cb >= 0) ? (int)((unsigned)cb * plane_b) : 0, 0);
        } else {
            if (accumulate) g += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rda, vo, so, 0));
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, g), rda, vst, so, 0);
        }
    };
    if (CPT > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) one(j, va[j], vb[j]);
    } else {
#pragma unroll 4
        for (int j = 0; j < nj; ++j) one(j, ld(ra, j), ld(rb, j));
    }
}

// dz = dy where y > 0 else 0, channels [0, cs) to dz_a [n, cs, hw] and [cs, c) to dz_b [n, c - cs, hw] (Fire concat halves)
__global__ __launch_bounds__(256) void relu_bwd_split_kernel(float* dz_a, float* dz_b, const float* dy, const float* y, int c, int cs,
                                                             int64_t hw, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t p = i % hw, r = i / hw;
        const int ch = (int)(r % c);
        const int64_t nn = r / c;
        const float v = y[i] > 0.f ? dy[i] : 0.f;
        if (ch < cs) dz_a[(nn * cs + ch) * hw + p] = v;
        else dz_b[(nn * (c - cs) + (ch - cs)) * hw + p] = v;
    }
}

// dimg (+)= scale * 2 (a - b) / numel    (gradient of scale * mean((a - b)^2) per sample)
__global__ __launch_bounds__(256) void mse_grad_kernel(float* d, const float* a, const float* b, int64_t numel, int64_t b_bs, float k,
                                                       int accumulate, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t nn = i / numel, p = i % numel;
        const float g = k * (a[i] - b[nn * b_bs + p]);
        d[i] = accumulate ? d[i] + g : g;
    }
}

}  // namespace

// Pixels per workgroup: 64 (256-byte row segments per channel) while that leaves >= 512 workgroups, else 32 while >= 256, else 16 -- the
// 16-pixel form moves 64-byte segments and streams at half the rate (1.7 vs 3.4 TB/s at 8 x 256 x 127^2).  MGF_LPIPS_BWD_PXB pins one,
// MGF_LPIPS_BWD_CACHE=0 turns the register-resident second sweep off (tuning).
template <bool RELU>
static void lpips_bwd_launch(float* oa, float* ob, const float* din, const float* f0, const float* f1u, const float* lin, int n, int c,
                             int c_split, int64_t hw, int64_t f1_bs, float k, int accumulate, hipStream_t st, const float* stats = nullptr,
                             const float* wmap = nullptr, int64_t w_bs = 0) {
    static const int env_pxb = [] { const char* e = mgf_knob("MGF_LPIPS_BWD_PXB"); return e ? atoi(e) : 0; }();
    int pxb = mgf_cdiv(hw, 64) * n >= 512 ? 64 : mgf_cdiv(hw, 32) * n >= 256 ? 32 : 16;
    if (env_pxb == 16 || env_pxb == 32 || env_pxb == 64) pxb = env_pxb;
    static const bool no_cache = [] { const char* e = mgf_knob("MGF_LPIPS_BWD_CACHE"); return e && e[0] == '0'; }();
    const dim3 grid((unsigned)mgf_cdiv(hw, pxb), n);
#define MGF_LPB_LAUNCH(PX, CP)                                                                                                                     \
    do {                                                                                                                                           \
        if (wmap)                                                                                                                                  \
            hipLaunchKernelGGL((lpips_layer_bwd_kernel<PX, RELU, CP, true>), grid, dim3(256), 0, st, oa, ob, din, f0, f1u, lin, c, c_split, hw,    \
                               f1_bs, k, accumulate, stats, wmap, w_bs);                                                                           \
        else                                                                                                                                       \
            hipLaunchKernelGGL((lpips_layer_bwd_kernel<PX, RELU, CP>), grid, dim3(256), 0, st, oa, ob, din, f0, f1u, lin, c, c_split, hw, f1_bs,   \
                               k, accumulate, stats, nullptr, 0);                                                                                  \
    } while (0)
    if (pxb == 64) {
        if (c <= 64 && !no_cache && !stats) MGF_LPB_LAUNCH(64, 16);
        else MGF_LPB_LAUNCH(64, 0);
    } else if (pxb == 32) {
        if (c <= 128 && !no_cache && !stats) MGF_LPB_LAUNCH(32, 16);
        else MGF_LPB_LAUNCH(32, 0);
    } else MGF_LPB_LAUNCH(16, 0);
#undef MGF_LPB_LAUNCH
}

extern "C" int mgf_lpips_layer_bwd_f32(float* df0, const float* f0, const float* f1_unit, const float* lin, int32_t n, int32_t c, int64_t hw,
                                       int64_t f1_batch_stride, float scale, int32_t accumulate, mgf_stream_t stream) {
    MGF_REQUIRE(df0 && f0 && f1_unit && lin && n >= 1 && c >= 1 && hw >= 1, MGF_EINVAL, "lpips_layer_bwd: bad arguments");
    MGF_REQUIRE((int64_t)c * hw < (1LL << 30), MGF_ETOOBIG, "lpips_layer_bwd: one sample's tap must stay below 4 GiB (32-bit buffer offsets)");
    MGF_REQUIRE(n <= 65535, MGF_ETOOBIG, "lpips_layer_bwd: n must be <= 65535");
    const float kk = 2.f * scale / (float)hw;
    lpips_bwd_launch<false>(df0, nullptr, nullptr, f0, f1_unit, lin, n, c, c, hw, f1_batch_stride, kk, accumulate, (hipStream_t)stream);
    MGF_CHECK_LAUNCH("lpips_layer_bwd");
    return MGF_OK;
}

extern "C" int mgf_lpips_layer_bwd_relu_f32(float* dz_a, float* dz_b, const float* dy, const float* f0, const float* f1_unit,
                                            const float* lin, int32_t n, int32_t c, int32_t c_split, int64_t hw, int64_t f1_batch_stride,
                                            float scale, mgf_stream_t stream) {
    return mgf_lpips_layer_bwd_relu_stats_f32(dz_a, dz_b, dy, f0, f1_unit, lin, nullptr, n, c, c_split, hw, f1_batch_stride, scale, stream);
}

extern "C" int mgf_lpips_layer_bwd_relu_stats_f32(float* dz_a, float* dz_b, const float* dy, const float* f0, const float* f1_unit,
                                                  const float* lin, const float* stats, int32_t n, int32_t c, int32_t c_split, int64_t hw,
                                                  int64_t f1_batch_stride, float scale, mgf_stream_t stream) {
    MGF_REQUIRE(dz_a && f0 && f1_unit && lin && n >= 1 && c >= 1 && hw >= 1, MGF_EINVAL, "lpips_layer_bwd_relu: bad arguments");
    MGF_REQUIRE(c_split >= 1 && c_split <= c && (dz_b || c_split == c), MGF_EINVAL, "lpips_layer_bwd_relu: bad split %d of %d channels", c_split, c);
    MGF_REQUIRE(n <= 65535, MGF_ETOOBIG, "lpips_layer_bwd_relu: n must be <= 65535");
    MGF_REQUIRE((int64_t)c * hw < (1LL << 30), MGF_ETOOBIG, "lpips_layer_bwd_relu: one sample's tap must stay below 4 GiB (32-bit buffer offsets)");
    const float kk = 2.f * scale / (float)hw;
    lpips_bwd_launch<true>(dz_a, dz_b, dy, f0, f1_unit, lin, n, c, c_split, hw, f1_batch_stride, kk, 0, (hipStream_t)stream, stats);
    MGF_CHECK_LAUNCH("lpips_layer_bwd_relu");
    return MGF_OK;
}

/* The region-weighted forms: the factor 2 scale / hw becomes 2 scale omega[p] (wmap: normalised weights, w_batch_stride 0 = shared) */
extern "C" int mgf_lpips_layer_bwd_weighted_f32(float* df0, const float* f0, const float* f1_unit, const float* lin, const float* wmap, int32_t n,
                                                int32_t c, int64_t hw, int64_t f1_batch_stride, int64_t w_batch_stride, float scale,
                                                int32_t accumulate, mgf_stream_t stream) {
    MGF_REQUIRE(df0 && f0 && f1_unit && lin && wmap && n >= 1 && c >= 1 && hw >= 1 && w_batch_stride >= 0, MGF_EINVAL, "lpips_layer_bwd_weighted: bad arguments");
    MGF_REQUIRE((int64_t)c * hw < (1LL << 30), MGF_ETOOBIG, "lpips_layer_bwd_weighted: one sample's tap must stay below 4 GiB (32-bit buffer offsets)");
    MGF_REQUIRE(n <= 65535, MGF_ETOOBIG, "lpips_layer_bwd_weighted: n must be <= 65535");
    lpips_bwd_launch<false>(df0, nullptr, nullptr, f0, f1_unit, lin, n, c, c, hw, f1_batch_stride, 2.f * scale, accumulate, (hipStream_t)stream, nullptr,
                            wmap, w_batch_stride);
    MGF_CHECK_LAUNCH("lpips_layer_bwd_weighted");
    return MGF_OK;
}

extern "C" int mgf_lpips_layer_bwd_relu_stats_weighted_f32(float* dz_a, float* dz_b, const float* dy, const float* f0, const float* f1_unit,
                                                           const float* lin, const float* stats, const float* wmap, int32_t n, int32_t c,
                                                           int32_t c_split, int64_t hw, int64_t f1_batch_stride, int64_t w_batch_stride,
                                                           float scale, mgf_stream_t stream) {
    MGF_REQUIRE(dz_a && f0 && f1_unit && lin && wmap && n >= 1 && c >= 1 && hw >= 1 && w_batch_stride >= 0, MGF_EINVAL, "lpips_layer_bwd_relu_weighted: bad arguments");
    MGF_REQUIRE(c_split >= 1 && c_split <= c && (dz_b || c_split == c), MGF_EINVAL, "lpips_layer_bwd_relu_weighted: bad split %d of %d channels", c_split, c);
    MGF_REQUIRE(n <= 65535, MGF_ETOOBIG, "lpips_layer_bwd_relu_weighted: n must be <= 65535");
    MGF_REQUIRE((int64_t)c * hw < (1LL << 30), MGF_ETOOBIG, "lpips_layer_bwd_relu_weighted: one sample's tap must stay below 4 GiB (32-bit buffer offsets)");
    lpips_bwd_launch<true>(dz_a, dz_b, dy, f0, f1_unit, lin, n, c, c_split, hw, f1_batch_stride, 2.f * scale, 0, (hipStream_t)stream, stats, wmap,
                           w_batch_stride);
    MGF_CHECK_LAUNCH("lpips_layer_bwd_relu_weighted");
    return MGF_OK;
}

extern "C" int mgf_relu_bwd_split_f32(float* dz_a, float* dz_b, const float* dy, const float* y, int32_t n, int32_t c, int32_t c_split,
                                      int64_t hw, mgf_stream_t stream) {
    MGF_REQUIRE(dz_a && dy && y && n >= 1 && c >= 1 && hw >= 1, MGF_EINVAL, "relu_bwd_split: bad arguments");
    MGF_REQUIRE(c_split >= 1 && c_split <= c && (dz_b || c_split == c), MGF_EINVAL, "relu_bwd_split: bad split %d of %d channels", c_split, c);
    const int64_t total = (int64_t)n * c * hw;
    hipLaunchKernelGGL(relu_bwd_split_kernel, dim3(mgf_stream_grid(total, 256, 4)), dim3(256), 0, (hipStream_t)stream, dz_a, dz_b, dy, y, c,
                       c_split, hw, total);
    MGF_CHECK_LAUNCH("relu_bwd_split");
    return MGF_OK;
}

extern "C" int mgf_mse_grad_f32(float* d, const float* a, const float* b, int32_t n, int64_t numel, int64_t b_batch_stride, float scale,
                                int32_t accumulate, mgf_stream_t stream) {
    MGF_REQUIRE(d && a && b && n >= 1 && numel >= 1, MGF_EINVAL, "mse_grad: bad arguments");
    const int64_t total = (int64_t)n * numel;
    hipLaunchKernelGGL(mse_grad_kernel, dim3(mgf_stream_grid(total, 256, 4)), dim3(256), 0, (hipStream_t)stream, d, a, b, numel, b_batch_stride,
                       2.f * scale / (float)numel, accumulate, total);
    MGF_CHECK_LAUNCH("mse_grad");
    return MGF_OK;
}
