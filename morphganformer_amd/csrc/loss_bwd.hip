// Gradient mode, loss side: dLoss/dimage of the terms the synthesis network's pass (backward.hip) starts from -- what torch autograd does
// for the reference through the LPIPS taps (lpips/networks_basic.py:64-92), the backbones' ReLU and max-pool layers
// (lpips/pretrained_networks.py) and torch.nn.MSELoss.  The convolutions' data gradients are the forward kernels on transposed taps and live
// with them; here are the element-wise and window kernels:
//   mgf_lpips_layer_bwd*              one tap's gradient, alone or fused with the tap's ReLU backward, plain / from stored stats / weighted
//   mgf_relu_bwd_split_f32            ReLU backward into the two halves of a Fire concat
//   mgf_maxpool*_bwd*                 MaxPool2d(3, 2, ceil_mode) from the input or from stored tap indices, MaxPool2d(2 | 3, 2) floor mode
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

// MaxPool2d(3, 2, ceil_mode=True) backward: the gradient of a window goes to its FIRST maximum in row-major order (torch's argmax rule).
// A workgroup owns a 32 x 32 tile of INPUT elements of one plane.  The 17 x 17 windows that touch it (one row / column of them
// belongs to the neighbouring tile and is recomputed) read a 35 x 35 input patch from LDS; every window's argmax (as a patch offset)
// and gradient are computed once, then each input element collects from the <= 4 windows that cover it.
// Input tile owned by a workgroup: 64 columns x 32 rows (both even: windows start on even rows / columns), the (32/2 + 1) x (64/2 + 1)
// windows that touch it, and their (32 + 3) x (64 + 3) input patch.  The kernel is bound by its instruction count, not by memory
// (2.1 TB/s in its first form): no coordinates are divided, the patch is padded with -inf so the window scan needs no bounds tests,
// and a lane scatters the windows' gradients to one 2 x 2 block of inputs (whose four window memberships are fixed by parity).
constexpr int MPTX = 64, MPTY = 32, MPWX = MPTX / 2 + 1, MPWY = MPTY / 2 + 1, MPIX = MPTX + 3, MPIY = MPTY + 3, MPS = MPIX + 1;
__global__ __launch_bounds__(256) void maxpool3x3s2_bwd_kernel(float* dx, const float* dy, const float* x, int ih, int iw, int oh, int ow,
                                                               int tiles_x, int tiles_y) {
    __shared__ float patch[MPIY * MPS];
    __shared__ int16_t arg[MPWY][MPWX + 1];
    __shared__ float gw[MPWY][MPWX + 1];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y;
    const int64_t pl = blockIdx.x / ((int64_t)tiles_x * tiles_y);
    const int iy0 = ty * MPTY, ix0 = tx * MPTX;          // first owned input row / column
    const int py0 = iy0 - 2, px0 = ix0 - 2;              // patch origin: patch[2 wy + ky][2 wx + kx] is tap (ky, kx) of local window (wy, wx)
    const int wy0 = iy0 / 2 - 1, wx0 = ix0 / 2 - 1;      // first window row / column (may be -1)
    const float* xp = x + pl * ih * iw;
    const float* dp = dy + pl * oh * ow;
    const float NEG = -__builtin_inff();
    {
        const int cc = tid & 63, r0 = tid >> 6;
        const int xx = px0 + cc;
        const bool xin = xx >= 0 && xx < iw;
#pragma unroll
        for (int r = r0; r < MPIY; r += 4) {
            const int yy = py0 + r;
            patch[r * MPS + cc] = (xin && yy >= 0 && yy < ih) ? xp[(int64_t)yy * iw + xx] : NEG;
        }
        if (tid < 3 * MPIY) {                            // the three columns past the 64th
            const int r = tid / 3, c3 = 64 + tid - 3 * r;
            const int yy = py0 + r, x3 = px0 + c3;
            patch[r * MPS + c3] = (x3 < iw && yy >= 0 && yy < ih) ? xp[(int64_t)yy * iw + x3] : NEG;
        }
    }
    __syncthreads();
    for (int i = tid; i < MPWY * MPWX; i += 256) {
        const int wy = i / MPWX, wx = i - wy * MPWX;
        const int oy = wy0 + wy, ox = wx0 + wx;
        int best = -1;
        float g = 0.f;
        if (oy >= 0 && ox >= 0 && oy < oh && ox < ow) {  // tap (0, 0) of a window that exists is inside the input
            const int base = 2 * wy * MPS + 2 * wx;
            float bv = patch[base];
            best = base;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    if (ky == 0 && kx == 0) continue;
                    const float v = patch[base + ky * MPS + kx];
                    if (v > bv) { bv = v; best = base + ky * MPS + kx; }       // first maximum in row-major order (torch)
                }
            g = dp[(int64_t)oy * ow + ox];
        }
        arg[wy][wx] = (int16_t)best;
        gw[wy][wx] = g;
    }
    __syncthreads();
    // input block (2 br, 2 bc) + {0,1}^2 of the tile: windows (br, bc) .. (br + 1, bc + 1) in local indices; element (0,0) is in
    // all four, (0,1) in the right two, (1,0) in the lower two, (1,1) in the last -- summed in ascending window order like torch
#pragma unroll
    for (int i = tid; i < (MPTY / 2) * (MPTX / 2); i += 256) {
        const int br = i / (MPTX / 2), bc = i - br * (MPTX / 2);
        const int yy = iy0 + 2 * br, xx = ix0 + 2 * bc;
        if (yy >= ih || xx >= iw) continue;
        const int me = (2 * br + 2) * MPS + 2 * bc + 2;
        const int a00 = arg[br][bc], a01 = arg[br][bc + 1], a10 = arg[br + 1][bc], a11 = arg[br + 1][bc + 1];
        const float g00 = gw[br][bc], g01 = gw[br][bc + 1], g10 = gw[br + 1][bc], g11 = gw[br + 1][bc + 1];
        float e00 = 0.f, e01 = 0.f, e10 = 0.f, e11 = 0.f;
        if (a00 == me) e00 += g00;
        if (a01 == me) e00 += g01;
        if (a10 == me) e00 += g10;
        if (a11 == me) e00 += g11;
        if (a01 == me + 1) e01 += g01;
        if (a11 == me + 1) e01 += g11;
        if (a10 == me + MPS) e10 += g10;
        if (a11 == me + MPS) e10 += g11;
        if (a11 == me + MPS + 1) e11 += g11;
        float* o = dx + pl * ih * iw + (int64_t)yy * iw + xx;
        const bool x1 = xx + 1 < iw;
        o[0] = e00;
        if (x1) o[1] = e01;
        if (yy + 1 < ih) {
            o[iw] = e10;
            if (x1) o[iw + 1] = e11;
        }
    }
}

// MaxPool2d(2, 2) backward (VGG): windows do not overlap, an input element belongs to at most one
__global__ __launch_bounds__(256) void maxpool2x2s2_bwd_kernel(float* dx, const float* dy, const float* x, int ih, int iw, int oh, int ow,
                                                               int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ix = (int)(i % iw);
        const int64_t r = i / iw;
        const int iy = (int)(r % ih);
        const int64_t pl = r / ih;
        const int oy = iy / 2, ox = ix / 2;
        float g = 0.f;
        if (oy < oh && ox < ow) {
            const float* xp = x + pl * ih * iw + (int64_t)(2 * oy) * iw + 2 * ox;
            const float v00 = xp[0], v01 = xp[1], v10 = xp[iw], v11 = xp[iw + 1];
            int best = 0;
            float bv = v00;
            if (v01 > bv) { bv = v01; best = 1; }
            if (v10 > bv) { bv = v10; best = 2; }
            if (v11 > bv) { bv = v11; best = 3; }
            if (best == (iy & 1) * 2 + (ix & 1)) g = dy[pl * oh * ow + (int64_t)oy * ow + ox];
        }
        dx[i] = g;
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

namespace {
// dx of the 3x3 / stride-2 ceil-mode pool from the forward's stored tap indices: one lane per 2 x 2 input block (2 bi, 2 bj) + {0,1}^2,
// whose elements sit at fixed taps of the <= 4 windows around it -- (0,0): tap 8 of window (bi-1, bj-1), 6 of (bi-1, bj), 2 of
// (bi, bj-1), 0 of (bi, bj); (0,1): 7 of (bi-1, bj), 1 of (bi, bj); (1,0): 5 of (bi, bj-1), 3 of (bi, bj); (1,1): 4 of (bi, bj) --
// summed in ascending window order like torch.  No LDS, no input map: a stream of stores.
__global__ __launch_bounds__(256) void maxpool3x3s2_bwd_idx_kernel(float* __restrict__ dx, const float* __restrict__ dy,
                                                                   const uint8_t* __restrict__ idx, int ih, int iw, int oh, int ow) {
    const int bj = blockIdx.x * 256 + threadIdx.x, bi = blockIdx.y;
    const int64_t pl = blockIdx.z;
    const int yy = 2 * bi, xx = 2 * bj;
    if (xx >= iw) return;
    const float* dp = dy + pl * oh * ow;
    const uint8_t* ip = idx + pl * oh * ow;
    float g[2][2];
    int t[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int oy = bi - 1 + a, ox = bj - 1 + b;
            const bool in = oy >= 0 && ox >= 0 && oy < oh && ox < ow;
            g[a][b] = in ? dp[(int64_t)oy * ow + ox] : 0.f;
            t[a][b] = in ? (int)ip[(int64_t)oy * ow + ox] : -1;
        }
    float e00 = 0.f, e01 = 0.f, e10 = 0.f, e11 = 0.f;
    if (t[0][0] == 8) e00 += g[0][0];
    if (t[0][1] == 6) e00 += g[0][1];
    if (t[1][0] == 2) e00 += g[1][0];
    if (t[1][1] == 0) e00 += g[1][1];
    if (t[0][1] == 7) e01 += g[0][1];
    if (t[1][1] == 1) e01 += g[1][1];
    if (t[1][0] == 5) e10 += g[1][0];
    if (t[1][1] == 3) e10 += g[1][1];
    if (t[1][1] == 4) e11 += g[1][1];
    float* o = dx + pl * ih * iw + (int64_t)yy * iw + xx;
    const bool x1 = xx + 1 < iw;
    o[0] = e00;
    if (x1) o[1] = e01;
    if (yy + 1 < ih) {
        o[iw] = e10;
        if (x1) o[iw + 1] = e11;
    }
}
}  // namespace

extern "C" int mgf_maxpool3x3s2_ceil_bwd_idx_f32(float* dx, const float* dy, const uint8_t* idx, int32_t nc, int32_t in_h, int32_t in_w,
                                                 int32_t out_h, int32_t out_w, mgf_stream_t stream) {
    MGF_REQUIRE(dx && dy && idx && nc >= 1 && in_h >= 1 && in_w >= 1 && out_h >= 1 && out_w >= 1, MGF_EINVAL, "maxpool3x3s2_ceil_bwd_idx: bad arguments");
    MGF_REQUIRE(2 * (out_h - 1) < in_h && 2 * (out_w - 1) < in_w, MGF_EINVAL, "maxpool3x3s2_ceil_bwd_idx: output extent does not match the input");
    MGF_REQUIRE(nc <= 65535 && (in_h + 1) / 2 <= 65535, MGF_ETOOBIG, "maxpool3x3s2_ceil_bwd_idx: at most 65535 planes and 131070 rows");
    const dim3 grid((unsigned)mgf_cdiv((in_w + 1) / 2, 256), (unsigned)((in_h + 1) / 2), nc);
    hipLaunchKernelGGL(maxpool3x3s2_bwd_idx_kernel, grid, dim3(256), 0, (hipStream_t)stream, dx, dy, idx, in_h, in_w, out_h, out_w);
    MGF_CHECK_LAUNCH("maxpool3x3s2_ceil_bwd_idx");
    return MGF_OK;
}

extern "C" int mgf_maxpool3x3s2_ceil_bwd_f32(float* dx, const float* dy, const float* x, int32_t nc, int32_t in_h, int32_t in_w, int32_t out_h,
                                             int32_t out_w, mgf_stream_t stream) {
    MGF_REQUIRE(dx && dy && x && nc >= 1 && in_h >= 1 && in_w >= 1 && out_h >= 1 && out_w >= 1, MGF_EINVAL, "maxpool3x3s2_ceil_bwd: bad arguments");
    MGF_REQUIRE(2 * (out_h - 1) < in_h && 2 * (out_w - 1) < in_w, MGF_EINVAL, "maxpool3x3s2_ceil_bwd: output extent does not match the input");
    const int tiles_x = (int)mgf_cdiv(in_w, MPTX), tiles_y = (int)mgf_cdiv(in_h, MPTY);
    MGF_REQUIRE((int64_t)nc * tiles_x * tiles_y <= INT32_MAX, MGF_ETOOBIG, "maxpool3x3s2_ceil_bwd: too many tiles");
    hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel, dim3((unsigned)((int64_t)nc * tiles_x * tiles_y)), dim3(256), 0, (hipStream_t)stream, dx, dy, x,
                       in_h, in_w, out_h, out_w, tiles_x, tiles_y);
    MGF_CHECK_LAUNCH("maxpool3x3s2_ceil_bwd");
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

extern "C" int mgf_maxpool_s2_floor_bwd_f32(float* dx, const float* dy, const float* x, int32_t nc, int32_t in_h, int32_t in_w, int32_t ksize,
                                            mgf_stream_t stream) {
    MGF_REQUIRE(dx && dy && x && nc >= 1 && (ksize == 2 || ksize == 3) && in_h >= ksize && in_w >= ksize, MGF_EINVAL, "maxpool_s2_floor_bwd: bad arguments");
    const int out_h = (in_h - ksize) / 2 + 1, out_w = (in_w - ksize) / 2 + 1;
    if (ksize == 3) return mgf_maxpool3x3s2_ceil_bwd_f32(dx, dy, x, nc, in_h, in_w, out_h, out_w, stream);      // same rule, fewer windows
    const int64_t total = (int64_t)nc * in_h * in_w;
    hipLaunchKernelGGL(maxpool2x2s2_bwd_kernel, dim3(mgf_stream_grid(total, 256, 2)), dim3(256), 0, (hipStream_t)stream, dx, dy, x, in_h, in_w,
                       out_h, out_w, total);
    MGF_CHECK_LAUNCH("maxpool_s2_floor_bwd");
    return MGF_OK;
}
