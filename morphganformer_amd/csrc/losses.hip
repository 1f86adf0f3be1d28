// Losses of the projection loop, all device-side so an iteration never synchronises with the host: MSE and its region-weighted forms, the
// LPIPS tap distance (scalar and spatial), Wing / AWing.  (The pools: maxpool.hip; the loop's step kernels: loop_step.hip; DSSIM: dssim.hip.)
// Contract: include/mgf.h.  Every op is BATCHED over n independent candidates (the literal loop's steps do not depend on each
// other, so several of them are evaluated per generator forward); reductions are deterministic: fixed grid, per-block
// partials in `scratch`, one finishing block per sample sums them in index order (no float atomics -> bit-reproducible).
#include "mgf_common.h"

namespace {

constexpr int RED_BLOCKS = 16384;     // scratch floats per sample

// (not mgf_block_sum_256 of mgf_common.h: this one's second barrier comes AFTER the read -- sm is free on return, not on entry)
__device__ __forceinline__ float block_sum_256(float v, float* sm) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sm[0] + sm[1] + sm[2] + sm[3];
    __syncthreads();
    return r;
}

// out[s] (+)= scale * sum(scratch[s][0 .. nparts))   -- one workgroup per sample
__global__ __launch_bounds__(256) void finish_kernel(float* out, const float* scratch, int nparts, float scale, int accumulate) {
    __shared__ float sm[4];
    const float* sc = scratch + (int64_t)blockIdx.x * RED_BLOCKS;
    float v = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) v += sc[i];
    v = block_sum_256(v, sm);
    if (threadIdx.x == 0) out[blockIdx.x] = (accumulate ? out[blockIdx.x] : 0.f) + v * scale;
}

// the same finish for up to 8 partial sets at once (the taps of one LPIPS evaluation), added to out[s] in set order with the arithmetic of
// that many finish_kernel launches: out = (accumulate ? out : 0) + v_0 * scale_0; out += v_1 * scale_1; ...
struct FinishSets { int nparts[8]; float scale[8]; };
__global__ __launch_bounds__(256) void finish_multi_kernel(float* out, const float* scratch, int64_t set_stride, int nsets, FinishSets fs, int accumulate) {
    __shared__ float sm[4];
    float acc = accumulate ? out[blockIdx.x] : 0.f;
    for (int t = 0; t < nsets; ++t) {
        const float* sc = scratch + (int64_t)t * set_stride + (int64_t)blockIdx.x * RED_BLOCKS;
        float v = 0.f;
        for (int i = threadIdx.x; i < fs.nparts[t]; i += 256) v += sc[i];
        v = block_sum_256(v, sm);
        acc = acc + v * fs.scale[t];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

// grid = (blocks, n)
__global__ __launch_bounds__(256) void mse_partial_kernel(float* scratch, const float* a, const float* b, int64_t numel, int64_t b_stride) {
    __shared__ float sm[4];
    const float* as = a + (int64_t)blockIdx.y * numel;
    const float* bs = b + (int64_t)blockIdx.y * b_stride;
    float acc = 0.f;
    const int64_t nvec = numel / 4;
    const float4* a4 = reinterpret_cast<const float4*>(as);
    const float4* b4 = reinterpret_cast<const float4*>(bs);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
        float4 u = a4[i], v = b4[i];
        float d0 = u.x - v.x, d1 = u.y - v.y, d2 = u.z - v.z, d3 = u.w - v.w;
        acc += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    for (int64_t i = nvec * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += (int64_t)gridDim.x * 256) {
        float d0 = as[i] - bs[i];
        acc += d0 * d0;
    }
    acc = block_sum_256(acc, sm);
    if (threadIdx.x == 0) scratch[(int64_t)blockIdx.y * RED_BLOCKS + blockIdx.x] = acc;
}

// Region-weighted pixel term on [n][c][hw] images: a thread takes quads of 4 consecutive elements of a sample (flat over c * hw) with the
// weight of each element's pixel.  VEC (hw % 4 == 0, all pointers 16-byte aligned per sample): a quad lies in one channel plane and is three
// 16-byte loads; otherwise the same quad through scalar loads -- the same operands in the same expressions, so both paths give the same bits.
template <bool VEC>
__device__ __forceinline__ void wquad_load(float (&u)[4], float (&v)[4], float (&w)[4], const float* as, const float* bs, const float* ws,
                                           int64_t q, int64_t numel, int64_t hw) {
    if (VEC) {
        const float4 a4 = reinterpret_cast<const float4*>(as)[q], b4 = reinterpret_cast<const float4*>(bs)[q];
        const float4 w4 = reinterpret_cast<const float4*>(ws)[q % (hw >> 2)];
        u[0] = a4.x; u[1] = a4.y; u[2] = a4.z; u[3] = a4.w;
        v[0] = b4.x; v[1] = b4.y; v[2] = b4.z; v[3] = b4.w;
        w[0] = w4.x; w[1] = w4.y; w[2] = w4.z; w[3] = w4.w;
    } else {
        int64_t p = (q * 4) % hw;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t i = q * 4 + e;
            const bool in = i < numel;                      // the last quad of a sample may be ragged: a = b = w = 0 adds +0
            u[e] = in ? as[i] : 0.f; v[e] = in ? bs[i] : 0.f; w[e] = in ? ws[p] : 0.f;
            if (++p == hw) p = 0;
        }
    }
}

// grid = (blocks, n): scratch[s][block] = sum over the block's quads of omega[p] (a - b)^2
template <bool VEC>
__global__ __launch_bounds__(256) void mse_weighted_partial_kernel(float* scratch, const float* a, const float* b, const float* wmap, int64_t numel,
                                                                   int64_t hw, int64_t b_stride, int64_t w_stride) {
    __shared__ float sm[4];
    const float* as = a + (int64_t)blockIdx.y * numel;
    const float* bs = b + (int64_t)blockIdx.y * b_stride;
    const float* ws = wmap + (int64_t)blockIdx.y * w_stride;
    const int64_t nquad = (numel + 3) >> 2;
    float acc = 0.f;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * 256) {
        float u[4], v[4], w[4];
        wquad_load<VEC>(u, v, w, as, bs, ws, q, numel, hw);
        const float d0 = u[0] - v[0], d1 = u[1] - v[1], d2 = u[2] - v[2], d3 = u[3] - v[3];
        acc += w[0] * (d0 * d0) + w[1] * (d1 * d1) + w[2] * (d2 * d2) + w[3] * (d3 * d3);
    }
    acc = block_sum_256(acc, sm);
    if (threadIdx.x == 0) scratch[(int64_t)blockIdx.y * RED_BLOCKS + blockIdx.x] = acc;
}

// grid = (blocks, n): d (+)= k omega[p] (a - b)        (k = 2 scale)
template <bool VEC>
__global__ __launch_bounds__(256) void mse_weighted_grad_kernel(float* d, const float* a, const float* b, const float* wmap, int64_t numel, int64_t hw,
                                                                int64_t b_stride, int64_t w_stride, float k, int accumulate) {
    const float* as = a + (int64_t)blockIdx.y * numel;
    const float* bs = b + (int64_t)blockIdx.y * b_stride;
    const float* ws = wmap + (int64_t)blockIdx.y * w_stride;
    float* ds = d + (int64_t)blockIdx.y * numel;
    const int64_t nquad = (numel + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * 256) {
        float u[4], v[4], w[4], g[4];
        wquad_load<VEC>(u, v, w, as, bs, ws, q, numel, hw);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = (k * w[e]) * (u[e] - v[e]);
        if (VEC) {
            float4* dp = reinterpret_cast<float4*>(ds) + q;
            if (accumulate) { const float4 o = *dp; g[0] = o.x + g[0]; g[1] = o.y + g[1]; g[2] = o.z + g[2]; g[3] = o.w + g[3]; }
            *dp = make_float4(g[0], g[1], g[2], g[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t i = q * 4 + e;
                if (i < numel) ds[i] = accumulate ? ds[i] + g[e] : g[e];
            }
        }
    }
}

// grid = (pixel blocks, n).  A workgroup owns PXB consecutive pixels of one sample (lanes = consecutive pixels, so a wave reads
// whole 64/256-byte segments of a channel plane); its G = 256 / PXB lane groups take the channels grp, grp + G, grp + 2G ...
// ONE sweep over HBM: each thread keeps its <= CPT channel values in registers, the squared norms meet in LDS in a fixed order
// (bit-reproducible), then the registers are either written back unit-normalised (UNIT_OUT: the reference image's taps, once
// per target) or compared with the stored unit-normalised reference taps and reduced to one partial per workgroup.
// MAP (spatial LPIPS, networks_basic.py:75-76): the per-pixel distance itself is the result -- the G lane groups' d meet in LDS, are added in
// group order and lane group 0 stores one float per pixel to `stats` (here the [n][hw] map); no partial sums, no finish launch.
// WEIGHTED (region weights): the partial sums are of omega[p] * d[p] -- every lane loads its pixel's normalised weight (one more buffer
// load; the G lane groups of a pixel hit the same line) and scales its own share of d; STATS are formed as without a weight.
template <int PXB, int CPT, bool UNIT_OUT, bool STATS = false, bool MAP = false, bool WEIGHTED = false>
__global__ __launch_bounds__(256) void lpips_layer_kernel(float* scratch, float* unit_out, const float* f0, const float* f1u,
                                                           const float* lin, int c, int64_t hw, int64_t f1_stride, int nsamp, int nblk,
                                                           int xcd_per, float* stats, const float* wmap, int64_t w_stride) {
    constexpr int G = 256 / PXB;
    __shared__ float red[G][PXB];
    __shared__ float redb[(STATS || MAP) ? G : 1][PXB], redc[STATS ? G : 1][PXB];      // STATS: the two other per-pixel sums the gradient needs
    __shared__ float sm[4];
    const int px = threadIdx.x % PXB, grp = threadIdx.x / PXB;
    // work order: XCD b % 8 walks a contiguous item range with the SAMPLE as the fastest index -- the n candidates of a pixel block read
    // the same block of the target's stored taps and now share it through one L2 (it came from the Infinity Cache once per candidate:
    // as many bytes again as the candidates' own taps)
    int item = (blockIdx.x & 7) * xcd_per + (blockIdx.x >> 3);
    if (item >= nsamp * nblk) return;
    const int nn = item % nsamp;
    const int blk = item / nsamp;
    const int64_t i = (int64_t)blk * PXB + px;
    const bool valid = i < hw;
    const int64_t pp = valid ? i : hw - 1;
    // Buffer addressing: a thread's channels are G planes apart, so the channel part of every address is a wave-uniform scalar offset
    // (j * G * hw) on ONE per-lane offset (grp * hw + pixel); a channel past c gets an offset beyond num_records and reads 0.  With flat
    // addresses each of the 2 * CPT loads carried a 64-bit multiply-add (quarter-rate integer multiplies) and its own exec-mask branch.
    const unsigned plane_bytes = 4u * (unsigned)hw;                                   // host: c * hw * 4 < 2^32
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)(f0 + (int64_t)nn * c * hw), 0, (int)((unsigned)c * plane_bytes), 0x00020000);
    const unsigned vo = (unsigned)grp * plane_bytes + 4u * (unsigned)pp;
    float u[CPT], v[UNIT_OUT ? 1 : CPT];
    float na = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; ++j)
        u[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra, grp + j * G < c ? vo : 0xFFFFFFF0u, (int)((unsigned)(j * G) * plane_bytes), 0));
    if (!UNIT_OUT) {                    // the reference taps are requested in the same burst: one memory round trip per workgroup
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(f1u + (int64_t)nn * f1_stride), 0, (int)((unsigned)c * plane_bytes), 0x00020000);
#pragma unroll
        for (int j = 0; j < CPT; ++j)
            v[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, grp + j * G < c ? vo : 0xFFFFFFF0u, (int)((unsigned)(j * G) * plane_bytes), 0));
    }
#pragma unroll
    for (int j = 0; j < CPT; ++j) na += u[j] * u[j];
    red[grp][px] = na;
    __syncthreads();
    na = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) na += red[g][px];
    const float ia = 1.f / (sqrtf(na) + 1e-10f);
    if (UNIT_OUT) {
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)(unit_out + (int64_t)nn * c * hw), 0, (int)((unsigned)c * plane_bytes), 0x00020000);
#pragma unroll
        for (int j = 0; j < CPT; ++j)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, u[j] * ia), ro, (valid && grp + j * G < c) ? vo : 0xFFFFFFF0u,
                                                  (int)((unsigned)(j * G) * plane_bytes), 0);
        return;
    }
    float d = 0.f, nb = 0.f, nc = 0.f;
    const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc((void*)lin, 0, 4 * c, 0x00020000);
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        // (no `k < c` branch: a channel past c arrived as u = v = 0 and its `lin` read is out of range, i.e. 0 as well)
        // separate statements: the product is rounded before the subtraction (build uses -ffp-contract=on) exactly like the
        // stored reference taps (u * ia above), so identical images give exactly zero
        const float ua = u[j] * ia;
        const float e = ua - v[UNIT_OUT ? 0 : j];
        const float l = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rl, 4u * (unsigned)grp, 4 * j * G, 0));
        d += l * e * e;
        if (STATS) { nb += l * u[j] * u[j]; nc += l * v[UNIT_OUT ? 0 : j] * u[j]; }
    }
    // STATS (gradient mode): A = sum f0^2, B = sum lin f0^2, C = sum lin u1 f0 per pixel -> [n][3][hw]; the backward
    // (mgf_lpips_layer_bwd_relu_stats_f32) then skips its own sweep over both maps for them.  Formed beside the distance (same operands, two
    // more FMAs; as a loop of their own they cost the forward 75 % more time than they saved the backward)
    if (STATS) {
        redb[grp][px] = nb;
        redc[grp][px] = nc;
        __syncthreads();
        if (grp == 0 && valid) {
            float sb = 0.f, sc = 0.f;
#pragma unroll
            for (int g = 0; g < G; ++g) { sb += redb[g][px]; sc += redc[g][px]; }
            float* so = stats + (int64_t)nn * 3 * hw + i;
            so[0] = na; so[hw] = sb; so[2 * hw] = sc;
        }
    }
    if (MAP) {
        redb[grp][px] = d;
        __syncthreads();
        if (grp == 0 && valid) {
            float sd = 0.f;
#pragma unroll
            for (int g = 0; g < G; ++g) sd += redb[g][px];
            stats[(int64_t)nn * hw + i] = sd;
        }
        return;
    }
    if (WEIGHTED) {
        // loaded HERE, behind the barriers and the channel sweep, not in the tap burst: one more live register through the sweep takes the
        // 64-values-per-thread forms from 168 to 169 VGPRs, i.e. from three waves per SIMD to two (+18 % at 32 x 512 @ 63^2)
        // (the pixel offset is formed again from the thread index -- the empty asm keeps the compiler from carrying `pp` through instead)
        unsigned t = threadIdx.x;
        asm volatile("" : "+v"(t));
        const int64_t iw = (int64_t)blk * PXB + (int)(t % PXB);
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(wmap + (int64_t)nn * w_stride), 0, (int)plane_bytes, 0x00020000);
        d *= __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rw, 4u * (unsigned)(iw < hw ? iw : hw - 1), 0, 0));
    }
    const float acc = block_sum_256(valid ? d : 0.f, sm);
    if (threadIdx.x == 0) scratch[(int64_t)nn * RED_BLOCKS + blk] = acc;
}

template <bool UNIT_OUT>
int launch_lpips_layer(float* scratch, float* unit_out, const float* f0, const float* f1u, const float* lin, int n, int c, int64_t hw,
                       int64_t f1_stride, hipStream_t st, int* grid_out, float* stats = nullptr, float* map = nullptr,
                       const float* wmap = nullptr, int64_t w_stride = 0) {
    // 64 pixels per workgroup (256-byte segments) whenever that still yields >= 4 workgroups per CU, 16 for the small deep taps
    static const int pxb_env = [] { const char* e = mgf_knob("MGF_LPIPS_PXB"); return e ? atoi(e) : 0; }();      // tuning hook: 16 | 32 | 64
    // (re-tuned on buffer addressing, 32 x {128 @ 255^2, 256 @ 127^2, 384 @ 63^2, 512 @ 63^2}, us for 64 / 32 / 16-pixel blocks:
    // 264 / 306 / 386, 145 / 155 / 195, 100 / 60 / 58, 126 / 70 / 74 -- tools/lpips_layer_micro.py; with flat addressing 64 values per thread
    // had been the slow case and the 256-channel tap ran on 32-pixel blocks)
    const int pxb = pxb_env ? pxb_env
                  : (c <= 256 && (hw >= 65536 || (int64_t)n * mgf_cdiv(hw, 64) >= 1024)) ? 64
                  : (c > 384 && (int64_t)n * mgf_cdiv(hw, 32) >= 1024) ? 32 : 16;
    const int64_t grid64 = mgf_cdiv(hw, pxb);
    MGF_REQUIRE(grid64 <= RED_BLOCKS, MGF_ETOOBIG, "lpips_layer: %lld pixels per sample need %lld scratch floats (have %d per sample)",
                (long long)hw, (long long)grid64, RED_BLOCKS);
    MGF_REQUIRE(c <= 512, MGF_EUNSUPPORTED, "lpips_layer: at most 512 channels per tap (got %d)", c);
    MGF_REQUIRE((int64_t)c * hw < (1LL << 30), MGF_ETOOBIG, "lpips_layer: one sample's tap must stay below 4 GiB");
    MGF_REQUIRE(grid64 * n <= INT32_MAX - 8, MGF_ETOOBIG, "lpips_layer: too many workgroups");
    const int xcd_per = (int)mgf_cdiv(grid64 * n, 8);
    const dim3 grid((unsigned)(xcd_per * 8));
    *grid_out = (int)grid64;
#define MGF_LPIPS_LAUNCH(PXB, CPT)                                                                                                            \
    do {                                                                                                                                      \
        if (!UNIT_OUT && wmap && stats)                                                                                                       \
            hipLaunchKernelGGL((lpips_layer_kernel<PXB, CPT, false, true, false, true>), grid, dim3(256), 0, st, scratch, unit_out, f0, f1u,  \
                               lin, c, hw, f1_stride, n, (int)grid64, xcd_per, stats, wmap, w_stride);                                        \
        else if (!UNIT_OUT && wmap)                                                                                                           \
            hipLaunchKernelGGL((lpips_layer_kernel<PXB, CPT, false, false, false, true>), grid, dim3(256), 0, st, scratch, unit_out, f0, f1u, \
                               lin, c, hw, f1_stride, n, (int)grid64, xcd_per, nullptr, wmap, w_stride);                                      \
        else if (!UNIT_OUT && map)                                                                                                            \
            hipLaunchKernelGGL((lpips_layer_kernel<PXB, CPT, false, false, true>), grid, dim3(256), 0, st, scratch, unit_out, f0, f1u, lin, c,\
                               hw, f1_stride, n, (int)grid64, xcd_per, map, nullptr, 0);                                                      \
        else if (!UNIT_OUT && stats)                                                                                                          \
            hipLaunchKernelGGL((lpips_layer_kernel<PXB, CPT, false, true>), grid, dim3(256), 0, st, scratch, unit_out, f0, f1u, lin, c, hw,   \
                               f1_stride, n, (int)grid64, xcd_per, stats, nullptr, 0);                                                        \
        else                                                                                                                                  \
            hipLaunchKernelGGL((lpips_layer_kernel<PXB, CPT, UNIT_OUT>), grid, dim3(256), 0, st, scratch, unit_out, f0, f1u, lin, c, hw,      \
                               f1_stride, n, (int)grid64, xcd_per, nullptr, nullptr, 0);                                                      \
    } while (0)
    if (pxb == 64) {
        if (c <= 128) MGF_LPIPS_LAUNCH(64, 32); else if (c <= 256) MGF_LPIPS_LAUNCH(64, 64); else MGF_LPIPS_LAUNCH(64, 128);
    } else if (pxb == 32) {
        if (c <= 128) MGF_LPIPS_LAUNCH(32, 16); else if (c <= 256) MGF_LPIPS_LAUNCH(32, 32); else MGF_LPIPS_LAUNCH(32, 64);
    } else {
        if (c <= 128) MGF_LPIPS_LAUNCH(16, 8); else if (c <= 256) MGF_LPIPS_LAUNCH(16, 16); else MGF_LPIPS_LAUNCH(16, 32);
    }
#undef MGF_LPIPS_LAUNCH
    return MGF_OK;
}

// one workgroup per candidate: out[j] = WingLoss(pred row (*pred_step + j), target) in float64
__global__ __launch_bounds__(256) void wing_kernel(double* out, const double* pred, const double* target, int64_t numel, double omega,
                                                   double epsilon, const int32_t* pred_step, int max_row) {
    __shared__ double sm[4];
    int row = (pred_step ? *pred_step : 0) + (int)blockIdx.x;
    if (max_row >= 0 && row > max_row) row = max_row;
    pred += (int64_t)row * numel;
    const double cc = omega - omega * log(1.0 + omega / epsilon);
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < numel; i += 256) {
        double dlt = fabs(target[i] - pred[i]);
        acc += dlt < omega ? omega * log(1.0 + dlt / epsilon) : dlt - cc;
    }
    acc = mgf_block_sum_256(acc, sm);
    if (threadIdx.x == 0) out[blockIdx.x] = acc / (double)numel;
}

// AdaptiveWingLoss (adaptive_wing_loss.py:20-39): the exponent alpha - y depends on the TARGET value y; mean over all elements
__global__ __launch_bounds__(256) void awing_kernel(double* out, const double* pred, const double* target, int64_t numel, double omega,
                                                    double theta, double epsilon, double alpha, const int32_t* pred_step, int max_row) {
    __shared__ double sm[4];
    int row = (pred_step ? *pred_step : 0) + (int)blockIdx.x;
    if (max_row >= 0 && row > max_row) row = max_row;
    pred += (int64_t)row * numel;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < numel; i += 256) {
        const double y = target[i];
        const double dlt = fabs(y - pred[i]);
        const double pw = alpha - y;
        if (dlt < theta) {
            acc += omega * log(1.0 + pow(dlt / omega, pw));
        } else {
            const double tp = pow(theta / epsilon, pw);
            const double A = omega * (1.0 / (1.0 + tp)) * pw * pow(theta / epsilon, pw - 1.0) * (1.0 / epsilon);
            const double C = theta * A - omega * log(1.0 + tp);
            acc += A * dlt - C;
        }
    }
    acc = mgf_block_sum_256(acc, sm);
    if (threadIdx.x == 0) out[blockIdx.x] = acc / (double)numel;
}

}  // namespace

extern "C" int64_t mgf_reduce_scratch_floats(void) { return RED_BLOCKS; }

extern "C" int mgf_mse_f32(float* out, const float* a, const float* b, int32_t n, int64_t numel, int64_t b_batch_stride, float scale,
                           int32_t accumulate, float* scratch, mgf_stream_t stream) {
    MGF_REQUIRE(out && a && b && scratch && numel >= 1 && n >= 1 && n <= 65535, MGF_EINVAL, "mse: bad arguments");
    MGF_REQUIRE(((uintptr_t)a % 16 == 0) && ((uintptr_t)b % 16 == 0) && (numel % 4 == 0 || n == 1) && b_batch_stride % 4 == 0, MGF_EINVAL,
                "mse: inputs must be 16-byte aligned per sample");
    const int grid = (int)(mgf_cdiv(numel, 256 * 8) < 1024 ? mgf_cdiv(numel, 256 * 8) : 1024);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mse_partial_kernel, dim3(grid, n), dim3(256), 0, st, scratch, a, b, numel, b_batch_stride);
    hipLaunchKernelGGL(finish_kernel, dim3(n), dim3(256), 0, st, out, scratch, grid, scale / (float)numel, accumulate);
    MGF_CHECK_LAUNCH("mse");
    return MGF_OK;
}

namespace {
// the 16-byte path of the weighted pixel term: whole quads per plane and every sample's rows aligned
bool wquad_vec(const void* a, const void* b, const void* w, const void* d, int32_t n, int64_t numel, int64_t hw, int64_t b_bs, int64_t w_bs) {
    const auto al = [](const void* p) { return (uintptr_t)p % 16 == 0; };
    return hw % 4 == 0 && al(a) && al(b) && al(w) && al(d) && b_bs % 4 == 0 && w_bs % 4 == 0 && (numel % 4 == 0 || n == 1);
}
}  // namespace

extern "C" int mgf_mse_weighted_f32(float* out, const float* a, const float* b, const float* wmap, int32_t n, int32_t c, int64_t hw,
                                    int64_t b_batch_stride, int64_t w_batch_stride, float scale, int32_t accumulate, float* scratch,
                                    mgf_stream_t stream) {
    MGF_REQUIRE(out && a && b && wmap && scratch && c >= 1 && hw >= 1 && n >= 1 && n <= 65535 && b_batch_stride >= 0 && w_batch_stride >= 0,
                MGF_EINVAL, "mse_weighted: bad arguments");
    const int64_t numel = (int64_t)c * hw;
    const int grid = (int)(mgf_cdiv(numel, 256 * 8) < 1024 ? mgf_cdiv(numel, 256 * 8) : 1024);
    hipStream_t st = (hipStream_t)stream;
    if (wquad_vec(a, b, wmap, nullptr, n, numel, hw, b_batch_stride, w_batch_stride))
        hipLaunchKernelGGL(mse_weighted_partial_kernel<true>, dim3(grid, n), dim3(256), 0, st, scratch, a, b, wmap, numel, hw, b_batch_stride, w_batch_stride);
    else
        hipLaunchKernelGGL(mse_weighted_partial_kernel<false>, dim3(grid, n), dim3(256), 0, st, scratch, a, b, wmap, numel, hw, b_batch_stride, w_batch_stride);
    hipLaunchKernelGGL(finish_kernel, dim3(n), dim3(256), 0, st, out, scratch, grid, scale, accumulate);
    MGF_CHECK_LAUNCH("mse_weighted");
    return MGF_OK;
}

extern "C" int mgf_mse_weighted_grad_f32(float* d, const float* a, const float* b, const float* wmap, int32_t n, int32_t c, int64_t hw,
                                         int64_t b_batch_stride, int64_t w_batch_stride, float scale, int32_t accumulate, mgf_stream_t stream) {
    MGF_REQUIRE(d && a && b && wmap && c >= 1 && hw >= 1 && n >= 1 && n <= 65535 && b_batch_stride >= 0 && w_batch_stride >= 0, MGF_EINVAL,
                "mse_weighted_grad: bad arguments");
    const int64_t numel = (int64_t)c * hw;
    const int grid = (int)(mgf_cdiv(numel, 256 * 8) < 1024 ? mgf_cdiv(numel, 256 * 8) : 1024);
    hipStream_t st = (hipStream_t)stream;
    if (wquad_vec(a, b, wmap, d, n, numel, hw, b_batch_stride, w_batch_stride))
        hipLaunchKernelGGL(mse_weighted_grad_kernel<true>, dim3(grid, n), dim3(256), 0, st, d, a, b, wmap, numel, hw, b_batch_stride, w_batch_stride,
                           2.f * scale, accumulate);
    else
        hipLaunchKernelGGL(mse_weighted_grad_kernel<false>, dim3(grid, n), dim3(256), 0, st, d, a, b, wmap, numel, hw, b_batch_stride, w_batch_stride,
                           2.f * scale, accumulate);
    MGF_CHECK_LAUNCH("mse_weighted_grad");
    return MGF_OK;
}

extern "C" int mgf_lpips_unit_f32(float* out, const float* f, int32_t n, int32_t c, int64_t hw, mgf_stream_t stream) {
    MGF_REQUIRE(out && f && n >= 1 && n <= 65535 && c >= 1 && hw >= 1, MGF_EINVAL, "lpips_unit: bad arguments");
    int grid = 0;
    const int rc = launch_lpips_layer<true>(nullptr, out, f, nullptr, nullptr, n, c, hw, 0, (hipStream_t)stream, &grid);
    if (rc != MGF_OK) return rc;
    MGF_CHECK_LAUNCH("lpips_unit");
    return MGF_OK;
}

extern "C" int mgf_lpips_layer_f32(float* out, const float* f0, const float* f1_unit, const float* lin, int32_t n, int32_t c, int64_t hw,
                                   int64_t f1_batch_stride, int32_t accumulate, float* scratch, mgf_stream_t stream) {
    return mgf_lpips_layer_stats_f32(out, nullptr, f0, f1_unit, lin, n, c, hw, f1_batch_stride, accumulate, scratch, stream);
}

extern "C" int mgf_lpips_layer_stats_f32(float* out, float* stats, const float* f0, const float* f1_unit, const float* lin, int32_t n, int32_t c,
                                         int64_t hw, int64_t f1_batch_stride, int32_t accumulate, float* scratch, mgf_stream_t stream) {
    MGF_REQUIRE(out && f0 && f1_unit && lin && scratch && n >= 1 && n <= 65535 && c >= 1 && hw >= 1, MGF_EINVAL, "lpips_layer: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    int grid = 0;
    const int rc = launch_lpips_layer<false>(scratch, nullptr, f0, f1_unit, lin, n, c, hw, f1_batch_stride, st, &grid, stats);
    if (rc != MGF_OK) return rc;
    // spatial mean per sample (networks_basic.py:85-87)
    hipLaunchKernelGGL(finish_kernel, dim3(n), dim3(256), 0, st, out, scratch, grid, 1.0f / (float)hw, accumulate);
    MGF_CHECK_LAUNCH("lpips_layer");
    return MGF_OK;
}

/* mgf_lpips_layer_stats_f32 without its finish launch: the tap's partial sums stay in `scratch` (n * mgf_reduce_scratch_floats() floats: one
 * set per tap) and *nparts_out says how many there are per sample; mgf_lpips_finish_taps_f32 then adds all taps to out in tap order -- the
 * same sums in the same order as one finish per tap, in ONE launch (the loss VALUE is a by-product in gradient mode: nothing waits for it). */
extern "C" int mgf_lpips_layer_defer_f32(float* scratch, float* stats, const float* f0, const float* f1_unit, const float* lin, int32_t n, int32_t c,
                                         int64_t hw, int64_t f1_batch_stride, int32_t* nparts_out, mgf_stream_t stream) {
    MGF_REQUIRE(scratch && f0 && f1_unit && lin && nparts_out && n >= 1 && n <= 65535 && c >= 1 && hw >= 1, MGF_EINVAL, "lpips_layer_defer: bad arguments");
    int grid = 0;
    const int rc = launch_lpips_layer<false>(scratch, nullptr, f0, f1_unit, lin, n, c, hw, f1_batch_stride, (hipStream_t)stream, &grid, stats);
    if (rc != MGF_OK) return rc;
    *nparts_out = grid;
    MGF_CHECK_LAUNCH("lpips_layer_defer");
    return MGF_OK;
}

/* mgf_lpips_layer_defer_f32 with a normalised per-pixel weight: the partials are of omega[p] * d[p] (finish with scale 1) */
extern "C" int mgf_lpips_layer_defer_weighted_f32(float* scratch, float* stats, const float* f0, const float* f1_unit, const float* lin,
                                                  const float* wmap, int32_t n, int32_t c, int64_t hw, int64_t f1_batch_stride,
                                                  int64_t w_batch_stride, int32_t* nparts_out, mgf_stream_t stream) {
    MGF_REQUIRE(scratch && f0 && f1_unit && lin && wmap && nparts_out && n >= 1 && n <= 65535 && c >= 1 && hw >= 1 && w_batch_stride >= 0, MGF_EINVAL,
                "lpips_layer_defer_weighted: bad arguments");
    int grid = 0;
    const int rc = launch_lpips_layer<false>(scratch, nullptr, f0, f1_unit, lin, n, c, hw, f1_batch_stride, (hipStream_t)stream, &grid, stats, nullptr,
                                             wmap, w_batch_stride);
    if (rc != MGF_OK) return rc;
    *nparts_out = grid;
    MGF_CHECK_LAUNCH("lpips_layer_defer_weighted");
    return MGF_OK;
}

extern "C" int mgf_lpips_finish_taps_f32(float* out, const float* scratch, int64_t set_stride_floats, int32_t ntaps, const int32_t* nparts,
                                         const float* scales, int32_t n, int32_t accumulate, mgf_stream_t stream) {
    MGF_REQUIRE(out && scratch && nparts && scales && ntaps >= 1 && ntaps <= 8 && n >= 1 && n <= 65535, MGF_EINVAL, "lpips_finish_taps: bad arguments (1..8 taps)");
    FinishSets fs;
    for (int t = 0; t < 8; ++t) { fs.nparts[t] = t < ntaps ? nparts[t] : 0; fs.scale[t] = t < ntaps ? scales[t] : 0.f; }
    for (int t = 0; t < ntaps; ++t) MGF_REQUIRE(nparts[t] >= 1 && nparts[t] <= RED_BLOCKS, MGF_EINVAL, "lpips_finish_taps: bad partial count");
    hipLaunchKernelGGL(finish_multi_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, out, scratch, set_stride_floats, ntaps, fs, accumulate);
    MGF_CHECK_LAUNCH("lpips_finish_taps");
    return MGF_OK;
}

// ---- spatial LPIPS (PNetLin.forward with spatial=True, lpips/networks_basic.py:20-24,75-76,85-87): the per-pixel tap distance, and the taps'
// maps up-sampled bilinearly to the image size and summed
extern "C" int mgf_lpips_layer_map_f32(float* map, const float* f0, const float* f1_unit, const float* lin, int32_t n, int32_t c, int64_t hw,
                                       int64_t f1_batch_stride, mgf_stream_t stream) {
    MGF_REQUIRE(map && f0 && f1_unit && lin && n >= 1 && n <= 65535 && c >= 1 && hw >= 1, MGF_EINVAL, "lpips_layer_map: bad arguments");
    int grid = 0;
    const int rc = launch_lpips_layer<false>(nullptr, nullptr, f0, f1_unit, lin, n, c, hw, f1_batch_stride, (hipStream_t)stream, &grid, nullptr, map);
    if (rc != MGF_OK) return rc;
    MGF_CHECK_LAUNCH("lpips_layer_map");
    return MGF_OK;
}

namespace {

// the tap table travels in the kernel arguments (by value, like RegLevels of csrc/noise_opt.hip): nothing to allocate, copy or wait for
struct UpTaps { const float* map[8]; int side[8]; float rscale[8]; };

// torch's source index and weight of one axis (UpSample.h: area_pixel_compute_source_index + guard_index_and_lambda, align_corners=False)
__device__ __forceinline__ void up_axis(float rscale, int dst, int side, int& i0, int& i1, float& l0, float& l1) {
    float s = rscale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = min((int)s, side - 1);
    i1 = min(i0 + 1, side - 1);
    l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
    l0 = 1.f - l1;
}

// grid = (column blocks, H rows, n).  A thread owns 4 consecutive pixels of one output row (VEC: one 16-byte store; else -- H % 4 != 0 or an
// unaligned `out` -- four guarded scalar stores of the same values); the row is uniform in a workgroup, so every tap's row indices and row
// weights are scalars.  The tap loop is unrolled over the table, so the table never leaves the scalar registers.
template <bool VEC>
__global__ __launch_bounds__(256) void lpips_upsample_sum_kernel(float* __restrict__ out, UpTaps t, int ntaps, int H, int accumulate) {
    const int x0 = 4 * (int)(blockIdx.x * 256 + threadIdx.x);
    if (x0 >= H) return;
    const int y = blockIdx.y;
    float* o = out + ((int64_t)blockIdx.z * H + y) * H + x0;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (accumulate) {
        if (VEC) {
            const float4 p = *reinterpret_cast<const float4*>(o);
            acc[0] = p.x; acc[1] = p.y; acc[2] = p.z; acc[3] = p.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < H) acc[k] = o[k];
        }
    }
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        if (l >= ntaps) break;
        const int side = t.side[l];
        const float rs = t.rscale[l];
        const float* m = t.map[l] + (int64_t)blockIdx.z * side * side;
        int ya, yb;
        float ly0, ly1;
        up_axis(rs, y, side, ya, yb, ly0, ly1);
        const float* ra = m + (int64_t)ya * side;
        const float* rb = m + (int64_t)yb * side;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int xa, xb;
            float lx0, lx1;
            up_axis(rs, min(x0 + k, H - 1), side, xa, xb, lx0, lx1);
            const float top = lx0 * ra[xa] + lx1 * ra[xb];
            const float bot = lx0 * rb[xa] + lx1 * rb[xb];
            const float v = ly0 * top + ly1 * bot;
            acc[k] += v;
        }
    }
    if (VEC) {
        *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x0 + k < H) o[k] = acc[k];
    }
}

}  // namespace

extern "C" int mgf_lpips_upsample_sum_f32(float* out, const float* const* maps, const int32_t* sides, int32_t ntaps, int32_t n, int32_t H,
                                          int32_t accumulate, mgf_stream_t stream) {
    MGF_REQUIRE(out && maps && sides && ntaps >= 1 && ntaps <= 8 && n >= 1 && n <= 65535 && H >= 1 && H <= 65535, MGF_EINVAL,
                "lpips_upsample_sum: bad arguments (1..8 taps, n and H in 1..65535)");
    UpTaps t;
    for (int l = 0; l < 8; ++l) {
        const bool on = l < ntaps;
        MGF_REQUIRE(!on || (maps[l] && sides[l] >= 1 && sides[l] <= 32768), MGF_EINVAL, "lpips_upsample_sum: tap %d: bad map or side", l);
        t.map[l] = on ? maps[l] : nullptr;
        t.side[l] = on ? sides[l] : 1;
        // torch keeps the scale factor it was given: the source step is 1 / (H / side), rounded to float (UpSample.h compute_scales_value)
        t.rscale[l] = on ? (float)(1.0 / ((double)H / (double)sides[l])) : 0.f;
    }
    const dim3 grid((unsigned)mgf_cdiv(mgf_cdiv(H, 4), 256), (unsigned)H, (unsigned)n);
    if (H % 4 == 0 && ((uintptr_t)out & 15) == 0)
        hipLaunchKernelGGL(lpips_upsample_sum_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, out, t, ntaps, H, accumulate);
    else
        hipLaunchKernelGGL(lpips_upsample_sum_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, out, t, ntaps, H, accumulate);
    MGF_CHECK_LAUNCH("lpips_upsample_sum");
    return MGF_OK;
}

extern "C" int mgf_wing_loss_f64(double* out, const double* pred, const double* target, int32_t n, int64_t numel, double omega,
                                 double epsilon, const int32_t* pred_step, int32_t max_row, mgf_stream_t stream) {
    MGF_REQUIRE(out && pred && target && numel >= 1 && n >= 1, MGF_EINVAL, "wing_loss: bad arguments");
    hipLaunchKernelGGL(wing_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, out, pred, target, numel, omega, epsilon, pred_step, max_row);
    MGF_CHECK_LAUNCH("wing_loss");
    return MGF_OK;
}

extern "C" int mgf_adaptive_wing_loss_f64(double* out, const double* pred, const double* target, int32_t n, int64_t numel, double omega,
                                          double theta, double epsilon, double alpha, const int32_t* pred_step, int32_t max_row,
                                          mgf_stream_t stream) {
    MGF_REQUIRE(out && pred && target && numel >= 1 && n >= 1, MGF_EINVAL, "adaptive_wing_loss: bad arguments");
    hipLaunchKernelGGL(awing_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, out, pred, target, numel, omega, theta, epsilon, alpha,
                       pred_step, max_row);
    MGF_CHECK_LAUNCH("adaptive_wing_loss");
    return MGF_OK;
}
