// Stride-2 3x3 transposed convolution in polyphase Winograd form.  Contract: include/mgf.h (mgf_tconv3x3s2_winograd_f32,
// mgf_tconv_winograd_weights_f32).  Same arithmetic role as the tconv launch of conv_taps.hip (conv_transpose2d on the un-flipped
// weights, t[2i+kh, 2j+kw] += w[kh,kw] x[i,j]; training/networks.py:288-303 with up = 2), same [n, cout, 2h+1, pitch] workspace.
//
// Per dimension, one input pair x[p], x[p+1] (p even) with its left neighbour gives the four outputs t[2p .. 2p+3]; with
// d0, d1, d2 = x[p-1], x[p], x[p+1]:
//   t[2p] = w2 d0 + w0 d1,  t[2p+2] = w2 d1 + w0 d2   (even outputs: F(2,2) = three products)
//   t[2p+1] = w1 d1,        t[2p+3] = w1 d2           (odd outputs: the tap itself)
// i.e. five products m_r = D_r * W_r with data rows D = (d0 - d1, d1, d2 - d1, d1, d2) and weight rows W = (w2, w0 + w2, w0, w1, w1), and
//   t[2p] = m1 + m2,  t[2p+1] = m4,  t[2p+2] = m2 + m3,  t[2p+3] = m5.
// In 2D the outer product gives 25 products per 2x2 input block (a 4x4 output block) where the direct form needs 36: 0.69 of the
// matrix work.  Every product is a GEMM over the input channels: M_rc[co][tile] = sum_ci U_rc[co][ci] V_rc[ci][tile].
//
// The kernel is built like form 3 (wino3.hip): 4 waves, one 32x32 block (32 output channels x 32 input blocks = 64 x 8 outputs) per
// position; the transformed input goes from VALU registers straight into the MFMA B operand; the weight operand (A) comes from L2 one
// chunk ahead; the style modulation rides on the input when it is parked in LDS, the demodulation on the output.
// The 25 positions are dealt 6 + 6 + 6 + 6 + 1: wave a owns product row a + 1 (positions (a+1, 1..5)) and (5, a+1); the last product
// (5, 5) is split by k-step over the four waves -- waves 0 / 1 take its two k-steps in even chunks, waves 2 / 3 in odd ones -- and its
// four partial sums meet in the output transform.  Per chunk of 4 channels a wave thus issues 12 or 13 MFMAs (12.5 on average, every
// SIMD the same), 7 x 16 accumulators.
// The output transform is additions: each wave reduces its row over the columns, the rows meet once through LDS, and wave w writes
// output row (0, 2, 3, 1)[w] of every 4x4 block -- four consecutive floats of a row per channel, one 16-byte store.
// Row and column 2h / 2w of the workspace are not written here (mgf_tconv3x3s2_border_f32).
#include "mgf_common.h"
#include <algorithm>
#include <type_traits>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int WTCK = 4;                    // input channels per chunk
constexpr int WTFW = 34;                   // footprint width: 16 blocks x 2 + 1 left neighbour (+ 1 pad)
constexpr int WTFH = 5;                    // footprint rows: 2 block rows x 2 + 1 upper neighbour
constexpr int WTFP = WTFH * WTFW;          // 170 pixels: one staging slot per lane and channel
constexpr int WTNP = 25;                   // positions
constexpr int WTXS = 14;                   // exchange slots of the output transform ([16 values][64 lanes] each)
__constant__ float wt_ones[WTCK] = {1.f, 1.f, 1.f, 1.f};

struct WinoTParams {
    float* t;                 // [n][cout][2h+1][pitch]
    const float* x;           // [n][cin][h][w]
    const float* u;           // [25][cin / 4][cout][4 slots] (mgf_tconv_winograd_weights_f32)
    const float* in_scale;    // [n][cin] or null
    const float* out_scale;   // [n or 1][cout] (row stride os_stride) or null
    int n, cin, h, w, cout, os_stride, pitch;
    int tiles_x, tiles_y, co_tiles;
    int xcd_per;              // > 0: XCD-contiguous work order (as form 3)
    int64_t t_plane, t_batch; // elements between channels / samples of t
};

__global__ __launch_bounds__(256, 2) void wino_tconv_kernel(WinoTParams p) {
    constexpr int CST = 256, RAW = WTCK * CST;
    extern __shared__ float lds[];
    float* const raw0 = lds;
    float* const raw1 = raw0 + RAW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int a = __builtin_amdgcn_readfirstlane(tid >> 6);        // wave = product row a + 1 (wave-uniform)
    const int l31 = lane & 31, half = lane >> 5;
    const int tx = l31 & 15, ty = l31 >> 4;                         // input block (2 ty, 2 tx) of the tile

    int b_ = blockIdx.x;
    if (p.xcd_per > 0) {
        b_ = (b_ & 7) * p.xcd_per + (b_ >> 3);
        if (b_ >= p.n * p.tiles_x * p.tiles_y * p.co_tiles) return;
    }
    const int cot = b_ % p.co_tiles; b_ /= p.co_tiles;
    const int ptx = b_ % p.tiles_x; b_ /= p.tiles_x;
    const int pty = b_ % p.tiles_y;
    const int n = b_ / p.tiles_y;
    const int co0 = cot * 32, iy0 = pty * 4, ix0 = ptx * 32;
    const int plane = p.h * p.w;
    const float* xn = p.x + (int64_t)n * p.cin * plane;
    const float* sc = p.in_scale ? p.in_scale + (int64_t)n * p.cin : nullptr;
    const int nck = p.cin / WTCK;

    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)xn, 0, p.cin * plane * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc((void*)p.u, 0, WTNP * p.cin * p.cout * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rnull = __builtin_amdgcn_make_buffer_rsrc((void*)p.u, 0, 0, 0x00020000);   // tail loads: zeros, no branch
    // staging slot of lane tid: footprint pixel tid (rows iy0 - 1 .. iy0 + 3, columns ix0 - 1 .. ix0 + 32); outside the map = zero padding
    unsigned xoff;
    {
        const int r = tid / WTFW, q = tid - r * WTFW;
        const int iy = iy0 - 1 + r, ix = ix0 - 1 + q;
        xoff = (tid < WTFP && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w) ? (unsigned)(iy * p.w + ix) * 4u : 0xFFFFFFF0u;
    }
    // A operand of lane (l31, half): 8 bytes = slots {2 half, 2 half + 1} = channels {half, half + 2} of output channel co0 + l31
    const unsigned aoff = (unsigned)(((co0 + l31) * WTCK + half * 2) * 4);
    const int upos = nck * p.cout * WTCK * 4;                      // bytes between two positions
    // the wave's positions: (a+1, 1..5) = 5a .. 5a + 4, (5, a+1) = 20 + a; the shared one (5, 5) = 24, of which this wave reads the
    // single slot of its k-step (a & 1): channel half + 2 (a & 1)
    const int ubase_row = 5 * a * upos, ubase_col = (20 + a) * upos, ubase_sh = 24 * upos + (a & 1) * 4;

    float xr[WTCK];
    auto load_x = [&](float (&dst)[WTCK], int c0, bool live = true) {
        const __amdgpu_buffer_rsrc_t r = live ? rx : rnull;
#pragma unroll
        for (int j = 0; j < WTCK; ++j) dst[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, xoff, (c0 + j) * plane * 4, 0));
    };
    typedef const float __attribute__((address_space(4)))* cfp4;
    const cfp4 sbase = sc ? (cfp4)sc : (cfp4)wt_ones;
    const int sstep = sc ? 1 : 0;
    auto load_s = [&](float (&dst)[WTCK], int c0) {
#pragma unroll
        for (int j = 0; j < WTCK; ++j) dst[j] = sbase[c0 * sstep + j];
    };
    auto park_x = [&](float* R, const float (&src)[WTCK], const float (&sv)[WTCK]) {
#pragma unroll
        for (int j = 0; j < WTCK; ++j) R[j * CST + tid] = src[j] * sv[j];
    };
    struct Aop { v2f q[6]; float s; };
    auto load_a = [&](Aop& dst, int c0, bool live = true) {
        const int soff = c0 * p.cout * 4;
        const __amdgpu_buffer_rsrc_t r = live ? ru : rnull;
#pragma unroll
        for (int b = 0; b < 5; ++b)
            dst.q[b] = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(r, aoff, ubase_row + b * upos + soff, 0));
        dst.q[5] = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(r, aoff, ubase_col + soff, 0));
        dst.s = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, aoff, ubase_sh + soff, 0));
    };
    // transformed input of this lane's (block, channel half + 2 kk): the wave's data row e = P[pr] + sg P[qr] over the patch's three
    // columns, then its column values (e0 - e1, e1, e2 - e1, e2); the last patch row f = P[2] gives (5, a+1) = f[px] + sgf f[1] and (5, 5) = f2
    const int pr = a == 0 ? 0 : (a == 2 ? 2 : 1);
    const float sg = (a == 0 || a == 2) ? -1.f : 0.f;
    const int px = a == 0 ? 0 : (a == 2 ? 2 : 1);
    const float sgf = (a == 0 || a == 2) ? -1.f : 0.f;
    auto transform = [&](float (&B)[2][6], const float* R) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const float* src = R + (half + 2 * kk) * CST + 2 * ty * WTFW + 2 * tx;
            const float* rp = src + pr * WTFW;
            const float* r1 = src + WTFW;
            const float* r2 = src + 2 * WTFW;
            const v2f p01 = *reinterpret_cast<const v2f*>(rp), q01 = *reinterpret_cast<const v2f*>(r1), f01 = *reinterpret_cast<const v2f*>(r2);
            const float p2 = rp[2], q2 = r1[2], f2 = r2[2];
            const v2f sg2 = {sg, sg};
            const v2f e01 = p01 + sg2 * q01;
            const float e2 = p2 + sg * q2;
            B[kk][0] = e01.x - e01.y;
            B[kk][1] = e01.y;
            B[kk][2] = e2 - e01.y;
            B[kk][3] = e2;
            const float fp = px == 0 ? f01.x : (px == 2 ? f2 : f01.y);
            B[kk][4] = fp + sgf * f01.y;
            B[kk][5] = f2;
        }
    };

    // acc[0..4]: positions (a+1, 1..5); acc[5]: (5, a+1); accs: this wave's share of (5, 5)
    f32x16 acc[6];
    f32x16 accs = {};
    constexpr int BI[5] = {0, 1, 2, 1, 3};                         // column c -> value of the transformed row
    auto mfma_chunk = [&](const Aop& A, const float (&B)[2][6], auto first_tag, auto parity_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;
        constexpr int PAR = decltype(parity_tag)::value;
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const int bi = b < 5 ? BI[b] : 4;
            acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.q[b].x, B[0][bi], FIRST ? f32x16{} : acc[b], 0, 0, 0);
            acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.q[b].y, B[1][bi], acc[b], 0, 0, 0);
        }
        if ((a >> 1) == PAR) {                                     // (wave-uniform) this chunk's k-step of (5, 5)
            const float bs = (a & 1) ? B[1][5] : B[0][5];
            accs = __builtin_amdgcn_mfma_f32_32x32x2f32(A.s, bs, accs, 0, 0, 0);
        }
    };

    const int nchunks = nck;
    const int last = nchunks - 1;
    auto chunk0 = [&](int i) { return (i < last ? i : last) * WTCK; };
    Aop A0, A1;
    float B0[2][6], B1[2][6];
    float sv[WTCK];
    {
        float xa[WTCK], xb[WTCK], sa_[WTCK], sb_[WTCK];
        load_s(sv, chunk0(2));
        load_x(xa, 0);
        load_a(A0, 0);
        load_x(xb, chunk0(1));
        load_x(xr, chunk0(2));
        load_s(sa_, 0);
        load_s(sb_, chunk0(1));
        park_x(raw0, xa, sa_);
        park_x(raw1, xb, sb_);
        __syncthreads();
        transform(B0, raw0);
        __syncthreads();
    }
    // body(i): request A(i+1); transform chunk i+1 (parked during body(i-1)); the MFMAs of chunk i; park x(i+2) over chunk i's
    // footprint; request x(i+3) -- form 3's one-block pipeline
    auto body = [&](int i, Aop& Acur, Aop& Anxt, float (&Bcur)[2][6], float (&Bnxt)[2][6], float* raw_nxt, float* raw_park, auto first_tag,
                    auto parity_tag) {
        load_a(Anxt, chunk0(i + 1), i + 1 < nchunks);
        __builtin_amdgcn_sched_barrier(0);
        transform(Bnxt, raw_nxt);
        mfma_chunk(Acur, Bcur, first_tag, parity_tag);
        __builtin_amdgcn_sched_barrier(0);
        park_x(raw_park, xr, sv);
        load_x(xr, chunk0(i + 3), i + 3 < nchunks);
        load_s(sv, chunk0(i + 3));
        __syncthreads();
    };
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    body(0, A0, A1, B0, B1, raw1, raw0, std::true_type{}, P0{});
    if (1 < nchunks) body(1, A1, A0, B1, B0, raw0, raw1, std::false_type{}, P1{});
    for (int it = 2; it < nchunks; it += 2) {
        body(it, A0, A1, B0, B1, raw1, raw0, std::false_type{}, P0{});
        if (it + 1 < nchunks) body(it + 1, A1, A0, B1, B0, raw0, raw1, std::false_type{}, P1{});
    }

    // ---- output transform.  Own row over the columns: R0 = M1 + M2, R1 = M4, R2 = M2 + M3, R3 = M5 (per accumulator register).
    // Over the rows: Y0 = R[1] + R[2] (wave 0), Y2 = R[2] + R[3] (wave 1), Y1 = R[4] (wave 3), Y3 = R[5] (wave 2) with
    // R[5] = (M51 + M52, M54, M52 + M53, M55).  Exchange slots [16][64]: 0-3 R[2] (wave 1), 4-7 R[3] (wave 2), 8 M51, 9 its share of
    // M55 (wave 0), 10 M52, 11 share (wave 1), 12 M54, 13 share (wave 3). ----
    float R[4][16];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        R[0][v] = acc[0][v] + acc[1][v];
        R[1][v] = acc[3][v];
        R[2][v] = acc[1][v] + acc[2][v];
        R[3][v] = acc[4][v];
    }
    float* const xch = lds;                                        // the staging buffers are dead (every wave passed the last barrier)
    auto put = [&](int slot, const float* vals) {
        float* dst = xch + slot * 1024 + lane;
#pragma unroll
        for (int v = 0; v < 16; ++v) dst[v * 64] = vals[v];
    };
    float colv[16], shv[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) { colv[v] = acc[5][v]; shv[v] = accs[v]; }
    if (a == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) put(j, R[j]);
        put(10, colv);
        put(11, shv);
    } else if (a == 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) put(4 + j, R[j]);
    } else if (a == 0) {
        put(8, colv);
        put(9, shv);
    } else {
        put(12, colv);
        put(13, shv);
    }
    __syncthreads();
    const float* xl = xch + lane;
    float Y[4][16];
    if (a == 0 || a == 1) {
        const int s0 = a == 0 ? 0 : 4;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) Y[j][v] = R[j][v] + xl[(s0 + j) * 1024 + v * 64];
    } else if (a == 2) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const float m51 = xl[8 * 1024 + v * 64], m52 = xl[10 * 1024 + v * 64], m54 = xl[12 * 1024 + v * 64];
            Y[0][v] = m51 + m52;
            Y[1][v] = m54;
            Y[2][v] = m52 + colv[v];
            Y[3][v] = (xl[9 * 1024 + v * 64] + xl[11 * 1024 + v * 64]) + (shv[v] + xl[13 * 1024 + v * 64]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) Y[j][v] = R[j][v];
    }
    // output row i = (0, 2, 3, 1)[a] of the block: t row 2 (iy0 + 2 ty) + i, columns 2 (ix0 + 2 tx) .. + 3 of channel
    // co0 + 4 half + (v & 3) + 8 (v >> 2)
    const int orow = a == 0 ? 0 : (a == 1 ? 2 : (a == 2 ? 3 : 1));
    const int by = iy0 + 2 * ty, bx = ix0 + 2 * tx;
    const bool ok = by < p.h && bx < p.w;                          // h, w even: a block inside the map is whole
    const int cob = co0 + 4 * half;
    const float* osc = p.out_scale ? p.out_scale + (int64_t)n * p.os_stride + cob : nullptr;
    const unsigned toff = ok ? (unsigned)(((int64_t)cob * p.t_plane + (int64_t)(2 * by + orow) * p.pitch + 2 * bx) * 4) : 0xFFFFFFF0u;
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc((void*)(p.t + (int64_t)n * p.t_batch), 0,
                                                                       (int)((int64_t)p.cout * p.t_plane * 4), 0x00020000);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int cl = (v & 3) + 8 * (v >> 2);
        const float s = osc ? osc[cl] : 1.f;
        const v4u o = {__builtin_bit_cast(unsigned, Y[0][v] * s), __builtin_bit_cast(unsigned, Y[1][v] * s),
                       __builtin_bit_cast(unsigned, Y[2][v] * s), __builtin_bit_cast(unsigned, Y[3][v] * s)};
        __builtin_amdgcn_raw_buffer_store_b128(o, rt, toff, (int)(cl * p.t_plane * 4), 0);
    }
}

// U[5 (r-1) + (c-1)][ci / 4][co][slot] = gain * (T w T^T)[r][c], T = [[0,0,1],[1,0,1],[1,0,0],[0,1,0],[0,1,0]] (rows: w2, w0 + w2, w0,
// w1, w1), from w [cout][cin][3][3]; float64 sums, one rounding; the 4 channels of a chunk in MFMA slot order (as form 3)
__global__ __launch_bounds__(256) void wino_tconv_weights_kernel(float* u, const float* w, int cout, int cin, double gain) {
    const int64_t total = (int64_t)cout * cin;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int co = (int)(i % cout), ci = (int)(i / cout);
        const float* g = w + ((int64_t)co * cin + ci) * 9;
        double t[5][3];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const double g0 = g[v], g1 = g[3 + v], g2 = g[6 + v];
            t[0][v] = g2;
            t[1][v] = g0 + g2;
            t[2][v] = g0;
            t[3][v] = g1;
            t[4][v] = g1;
        }
        const int cl = ci & 3, slot = 2 * (cl & 1) + (cl >> 1);
        const int64_t pl = (int64_t)cin * cout;
        float* dst = u + (((int64_t)(ci >> 2)) * cout + co) * 4 + slot;
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const double o[5] = {t[r][2], t[r][0] + t[r][2], t[r][0], t[r][1], t[r][1]};
#pragma unroll
            for (int c = 0; c < 5; ++c) dst[(5 * r + c) * pl] = (float)(o[c] * gain);
        }
    }
}

}  // namespace

extern "C" int mgf_tconv_winograd_weights_f32(float* u, const float* w, int32_t cout, int32_t cin, double gain, mgf_stream_t stream) {
    MGF_REQUIRE(u && w && cout >= 1 && cin >= 1, MGF_EINVAL, "tconv_winograd_weights: bad arguments");
    MGF_REQUIRE(cin % WTCK == 0, MGF_EUNSUPPORTED, "tconv_winograd_weights: cin must be a multiple of %d (got %d)", WTCK, cin);
    hipLaunchKernelGGL(wino_tconv_weights_kernel, dim3(mgf_stream_grid((int64_t)cout * cin, 256, 1)), dim3(256), 0, (hipStream_t)stream, u, w, cout,
                       cin, gain);
    MGF_CHECK_LAUNCH("tconv_winograd_weights");
    return MGF_OK;
}

extern "C" int mgf_tconv3x3s2_winograd_f32(float* t, const float* x, const float* u, const float* in_scale, const float* out_scale, int32_t n,
                                           int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t pitch, int64_t t_plane, int64_t t_batch,
                                           int64_t out_scale_stride, mgf_stream_t stream) {
    MGF_REQUIRE(t && x && u && n >= 1 && cin >= 1 && cout >= 1 && h >= 2 && w >= 2, MGF_EINVAL, "tconv3x3s2_winograd: bad arguments");
    MGF_REQUIRE(cin % WTCK == 0 && cout % 32 == 0, MGF_EUNSUPPORTED, "tconv3x3s2_winograd: cin must be a multiple of %d and cout of 32 (got %d, %d)",
                WTCK, cin, cout);
    MGF_REQUIRE(h % 2 == 0 && w % 2 == 0, MGF_EUNSUPPORTED, "tconv3x3s2_winograd: even map sides only (got %dx%d)", h, w);
    MGF_REQUIRE(pitch >= 2 * w + 1 && pitch % 4 == 0 && t_plane >= (int64_t)(2 * h + 1) * pitch && t_plane % 4 == 0 && t_batch % 4 == 0 &&
                    t_batch >= (int64_t)cout * t_plane, MGF_EINVAL, "tconv3x3s2_winograd: bad workspace layout");
    MGF_REQUIRE(((uintptr_t)t % 16) == 0 && ((uintptr_t)u % 16) == 0, MGF_EINVAL, "tconv3x3s2_winograd: t and u must be 16-byte aligned");
    MGF_REQUIRE((int64_t)cin * h * w <= INT32_MAX / 4 && (int64_t)WTNP * cin * cout <= INT32_MAX / 4 && (int64_t)cout * t_plane <= INT32_MAX / 4,
                MGF_ETOOBIG, "tconv3x3s2_winograd: one sample / the weight planes must stay below 2 GiB (32-bit buffer offsets)");
    WinoTParams p{};
    p.t = t; p.x = x; p.u = u; p.in_scale = in_scale; p.out_scale = out_scale;
    p.n = n; p.cin = cin; p.h = h; p.w = w; p.cout = cout; p.os_stride = (int)out_scale_stride; p.pitch = pitch;
    p.t_plane = t_plane; p.t_batch = t_batch;
    p.tiles_x = (int)mgf_cdiv(w, 32);
    p.tiles_y = (int)mgf_cdiv(h, 4);
    p.co_tiles = cout / 32;
    int64_t blocks = (int64_t)n * p.tiles_x * p.tiles_y * p.co_tiles;
    MGF_REQUIRE(blocks <= INT32_MAX - 8, MGF_ETOOBIG, "tconv3x3s2_winograd: too many workgroups");
    p.xcd_per = 0;
    // XCD-contiguous order where the transformed weights fit one XCD's 4 MB L2 (as form 3)
    if ((int64_t)WTNP * cin * cout * 4 <= (4 << 20) && blocks >= 16) {
        p.xcd_per = (int)((blocks + 7) / 8);
        blocks = (int64_t)p.xcd_per * 8;
    }
    const size_t lds = std::max<size_t>((size_t)2 * WTCK * 256, (size_t)WTXS * 16 * 64) * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)wino_tconv_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
        if (e != hipSuccess) { mgf_set_error("tconv3x3s2_winograd: cannot raise dynamic LDS: %s", hipGetErrorString(e)); return MGF_ELAUNCH; }
        attr_set = true;
    }
    // algorithmic accounting of the direct form (what the launch replaces: 9 taps per input pixel)
    mgf_prof_external_begin((hipStream_t)stream, "wino_tconv_kernel", 2.0 * 9 * cin * (double)cout * h * w * n,
                            4.0 * ((double)n * cin * h * w + 9.0 * cin * cout + (double)n * cout * 4.0 * h * w));
    hipLaunchKernelGGL(wino_tconv_kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, p);
    mgf_prof_external_end((hipStream_t)stream);
    MGF_CHECK_LAUNCH("tconv3x3s2_winograd");
    return MGF_OK;
}
