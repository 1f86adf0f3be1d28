// Winograd F(2x2, 3x3), third kernel form: the transformed input never touches LDS.
// Contract: include/mgf.h (mgf_conv3x3_winograd3_f32 / _rgb_f32); weights in the layout of mgf_winograd2_weights_f32.
// Same arithmetic role as wino.hip (modulated 3x3 / stride-1 / pad-1 convolution, training/networks.py:288-303).
//
// What bounds a Winograd kernel on gfx950's FP32 matrix cores (tools/probes/mfma_lds.hip, mfma_coexec.hip): v_mfma_f32_32x32x2_f32
// holds its SIMD for 64 cycles and NOTHING else of that SIMD overlaps with it to speak of -- a VALU instruction costs ~4 cycles of
// matrix time (2 with two waves per SIMD), an LDS store ~8 cycles PER DWORD whatever its width (4 CU-wide cycles: the VGPR -> LDS path
// is shared by the CU), while LDS loads of up to four per MFMA are free.  Form 2 (wino.hip) stores 30 dwords per lane and chunk to LDS
// (input footprint 6, modulated weights 8, transformed input 16) and issues ~40 VALU instructions for 16 MFMAs.  This form:
//   * splits the 16 Winograd positions of a tile FOUR ways, by row `a` of the transformed patch, one row per wave.  Row a of B^T d B
//     needs two rows of the patch (a=0: d0-d2, 1: d1+d2, 2: d2-d1, 3: d1-d3) and 8 additions per (tile, channel), and a lane computes
//     exactly the values its own MFMA B-operand slots hold -- (tile = lane % 32, channels {half, half + 2} of the chunk) -- so the
//     transformed input goes from VALU registers straight into the MFMAs: no LDS store, no LDS buffer, no second barrier phase;
//   * reads the weight operand (A) for its 4 positions straight from L2 into registers (one 8-byte buffer load per position and
//     32-channel block: the two k-steps of a chunk), one chunk ahead: no LDS staging of weights either;
//   * folds the style modulation into the INPUT when the footprint is parked in LDS (x * s, 4-6 multiplies per lane and chunk,
//     instead of scaling the 16/9-times larger transformed weight slab): sum_i (W_oi s_i) * x_i = sum_i W_oi * (s_i x_i).
// Per lane and chunk of 4 input channels that leaves 4-6 LDS dword stores, 16-38 VALU instructions, 8-16 LDS reads and 16 MFMAs.
//
// Workgroup: 4 waves (wave = row a), 4 positions x NB blocks of 32x32 accumulators per wave.
//   <CB=2, TB=1>: 64 output channels x 32 tiles (16 x 2 Winograd tiles = 32 x 4 outputs), 128 accumulators, 2 workgroups per CU
//                 -- layers deep enough in K (>= 128 input channels) to be bound by the matrix pipe
//   <CB=1, TB=2>: 32 output channels x 64 tiles (32 x 8 outputs), 128 accumulators
//   <CB=1, TB=1>: 32 output channels x 32 tiles (32 x 4 outputs), 64 accumulators, 3 workgroups per CU, optional fused ToRGB
//                 -- the 512^2 / 1024^2 layers (8-16 chunks per workgroup): their time is the prologue / epilogue memory latency of a
//                 workgroup, which more resident workgroups hide
// The four rows meet once, at the end: Y = A^T M A is linear in M, every wave reduces its row to R[a][j] (2 values per accumulator
// register), the rows are exchanged through LDS so that wave w finishes output row (w >> 1) of block (w & 1).
#include "mgf_common.h"
#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float v2f __attribute__((ext_vector_type(2)));

struct Wino3Params {
    float* y;
    const float* x;
    const float* u;           // [16][cin / 4][cout][4 slots] (mgf_winograd2_weights_f32)
    const float* in_scale;    // [n][cin] or null
    const float* out_scale;   // [n or 1][cout] or null
    int n, cin, h, w, cout, os_stride;
    int tiles_x, tiles_y, co_tiles;
    int xcd_per;              // > 0: XCD-aware work order (see the kernel); 0: work item = blockIdx.x
    mgf_epilogue ep;
    int has_ep;
    const float* rgb_w;       // [n][rgb_channels][cout]
    const float* rgb_bias;    // [rgb_channels] or null
    float* rgb_out;           // [n][rgb_channels][h][w]
    int rgb_channels;
    const float* res_low;     // [n][cout][h/2][w/2] or null: the residual at HALF resolution, 2x up-sampled in the epilogue
    int64_t y_batch;          // elements between samples of y (y may be a channel slice of a wider concat buffer; residual likewise)
    int y_choff;              // channel offset into y
    int odd;                  // h or w odd: pixel pairs are stored / loaded element-wise with bounds checks
    int low_pieces;           // the half-resolution residual's rows are whole 16-byte pieces (one-shot kernel: three 16-byte DMAs per lane instead of nine 4-byte ones)
    int strip_len, strips_x;  // persistent form (wino3p_conv_kernel): tiles per workgroup, strips per tile row
    int vert, strips_y;       // ... vert: a strip walks DOWN a 32-pixel column (strips_x = tile columns, strips_y = strips per column)
    int mask_ring;            // masked variants (MASK = true): outputs outside ring mask_ring are 0, inside acc * (m > 0 ? 1 : mask_slope)
    float mask_slope;         // with m = ep.residual at the output (the MDF backward: the adjoint conv times LeakyReLU' of the stored activation)
};

#ifndef W3_OCC1
#define W3_OCC1 4                        // workgroups per CU the one-block shapes are compiled for (3 -> 4: conv_last + ToRGB 3.64 -> 3.26 ms)
#endif
constexpr int W3CK = 4;                    // input channels per chunk
constexpr int W3FW = 34;                   // footprint width: 16 tiles x 2 + 2
__constant__ float w3_ones[W3CK] = {1.f, 1.f, 1.f, 1.f};          // the "styles" of an un-modulated launch (read with stride 0)

// (MASK: the masked epilogue of the MDF backward -- see Wino3Params::mask_ring -- instead of the fused one)
template <int CB, int TB, bool RGB, bool MASK = false>
__global__ __launch_bounds__(256, (CB * TB == 2 ? 2 : W3_OCC1)) void wino3_conv_kernel(Wino3Params p) {
    static_assert(!MASK || (CB == 1 && TB == 1 && !RGB), "the masked epilogue is built for the one-block shape");
    constexpr int NB = CB * TB;                                    // 32x32 blocks per position and wave: 2 (128 accumulators) or 1 (64)
    static_assert(NB == 1 || NB == 2, "a wave carries one or two 32x32 blocks per position");
    constexpr int FH = 4 * TB + 2, FP = FH * W3FW;                 // footprint rows / pixels per channel
    constexpr int SPC = (FP + 255) / 256;                          // staging slots per lane and CHANNEL: 1 (TB = 1) or 2 (TB = 2)
    constexpr int XS = W3CK * SPC;                                 // staging slots per lane
    constexpr int CST = 256 * SPC;                                 // floats between the channels of a staging buffer
    constexpr int RAW = W3CK * CST;
    extern __shared__ float lds[];
    float* const raw0 = lds;
    float* const raw1 = raw0 + RAW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int a = __builtin_amdgcn_readfirstlane(tid >> 6);        // wave = row of the transformed patch (wave-uniform)
    const int l31 = lane & 31, half = lane >> 5;
    const int tx = l31 & 15, ty = l31 >> 4;

    // Work item -> (channel tile fastest, pixel tile, sample).  Workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share one),
    // each with its own L2.  With xcd_per > 0, XCD (b % 8) walks the CONTIGUOUS item range [(b % 8) * xcd_per, +xcd_per): all channel
    // tiles of a pixel tile -- which read the same input footprint -- and its neighbours run on one XCD, so the footprint comes from
    // fabric once instead of once per XCD.  Used when the layer's transformed weights (16 * cin * cout floats, then read by every
    // workgroup of the XCD) fit its 4 MB L2; for the 512-channel layers the plain order (two channel tiles per XCD) moves fewer bytes.
    int b_ = blockIdx.x;
    if (p.xcd_per > 0) {
        b_ = (b_ & 7) * p.xcd_per + (b_ >> 3);
        if (b_ >= p.n * p.tiles_x * p.tiles_y * p.co_tiles) return;
    }
    const int cot = b_ % p.co_tiles; b_ /= p.co_tiles;
    const int ptx = b_ % p.tiles_x; b_ /= p.tiles_x;
    const int pty = b_ % p.tiles_y;
    const int n = b_ / p.tiles_y;
    const int co0 = cot * 32 * CB, oy0 = pty * 4 * TB, ox0 = ptx * 32;
    const int plane = p.h * p.w;
    const float* xn = p.x + (int64_t)n * p.cin * plane;
    const float* sc = p.in_scale ? p.in_scale + (int64_t)n * p.cin : nullptr;
    const int nck = p.cin / W3CK;

    // raw BUFFER loads: scalar resource + 32-bit lane offset, out of range = 0 = the zero padding of the footprint
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)xn, 0, p.cin * plane * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc((void*)p.u, 0, 16 * p.cin * p.cout * 4, 0x00020000);
    // a resource of ZERO records: every access through it is out of range = returns 0 without touching memory.  The loop's tail
    // iterations load through it instead of branching around their loads: the instruction stream -- and with it the compiler's vmcnt
    // bookkeeping -- stays identical in every iteration (behind `if (more) load` the waits are merged conservatively over both paths
    // and drain the loads issued a moment ago, i.e. expose one L2 round trip per chunk)
    const __amdgpu_buffer_rsrc_t rnull = __builtin_amdgcn_make_buffer_rsrc((void*)p.u, 0, 0, 0x00020000);
    // A staging slot is ONE channel: slot j = channel j / SPC of the chunk, footprint pixel tid + 256 (j % SPC).  The pixel part of the
    // address is the same for all channels (one VGPR per pixel slot; the channel rides in the scalar offset -- the range check adds the two without
    // 32-bit wrap, so a pixel outside the map, marked by a sentinel vector offset, stays out of range) and the style of a slot is wave-uniform: a scalar load, no LDS table.
    unsigned xoff[SPC];
#pragma unroll
    for (int s = 0; s < SPC; ++s) {
        const int e = tid + 256 * s;
        const int r = e / W3FW, q = e - r * W3FW;
        const int iy = oy0 - 1 + r, ix = ox0 - 1 + q;
        xoff[s] = (e < FP && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w) ? (unsigned)(iy * p.w + ix) * 4u : 0xFFFFFFF0u;
    }
    // A operand of lane (l31, half) for position 4a + b, block cb: 8 bytes = slots {2 half, 2 half + 1} = channels {half, half + 2} of
    // output channel co0 + 32 cb + l31.  The position / chunk part of the address is wave-uniform and rides in the scalar offset.
    const unsigned aoff = (unsigned)(((co0 + l31) * W3CK + half * 2) * 4);
    const int upos = nck * p.cout * W3CK * 4;                      // bytes between two positions
    const int ubase = 4 * a * upos;

    float xr[XS];
    auto load_x = [&](float (&dst)[XS], int c0, bool live = true) {
        const __amdgpu_buffer_rsrc_t r = live ? rx : rnull;
#pragma unroll
        for (int j = 0; j < XS; ++j)
            dst[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, xoff[j % SPC], (c0 + j / SPC) * plane * 4, 0));
    };
    // (constant address space: the compiler then emits s_load for these uniform addresses -- through a generic pointer it falls back to
    // flat vector loads, which also poison the vmcnt bookkeeping; no branch in the loop: an un-modulated launch re-reads four ones)
    typedef const float __attribute__((address_space(4)))* cfp4;
    const cfp4 sbase = sc ? (cfp4)sc : (cfp4)w3_ones;
    const int sstep = sc ? 1 : 0;
    auto load_s = [&](float (&dst)[W3CK], int c0) {                // the chunk's styles (uniform addresses: scalar loads)
#pragma unroll
        for (int j = 0; j < W3CK; ++j) dst[j] = sbase[c0 * sstep + j];
    };
    auto park_x = [&](float* R, const float (&src)[XS], const float (&sv)[W3CK]) {
#pragma unroll
        for (int j = 0; j < XS; ++j) R[(j / SPC) * CST + tid + 256 * (j % SPC)] = src[j] * sv[j / SPC];      // the style modulation rides on the input
    };
    auto load_a = [&](v2f (&dst)[4][CB], int c0, bool live = true) {
        const int soff = ubase + c0 * p.cout * 4;                  // chunk c0 / 4 starts (c0 / 4) * cout * 4 floats into a position plane
        const __amdgpu_buffer_rsrc_t r = live ? ru : rnull;
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
                dst[b][cb] = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(r, aoff + cb * (32 * W3CK * 4), soff + b * upos, 0));
    };
    // row a of B^T d B for this lane's (tile, channel) pairs: t = d[pr] + sg * d[qr] over the 4 columns, then the row pass
    const int pr = a == 0 ? 0 : (a == 2 ? 2 : 1);
    const int qr = a == 2 ? 1 : (a == 3 ? 3 : 2);
    const float sg = a == 1 ? 1.f : -1.f;
    const v2f sg2 = {sg, sg}, pm = {-1.f, 1.f}, sgpm = {-sg, sg};
    auto transform = [&](float (&B)[TB][2][4], const float* R) {
#pragma unroll
        for (int tb = 0; tb < TB; ++tb)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const float* src = R + (half + 2 * kk) * CST + 2 * (tb * 2 + ty) * W3FW + 2 * tx;
                const v2f p01 = *reinterpret_cast<const v2f*>(src + pr * W3FW), p23 = *reinterpret_cast<const v2f*>(src + pr * W3FW + 2);
                const v2f q01 = *reinterpret_cast<const v2f*>(src + qr * W3FW), q23 = *reinterpret_cast<const v2f*>(src + qr * W3FW + 2);
                // PACKED fp32 (v_pk_fma_f32 / v_pk_add_f32: two lanes of math per issue slot), written so that every operand is a register
                // pair or a broadcast of one half of a pair (op_sel) -- 5 instructions for the 4 values instead of 8:
                //   t = p + sg q;  (B0, B1) = (t0 - t2, t1 + t2) = t01 + p2 (-1, 1) + q2 (-sg, sg);  (B2, -B3) = t23 - (t1, t1).
                // Position 3 of the row thus carries -B3, i.e. its accumulator -M3: the output transform below ADDS it.
                const v2f t01 = p01 + sg2 * q01, t23 = p23 + sg2 * q23;
                const v2f p2b = {p23.x, p23.x}, q2b = {q23.x, q23.x}, t1b = {t01.y, t01.y};
                const v2f b01 = q2b * sgpm + (p2b * pm + t01);
                const v2f b23 = t23 - t1b;
                B[tb][kk][0] = b01.x;
                B[tb][kk][1] = b01.y;
                B[tb][kk][2] = b23.x;
                B[tb][kk][3] = b23.y;
            }
    };

    // (never cleared: the first chunk's MFMAs take the constant 0 as their C operand -- 64 * CB * TB v_mov per workgroup cost as much matrix
    // time as 4 * CB * TB MFMAs, i.e. 6 % of an 8-chunk layer and 12 % of the 2-chunk Fire layers)
    f32x16 acc[4][CB][TB];
    auto mfma_chunk = [&](const v2f (&A)[4][CB], const float (&B)[TB][2][4], auto first_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                for (int tb = 0; tb < TB; ++tb) {
                    acc[b][cb][tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[b][cb].x, B[tb][0][b], FIRST ? f32x16{} : acc[b][cb][tb], 0, 0, 0);
                    acc[b][cb][tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[b][cb].y, B[tb][1][b], acc[b][cb][tb], 0, 0, 0);
                }
    };

    // ---- prologue: every load of chunks 0..2 is in flight before the first wait ----
    const int nchunks = nck;
    const int last = nchunks - 1;
    auto chunk0 = [&](int i) { return (i < last ? i : last) * W3CK; };
    v2f A0[4][CB], A1[4][CB];
    float B0[TB][2][4], B1[TB][2][4];
    float sv[W3CK];                                  // styles of the chunk parked next (scalar registers)
    // Epilogue operands of the one-block shape -- the half-resolution residual window, the noise rows, the demodulation and bias of the 32
    // channels -- are requested NOW, as LDS-DMA loads (buffer_load ... lds: no register holds them across the main loop) into LDS
    // behind the exchange slots, which the staging buffers do not reach: the epilogue then has no global load between the last MFMA and
    // its stores (it used to request them there and sit out an HBM round trip per workgroup -- with four workgroups per CU the kernel is
    // bound by the length of a workgroup's dependency chain, not by any throughput).  Lane l of a wave writes LDS base + 4 l; out-of-range
    // lanes write zeros.  These are the oldest loads in flight, so the first ordinary wait below retires them too.
    constexpr int UMODE = NB == 2 ? 0 : (RGB ? 2 : 1);
    constexpr int NV = UMODE == 0 ? 32 : 16;         // values per lane and exchange slot
    // half-resolution residual window of the tile's 32 channels: as 16-byte pieces [32][4 rows][24 columns] -- low-resolution columns
    // (ox0 >> 1) - 4 .. + 19, the 18 the tile needs are columns 3 .. 20 of them; 768 pieces, three 16-byte DMAs per lane (round 6; the nine 4-byte
    // requests per lane before were 5 % of the 512^2 layer, profiles/r6_w3_oneshot_ablation.txt) -- where the low map's rows are whole pieces
    // (width a multiple of 4, 16-byte aligned base: a piece is then entirely inside the map or entirely outside), else element-wise [32][4][18]
    float* const lowt = lds + 6 * NV * 64;
    const bool low_pieces = p.low_pieces != 0;                     // (uniform; decided by the host: low map width a multiple of 4, 16-byte aligned base)
    const int low_ch = low_pieces ? 96 : 72, low_row = low_pieces ? 24 : 18, low_col = low_pieces ? 3 : 0;
    float* const nzs = lowt + (p.res_low ? 3072 : 0);    // [4 rows][64]: noise of the tile's rows (32 px used)
    float* const obs = nzs + 256;                    // [2][64]: out_scale, bias of the 32 channels
    const bool pre_ep = UMODE == 1 && !p.odd;        // (uniform)
    if (pre_ep) {
        if (p.res_low) {
            const int hl = p.h >> 1, wl = p.w >> 1, pl = hl * wl;
            const __amdgpu_buffer_rsrc_t rlow = __builtin_amdgcn_make_buffer_rsrc((void*)(p.res_low + ((int64_t)n * p.cout + co0) * pl), 0, 32 * pl * 4, 0x00020000);
            const int m0 = (oy0 >> 1) - 1;
            if (low_pieces) {
                const int n0 = (ox0 >> 1) - 4;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int e = tid + 256 * j;                         // piece: channel e / 24, row (e % 24) / 6, columns 4 c .. 4 c + 3
                    const int ch = e / 24, rem = e - ch * 24;
                    const int r = rem / 6, c = rem - r * 6;
                    const int my = m0 + r, nx = n0 + 4 * c;
                    const unsigned off = (my >= 0 && my < hl && nx >= 0 && nx < wl) ? (unsigned)(ch * pl + my * wl + nx) * 4u : 0xFFFFFFF0u;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rlow, lowt + 4 * (256 * j + 64 * a), 16, off, 0, 0, 0);
                }
            } else {
                const int n0 = (ox0 >> 1) - 1;
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    const int e = tid + 256 * j;
                    const int ch = e / 72, rem = e - ch * 72;
                    const int r = rem / 18, c = rem - r * 18;
                    const int my = m0 + r, nx = n0 + c;
                    const unsigned off = (my >= 0 && my < hl && nx >= 0 && nx < wl) ? (unsigned)(ch * pl + my * wl + nx) * 4u : 0xFFFFFFF0u;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rlow, lowt + 256 * j + 64 * a, 4, off, 0, 0, 0);
                }
            }
        }
        if (p.has_ep && p.ep.noise) {                // wave a: row a of the tile, lanes 0..31 its 32 pixels
            const __amdgpu_buffer_rsrc_t rnz = __builtin_amdgcn_make_buffer_rsrc((void*)(p.ep.noise + (int64_t)(p.ep.noise_n > 1 ? n : 0) * plane), 0, plane * 4, 0x00020000);
            const int ny = oy0 + a, nx = ox0 + lane;
            const unsigned off = (lane < 32 && ny < p.h && nx < p.w) ? (unsigned)(ny * p.w + nx) * 4u : 0xFFFFFFF0u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rnz, nzs + 64 * a, 4, off, 0, 0, 0);
        }
        if (a < 2) {                                 // wave 0: out_scale, wave 1: bias (a null pointer gets a zero-size resource: zeros)
            const float* src = a == 0 ? (p.out_scale ? p.out_scale + (int64_t)n * p.os_stride + co0 : nullptr) : ((p.has_ep && p.ep.bias) ? p.ep.bias + co0 : nullptr);
            const __amdgpu_buffer_rsrc_t rob = __builtin_amdgcn_make_buffer_rsrc((void*)(src ? src : p.x), 0, src ? 32 * 4 : 0, 0x00020000);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rob, obs + 64 * a, 4, (unsigned)lane * 4u, 0, 0, 0);
        }
    }
    // (fused ToRGB: the projection weights times the demodulation, [3][32] behind the exchange slots, likewise fetched up front)
    float wv_pre = 0.f;
    if (RGB && tid < 96) {
        const int cc = tid >> 5, co = tid & 31;
        if (cc < p.rgb_channels)
            wv_pre = p.rgb_w[((int64_t)n * p.rgb_channels + cc) * p.cout + co0 + co] * (p.out_scale ? p.out_scale[(int64_t)n * p.os_stride + co0 + co] : 1.f);
    }
    // The two-block shapes (128 accumulators, TWO workgroups per CU: two waves per SIMD to cover a load's latency, and registers to spare)
    // request their operands one chunk EARLIER (round 6): weights two chunks ahead in a ring of three operand sets, the footprint two bodies
    // ahead in a ring of two -- 2516-2528 -> 2400-2413 us for the 256-channel 128^2 layer at 32 samples (tools/w3_layers_micro.py).  The
    // one-block shape sits at exactly 128 registers for its four workgroups per CU: the same ring there spills (2640 -> 2960-2990 us) or, compiled
    // for three workgroups, loses more residency than it gains distance (2640 -> 2690-2720 at 64^2, 3400 -> 3540-3570 at 512^2).
    constexpr bool DEEP = NB == 2;
    v2f A2[4][CB];
    float xr1[XS], sv1[W3CK];
    {
        float xa[XS], xb[XS], sa_[W3CK], sb_[W3CK];
        load_s(sv, chunk0(2));
        load_x(xa, 0);
        load_a(A0, 0);
        load_x(xb, chunk0(1));
        if constexpr (DEEP) load_a(A1, chunk0(1), 1 < nchunks);
        load_x(xr, chunk0(2));
        if constexpr (DEEP) {
            load_x(xr1, chunk0(3), 3 < nchunks);
            load_s(sv1, chunk0(3));
        }
        load_s(sa_, 0);
        load_s(sb_, chunk0(1));
        park_x(raw0, xa, sa_);
        park_x(raw1, xb, sb_);
        if (RGB && tid < 96) lowt[tid] = wv_pre;     // (= wvs of the epilogue)
        __syncthreads();
        transform(B0, raw0);
        __syncthreads();                             // body(0) parks chunk 2 over raw0: every wave must have read chunk 0 from it
    }
    // ---- steady state, one barrier per chunk.  body(i): request A(i+1); transform chunk i+1 (parked during body(i-1)) into the other
    // B registers; the 16 MFMAs of chunk i; park x(i+2) -- loaded during body(i-1) -- over chunk i's footprint (its transform is
    // done and every wave passed the barrier since); request x(i+3). ----
    auto body = [&](int i, v2f (&Acur)[4][CB], v2f (&Anxt)[4][CB], float (&Bcur)[TB][2][4], float (&Bnxt)[TB][2][4], float* raw_nxt, float* raw_park,
                    auto first_tag) {
        // ONE basic block: nothing here is conditional (past the last chunk the loads go through the null resource, the transform and
        // the parking work on values nobody reads)
        // the fences keep the order written here: left alone, the scheduler hoists the parking -- and with it the wait for x(i+2),
        // requested only one chunk ago -- in front of the MFMAs
        load_a(Anxt, chunk0(i + 1), i + 1 < nchunks);
        __builtin_amdgcn_sched_barrier(0);
        transform(Bnxt, raw_nxt);
        mfma_chunk(Acur, Bcur, first_tag);
        __builtin_amdgcn_sched_barrier(0);
        park_x(raw_park, xr, sv);
        load_x(xr, chunk0(i + 3), i + 3 < nchunks);
        load_s(sv, chunk0(i + 3));                   // (requested here, a whole chunk before their use: scalar loads share the LDS counter)
        __syncthreads();
    };
    // body2(i): the same with the deeper rings -- request A(i+2) into the set chunk i-1 used; park x(i+2) from ring slot i % 2, request x(i+4) into it
    auto body2 = [&](int i, v2f (&Acur)[4][CB], v2f (&Afar)[4][CB], float (&Bcur)[TB][2][4], float (&Bnxt)[TB][2][4], float* raw_nxt, float* raw_park,
                     float (&xq)[XS], float (&sq)[W3CK], auto first_tag) {
        load_a(Afar, chunk0(i + 2), i + 2 < nchunks);
        __builtin_amdgcn_sched_barrier(0);
        transform(Bnxt, raw_nxt);
        mfma_chunk(Acur, Bcur, first_tag);
        __builtin_amdgcn_sched_barrier(0);
        park_x(raw_park, xq, sq);
        load_x(xq, chunk0(i + 4), i + 4 < nchunks);
        load_s(sq, chunk0(i + 4));
        __syncthreads();
    };
    if constexpr (DEEP) {
        body2(0, A0, A2, B0, B1, raw1, raw0, xr, sv, std::true_type{});
        if (1 < nchunks) body2(1, A1, A0, B1, B0, raw0, raw1, xr1, sv1, std::false_type{});
        for (int it = 2; it < nchunks; it += 6) {        // (operand set = chunk % 3, B / staging buffer = chunk % 2: the pattern repeats every six)
            body2(it, A2, A1, B0, B1, raw1, raw0, xr, sv, std::false_type{});
            if (it + 1 < nchunks) body2(it + 1, A0, A2, B1, B0, raw0, raw1, xr1, sv1, std::false_type{});
            if (it + 2 < nchunks) body2(it + 2, A1, A0, B0, B1, raw1, raw0, xr, sv, std::false_type{});
            if (it + 3 < nchunks) body2(it + 3, A2, A1, B1, B0, raw0, raw1, xr1, sv1, std::false_type{});
            if (it + 4 < nchunks) body2(it + 4, A0, A2, B0, B1, raw1, raw0, xr, sv, std::false_type{});
            if (it + 5 < nchunks) body2(it + 5, A1, A0, B1, B0, raw0, raw1, xr1, sv1, std::false_type{});
        }
    } else {
        body(0, A0, A1, B0, B1, raw1, raw0, std::true_type{});
        if (1 < nchunks) body(1, A1, A0, B1, B0, raw0, raw1, std::false_type{});
        for (int it = 2; it < nchunks; it += 2) {
            body(it, A0, A1, B0, B1, raw1, raw0, std::false_type{});
            if (it + 1 < nchunks) body(it + 1, A1, A0, B1, B0, raw0, raw1, std::false_type{});
        }
    }

    // ---- output transform.  R[j] = row a of M times A: R0 = M0 + M1 + M2, R1 = M1 - M2 - M3 per accumulator register; then over the
    // rows (= waves): Y0 = R[0] + R[1] + R[2], Y1 = R[1] - R[2] - R[3].  The work is cut in two UNITS and wave w finishes output row
    // (w >> 1) of unit (w & 1):
    //   w0: Y0 u0 = own + s1 + s3     w1: Y0 u1 = s0 + own + s4     w2: Y1 u0 = s1 - own - s5     w3: Y1 u1 = s2 - s4 - own
    // with the exchange slots  s0 = R[0] u1, s1 = R[1] u0, s2 = R[1] u1, s3 = R[2] u0, s4 = R[2] u1, s5 = R[3] u0.
    // A unit is: one of the wave's two 32x32 blocks (NB = 2); a half of the block's 16 registers, i.e. 16 of its 32 channels (NB = 1);
    // or, for the fused ToRGB with one block, an output COLUMN j (the wave then holds one pixel of every quad for all 32 channels). ----
    float own[NV];
    float* xch = lds;                                // [6 slots][NV values][64 lanes]; the staging buffers are dead
    const int blk = a & 1, orow = a >> 1;
    {
        const int w0 = a == 1 ? 1 : (a == 2 ? 3 : (a == 3 ? 5 : -1));     // slot receiving my unit 0
        const int w1 = a == 0 ? 0 : (a == 1 ? 2 : (a == 2 ? 4 : -1));     // slot receiving my unit 1
        // (values first, then at most two wave-uniform branches: with the slot test around every store this was one basic block per value)
        float val[2][NV];
#pragma unroll
        for (int un = 0; un < 2; ++un)
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int r = UMODE == 0 ? (v >> 1) : (UMODE == 1 ? un * 8 + (v >> 1) : v);
                const int jj = UMODE == 2 ? un : (v & 1);
                const int cb = (UMODE == 0 && CB == 2) ? un : 0, tb = (UMODE == 0 && TB == 2) ? un : 0;
                const float m0 = acc[0][cb][tb][r], m1 = acc[1][cb][tb][r], m2 = acc[2][cb][tb][r], m3 = acc[3][cb][tb][r];
                val[un][v] = jj == 0 ? m0 + m1 + m2 : m1 - m2 + m3;        // (m3 = -M3, see transform)
            }
#pragma unroll
        for (int v = 0; v < NV; ++v) {               // own = unit `blk`, as a bit select (a ?: here becomes an indexed read of a stack array)
            const unsigned m = 0u - (unsigned)blk, b0 = __builtin_bit_cast(unsigned, val[0][v]), b1 = __builtin_bit_cast(unsigned, val[1][v]);
            own[v] = __builtin_bit_cast(float, (b1 & m) | (b0 & ~m));
        }
        if (w0 >= 0) {
            float* dst = xch + w0 * (NV * 64) + lane;
#pragma unroll
            for (int v = 0; v < NV; ++v) dst[v * 64] = val[0][v];
        }
        if (w1 >= 0) {
            float* dst = xch + w1 * (NV * 64) + lane;
#pragma unroll
            for (int v = 0; v < NV; ++v) dst[v * 64] = val[1][v];
        }
    }
    __builtin_amdgcn_sched_barrier(0);               // (the operand burst below must not move to where the accumulators are still live)
    // every global operand of the epilogue is requested here, in one burst in front of the exchange barrier
    const int trow = (UMODE == 0 && TB == 2 ? blk * 2 : 0) + ty;   // tile row inside the workgroup's tile
    const int oy = oy0 + 2 * trow + orow, ox = ox0 + 2 * tx + (UMODE == 2 ? blk : 0);
    const bool ok_px = oy < p.h && ox < p.w;         // h, w even: a pixel pair is inside whenever its first pixel is
    // channel of the wave's k-th channel row: cob + (k & 3) + 8 (k >> 2)
    const int cob = co0 + (UMODE == 0 && CB == 2 ? blk * 32 : 0) + (UMODE == 1 ? blk * 16 : 0) + 4 * half;
    const float* osc = p.out_scale ? p.out_scale + (int64_t)n * p.os_stride : nullptr;
    const bool do_ep = p.has_ep != 0;
    const int sa = a == 0 ? 1 : (a == 1 ? 0 : (a == 2 ? 1 : 2)), sb = a == 0 ? 3 : (a == 2 ? 5 : 4);
    const float sgn = a < 2 ? 1.f : -1.f;
    const float* pa = xch + sa * (NV * 64) + lane;
    const float* pb = xch + sb * (NV * 64) + lane;
    if (RGB) {
        // fused ToRGB: the wave holds, for all 32 channels (16 per lane half), row `orow` of its tiles' quads (UMODE 0: both columns)
        // or pixel (orow, blk) of them (UMODE 2).  The projection weights times the demodulation go through LDS once per workgroup.
        const int rc = p.rgb_channels;
        const float* wvs = lowt;                     // [3][32], written in the prologue
        __syncthreads();                             // the exchange slots are complete
        constexpr int NC = UMODE == 0 ? 2 : 1;       // output columns this wave produces
        float sum[3][NC];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
#pragma unroll
            for (int q = 0; q < NC; ++q) sum[cc][q] = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int k = UMODE == 0 ? (v >> 1) : v, q = UMODE == 0 ? (v & 1) : 0;
            const float yv = pa[v * 64] + sgn * (own[v] + pb[v * 64]);
            const int cl = 4 * half + (k & 3) + 8 * (k >> 2);
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) sum[cc][q] += yv * wvs[cc * 32 + cl];
        }
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
#pragma unroll
            for (int q = 0; q < NC; ++q) sum[cc][q] += __shfl_xor(sum[cc][q], 32, 64);
        if (half == 0 && ok_px) {
            for (int cc = 0; cc < rc; ++cc) {
                const float bb = p.rgb_bias ? p.rgb_bias[cc] : 0.f;
                float* o = p.rgb_out + ((int64_t)n * rc + cc) * plane + (int64_t)oy * p.w + ox;
                if (NC == 2) *reinterpret_cast<float2*>(o) = make_float2(sum[cc][0] + bb, sum[cc][NC - 1] + bb);
                else o[0] = sum[cc][0] + bb;
            }
        }
        return;
    }
    constexpr int NR = NV / 2;                       // channel rows this wave finishes (both columns of each)
    float osv[NR], bvv[NR];
    float2 rr[NR];
    float nz0 = 0.f, nz1 = 0.f;
#pragma unroll
    for (int k = 0; k < NR; ++k) { osv[k] = 1.f; bvv[k] = 0.f; rr[k] = make_float2(0.f, 0.f); }
    if (!pre_ep) {
        if (osc) {
#pragma unroll
            for (int k = 0; k < NR; ++k) osv[k] = osc[cob + (k & 3) + 8 * (k >> 2)];
        }
        if (do_ep && p.ep.bias) {
#pragma unroll
            for (int k = 0; k < NR; ++k) bvv[k] = p.ep.bias[cob + (k & 3) + 8 * (k >> 2)];
        }
    }
    const unsigned voff = ok_px ? (unsigned)(cob * plane + oy * p.w + ox) * 4u : 0xFFFFFFF0u;
    const bool pair_ok = ox + 1 < p.w;               // (always true on even maps)
    if (do_ep && p.ep.residual) {
        const __amdgpu_buffer_rsrc_t rres = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(p.ep.residual + (int64_t)n * p.y_batch + (int64_t)p.y_choff * plane), 0, p.cout * plane * 4, 0x00020000);
        if (!p.odd) {
#pragma unroll
            for (int k = 0; k < NR; ++k)
                rr[k] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rres, voff, ((k & 3) + 8 * (k >> 2)) * plane * 4, 0));
        } else {                                      // odd map sides: rows are not 8-byte aligned
            const unsigned voff1 = (ok_px && pair_ok) ? voff + 4u : 0xFFFFFFF0u;
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                rr[k].x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rres, voff, ((k & 3) + 8 * (k >> 2)) * plane * 4, 0));
                rr[k].y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rres, voff1, ((k & 3) + 8 * (k >> 2)) * plane * 4, 0));
            }
        }
    }
    // The residual at half resolution (the resnet skip branch: 1x1 conv at the block's INPUT resolution, networks.py:1157,245-250), 2x
    // up-sampled here with the [1,3,3,1] (x) [1,3,3,1] / 16 filter of upfirdn2d.upsample2d (up = 2, padding [2,1,2,1], gain 4):
    //   out[2m] = x[m-1] / 4 + 3 x[m] / 4,   out[2m+1] = 3 x[m] / 4 + x[m+1] / 4   per axis, zeros outside the map.
    // The workgroup's 4 x 18 low-resolution window of its 32 channels (9 KB) goes through LDS, behind the exchange slots: the full
    // resolution skip tensor -- one write and one read of the largest activation of the block -- never exists.
    // (the window itself was requested in the prologue, see there)
    if (do_ep && p.ep.noise && ok_px && !pre_ep) {
        const float ns = p.ep.noise_strength ? *p.ep.noise_strength : 1.f;
        const float* np_ = p.ep.noise + (int64_t)(p.ep.noise_n > 1 ? n : 0) * plane + (int64_t)oy * p.w + ox;
        if (!p.odd) {
            const float2 nv = *reinterpret_cast<const float2*>(np_);
            nz0 = nv.x * ns; nz1 = nv.y * ns;
        } else {
            nz0 = np_[0] * ns;
            nz1 = pair_ok ? np_[1] * ns : 0.f;
        }
    }
    __syncthreads();
    if (pre_ep) {
        const int chl = cob - co0;
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const int cl = chl + (k & 3) + 8 * (k >> 2);
            osv[k] = p.out_scale ? obs[cl] : 1.f;
            bvv[k] = obs[64 + cl];
        }
        if (do_ep && p.ep.noise) {
            const float ns = p.ep.noise_strength ? *p.ep.noise_strength : 1.f;
            const float2 nv = *reinterpret_cast<const float2*>(nzs + 64 * (2 * trow + orow) + 2 * tx);
            nz0 = nv.x * ns; nz1 = nv.y * ns;
        }
    }
    if (UMODE == 1 && p.res_low) {
        // this wave's output row is oy = oy0 + 2 trow + orow: low rows (m-1, m) with weights (1/4, 3/4) for orow = 0, (m, m+1) with
        // (3/4, 1/4) for orow = 1, i.e. window rows trow + orow and trow + orow + 1; window columns tx, tx + 1, tx + 2
        // (two channel rows per step in packed fp32 -- k and k + 1 are neighbouring channels, planes 72 floats apart; round 3: the scalar
        // form was 234 us of the persistent kernel's 4020 at 32 x 1024^2)
        const float wa = orow ? 0.75f : 0.25f, wb = 1.f - wa;
        const v2f wa2 = {wa, wa}, wb2 = {wb, wb}, q25 = {0.25f, 0.25f}, q75 = {0.75f, 0.75f};
        const int chl = cob - co0;
#pragma unroll
        for (int k = 0; k < NR; k += 2) {
            const float* lp = lowt + (chl + (k & 3) + 8 * (k >> 2)) * low_ch + (trow + orow) * low_row + tx + low_col;
            const float* lq = lp + low_ch;                        // the neighbouring channel
            const v2f a0 = {lp[0], lq[0]}, a1 = {lp[1], lq[1]}, a2 = {lp[2], lq[2]};
            const v2f b0 = {lp[low_row], lq[low_row]}, b1 = {lp[low_row + 1], lq[low_row + 1]}, b2 = {lp[low_row + 2], lq[low_row + 2]};
            const v2f c0 = wa2 * a0 + wb2 * b0, c1 = wa2 * a1 + wb2 * b1, c2 = wa2 * a2 + wb2 * b2;
            const v2f rx2 = q25 * c0 + q75 * c1, ry2 = q75 * c1 + q25 * c2;
            rr[k].x = rx2.x; rr[k + 1].x = rx2.y;
            rr[k].y = ry2.x; rr[k + 1].y = ry2.y;
        }
    }
    {
        // Branch-free: absent epilogue pieces take their neutral values (noise / bias / residual 0, slope and gain 1) and pixels outside
        // the map an out-of-range store offset, so the 16 outputs of a lane are straight-line code the compiler can batch -- written with
        // `if (do_ep)`, `if (act == ...)`, `if (ok_px)` around every element it became ~400 basic blocks, each an LDS read, a full wait
        // and a branch.
        const float slope = !do_ep ? 1.f : (p.ep.act == MGF_ACT_LRELU ? p.ep.alpha : (p.ep.act == MGF_ACT_RELU ? 0.f : 1.f));
        const float gain = do_ep ? p.ep.gain : 1.f;
        const float nzq[2] = {do_ep ? nz0 : 0.f, do_ep ? nz1 : 0.f};
        float2 vout[NR];
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            float v[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if constexpr (MASK) {
                    const float t = pa[(2 * k + q) * 64] + sgn * (own[2 * k + q] + pb[(2 * k + q) * 64]), m = q ? rr[k].y : rr[k].x;
                    const int r = p.mask_ring, px = ox + q;
                    v[q] = (oy >= r && oy < p.h - r && px >= r && px < p.w - r) ? (m > 0.f ? t : t * p.mask_slope) : 0.f;
                } else {
                float t = (pa[(2 * k + q) * 64] + sgn * (own[2 * k + q] + pb[(2 * k + q) * 64])) * osv[k];
                t += nzq[q];
                t += do_ep ? bvv[k] : 0.f;
                { float ts = t * slope, m; asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(t), "v"(ts)); t = m; }   // slope in [0, 1] (host-checked): leaky / plain ReLU / identity = max(t, slope t); as an instruction: `fmaxf` adds a canonicalising v_max x, x
                t = t * gain + (q ? rr[k].y : rr[k].x);
                v[q] = t;
                }
            }
            vout[k] = make_float2(v[0], v[1]);
        }
        typedef unsigned v2u __attribute__((ext_vector_type(2)));
        const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(p.y + (int64_t)n * p.y_batch + (int64_t)p.y_choff * plane), 0, p.cout * plane * 4, 0x00020000);
        if (!p.odd) {
#pragma unroll
            for (int k = 0; k < NR; ++k)
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, vout[k]), ry, voff, ((k & 3) + 8 * (k >> 2)) * plane * 4, 0);
        } else {                                      // odd map sides: rows are not 8-byte aligned, the last pair of a row may be half outside
            const unsigned voff1 = (ok_px && pair_ok) ? voff + 4u : 0xFFFFFFF0u;
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vout[k].x), ry, voff, ((k & 3) + 8 * (k >> 2)) * plane * 4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vout[k].y), ry, voff1, ((k & 3) + 8 * (k >> 2)) * plane * 4, 0);
            }
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------------------
// Form 3, PERSISTENT, weights resident in registers: the shallow-K layers (cin = 32 / 64: conv1 of the 512^2 / 1024^2 blocks and
// conv_last + ToRGB, 8 - 16 chunks per tile).  In the one-shot kernel above such a workgroup lives for 8 chunks: its time is the SUM of a
// prologue (addresses, three chunks of loads from a cold start), a loop too short to pipeline anything, and an epilogue, and every
// workgroup streams the whole 16 x cin x 32 weight slab from L2 -- 64 KB for 128 output pixels at 1024^2, more than its input footprint
// (ablations in DESIGN 3.1c: at 1024^2 only 1.4 of 3.4 ms are matrix work).  Here a workgroup walks a STRIP of `strip_len` consecutive tiles
// of one tile row:
//   * a wave's A operands -- its 4 positions x all cin channels of its 32 output channels, 8 bytes per position and chunk -- are loaded
//     ONCE and stay in 2 x 4 x NCK registers (64 at cin = 32), already multiplied by the sample's styles (the reference's w * s,
//     networks.py:288-291; the one-shot kernel scales the input instead): the loop has no weight loads and no style work;
//   * the chunk pipeline (load x three chunks ahead, park two ahead, transform one ahead) runs ACROSS tile boundaries: the next tile's
//     first chunks are in flight while the current tile's last MFMAs and its epilogue run, so nothing starts cold after the first tile;
//   * the epilogue's operands (half-resolution residual window, noise rows) come by LDS-DMA issued during the tile's second chunk
//     through inline asm, i.e. invisible to the compiler's s_waitcnt bookkeeping (a DMA it knows of makes it wait for that DMA in front
//     of the next LDS access of any kind).  Their completion is implied: vmcnt retires in issue order and every wave waits for the x
//     loads it issues AFTER the DMAs (one chunk later), several barriers before the epilogue reads the window;
//   * the exchange slots of the output transform have LDS of their own (the staging buffers are live across the epilogue).
// 43 KB of LDS and <= 256 registers: two workgroups per CU.
typedef int w3_v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ w3_v4i w3_make_rsrc(const void* ptr, unsigned bytes) {
    const uint64_t a = (uint64_t)ptr;
    w3_v4i r;
    r.x = (int)(unsigned)a;
    r.y = (int)((unsigned)(a >> 32) & 0xFFFFu);
    r.z = (int)bytes;
    r.w = 0x00020000;
    return r;
}

// buffer_load_dword ... lds outside the compiler's view: lane l writes its dword to LDS byte address lds_addr + 4 l (out of range =
// 0).  M0 carries the LDS address and is compiler-reserved: saved and restored inside the statement (guide: inline asm, LDS-DMA recipe).
__device__ __forceinline__ void w3_dma_b32(w3_v4i rsrc, unsigned lds_addr, unsigned voff, unsigned soff) {
    unsigned keep;
    asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(rsrc), "s"(lds_addr), "s"(soff)
                 : "memory");
}

// the 16-byte form (gfx950): lane l writes its four dwords to LDS byte address lds_addr + 16 l
__device__ __forceinline__ void w3_dma_b128(w3_v4i rsrc, unsigned lds_addr, unsigned voff, unsigned soff) {
    unsigned keep;
    asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(rsrc), "s"(lds_addr), "s"(soff)
                 : "memory");
}

#ifndef W3P_XD_PLAIN
#define W3P_XD_PLAIN 4
#endif
#ifndef W3P_XD_RGB
#define W3P_XD_RGB 8
#endif
template <int NCK, bool RGB, bool MASK = false>
__global__ __launch_bounds__(256, 2) void wino3p_conv_kernel(Wino3Params p) {
    static_assert(!MASK || !RGB, "the masked epilogue replaces the plain one");
    static_assert(NCK % 2 == 0 && NCK >= 4, "the staging buffers alternate per chunk");
    constexpr int FP = 6 * W3FW;                                   // footprint pixels per channel (6 rows x 34)
    constexpr int CST = 256, RAW = W3CK * CST;
    constexpr int NV = 16, NR = 8;
    static_assert(!RGB || NCK == NR, "the deferred ToRGB projection runs one part per chunk body and stores after part NR - 1");
    constexpr unsigned OOB = 0xFFFFFFF0u;
    extern __shared__ float lds[];
    float* const raw0 = lds;
    float* const raw1 = raw0 + RAW;
    float* const xch = raw1 + RAW;                                 // [6 slots][NV][64 lanes]
    float* const lowt = xch + 6 * NV * 64;                         // [32][4][24] half-resolution residual window in 16-byte pieces (RGB: [3][32] projection weights)
    float* const nzs = lowt + 3072;                                // [4 rows][64]
    float* const obs = nzs + 256;                                  // [2][64]: out_scale, bias of the 32 channels
    const int tid = threadIdx.x, lane = tid & 63;
    const int a = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int tx = l31 & 15, ty = l31 >> 4;

    int b_ = blockIdx.x;
    if (p.xcd_per > 0) {
        b_ = (b_ & 7) * p.xcd_per + (b_ >> 3);
        if (b_ >= p.n * p.strips_x * p.strips_y * p.co_tiles) return;
    }
    // Strip direction.  Horizontal (round 3, first half): the strip walks along x, its tiles re-request two of the three 128-byte lines of
    // every footprint row one tile later -- longer than an XCD's L2 keeps anything under this kernel's traffic -- and the launch fetched
    // 2.9 x its input (15.7 GB against 5.5 at 32 x 1024^2: it ran at the memory system's 5.3 TB/s, not at its instruction rate).
    // Vertical: the strip walks DOWN a 32-pixel column and the strips of neighbouring columns are consecutive work items, i.e. run side
    // by side on one XCD: the shared lines are requested by both neighbours at about the same time (one L2 miss), and what a tile
    // re-requests later is only its two halo ROWS of six.
    const int cot = b_ % p.co_tiles; b_ /= p.co_tiles;
    const int sx = b_ % p.strips_x; b_ /= p.strips_x;
    const int sy = b_ % p.strips_y;
    const int n = b_ / p.strips_y;
    const int vert = p.vert;
    const int co0 = cot * 32;
    const int oy_s = (vert ? sy * p.strip_len : sy) * 4, ox_s = (vert ? sx : sx * p.strip_len) * 32;
    const int tdx = vert ? 0 : 32, tdy = vert ? 4 : 0;             // position step per tile
    const int ntiles = vert ? min(p.strip_len, p.tiles_y - sy * p.strip_len) : min(p.strip_len, p.tiles_x - sx * p.strip_len);
    const int plane = p.h * p.w;
    const float* xn = p.x + (int64_t)n * p.cin * plane;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)xn, 0, p.cin * plane * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc((void*)p.u, 0, 16 * p.cin * p.cout * 4, 0x00020000);

    // ---- resident A operands: position 4a + b, chunk c -> channels {half, half + 2} of the chunk, output channel co0 + l31; x style ----
    v2f A[NCK][4];
    {
        const unsigned aoff = (unsigned)(((co0 + l31) * W3CK + half * 2) * 4);
        const int upos = NCK * p.cout * W3CK * 4;                  // bytes between two positions
        const int ubase = 4 * a * upos;
#pragma unroll
        for (int c = 0; c < NCK; ++c)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                A[c][b] = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(ru, aoff, ubase + c * p.cout * 16 + b * upos, 0));
        if (p.in_scale) {
            const float* sc = p.in_scale + (int64_t)n * p.cin;
#pragma unroll
            for (int c = 0; c < NCK; ++c) {
                const float s0 = sc[4 * c + half], s1 = sc[4 * c + half + 2];
#pragma unroll
                for (int b = 0; b < 4; ++b) { A[c][b].x *= s0; A[c][b].y *= s1; }
            }
        }
    }
    // ---- per-workgroup constants of the epilogue into LDS (visible after the first barrier) ----
    if (RGB) {
        if (tid < 96) {
            const int cc = tid >> 5, co = tid & 31;
            float v = 0.f;
            if (cc < p.rgb_channels)
                v = p.rgb_w[((int64_t)n * p.rgb_channels + cc) * p.cout + co0 + co] * (p.out_scale ? p.out_scale[(int64_t)n * p.os_stride + co0 + co] : 1.f);
            lowt[tid] = v;
        }
    } else if (tid < 32) {
        obs[tid] = p.out_scale ? p.out_scale[(int64_t)n * p.os_stride + co0 + tid] : 1.f;
        obs[64 + tid] = (p.has_ep && p.ep.bias) ? p.ep.bias[co0 + tid] : 0.f;
    }

    // ---- footprint addressing: thread = footprint pixel, channel in the scalar offset; the tile's x position enters per tile ----
    const int fr = tid / W3FW, fq = tid - fr * W3FW;
    auto tile_voff = [&](int t) -> unsigned {
        const int iy = oy_s + tdy * t - 1 + fr, ix = ox_s + tdx * t - 1 + fq;
        return (tid < FP && t < ntiles && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w) ? (unsigned)(iy * p.w + ix) * 4u : OOB;
    };
    auto load_x = [&](float (&dst)[W3CK], unsigned voff, int chunk) {
#pragma unroll
        for (int j = 0; j < W3CK; ++j)
            dst[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, voff, (chunk * W3CK + j) * plane * 4, 0));
    };
    auto park_x = [&](float* R, const float (&src)[W3CK]) {
#pragma unroll
        for (int j = 0; j < W3CK; ++j) R[j * CST + tid] = src[j];
    };
    const int pr = a == 0 ? 0 : (a == 2 ? 2 : 1);
    const int qr = a == 2 ? 1 : (a == 3 ? 3 : 2);
    const float sg = a == 1 ? 1.f : -1.f;
    // Row a of B^T d B.  The packed form (5 packed instructions per pair, as in the one-shot kernel) measures FASTER than the plain scalar
    // form with the minimum of 8 lane-operations per (tile, channel) (W3P_SCALAR_T=1: +1 - 3 %): beside FP32 MFMAs it is the number of
    // VALU instructions that costs matrix time, not the number of lane-operations.
    auto transform = [&](float (&B)[2][4], const float* R) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const float* src = R + (half + 2 * kk) * CST + 2 * ty * W3FW + 2 * tx;
            const v2f p01 = *reinterpret_cast<const v2f*>(src + pr * W3FW), p23 = *reinterpret_cast<const v2f*>(src + pr * W3FW + 2);
            const v2f q01 = *reinterpret_cast<const v2f*>(src + qr * W3FW), q23 = *reinterpret_cast<const v2f*>(src + qr * W3FW + 2);
            const v2f sg2 = {sg, sg}, pm = {-1.f, 1.f}, sgpm = {-sg, sg};
            const v2f t01 = p01 + sg2 * q01, t23 = p23 + sg2 * q23;
            const v2f p2b = {p23.x, p23.x}, q2b = {q23.x, q23.x}, t1b = {t01.y, t01.y};
            const v2f b01 = q2b * sgpm + (p2b * pm + t01);
            const v2f b23 = t23 - t1b;
            B[kk][0] = b01.x;
            B[kk][1] = b01.y;
            B[kk][2] = b23.x;
            B[kk][3] = b23.y;
        }
    };
    f32x16 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

    // ---- epilogue-operand DMA of one tile (non-RGB): half-resolution residual window + the tile's four noise rows ----
    const bool has_low = !RGB && p.res_low != nullptr;
    const bool has_nz = !RGB && p.has_ep && p.ep.noise != nullptr;
    const int hl = p.h >> 1, wl = p.w >> 1, pl = hl * wl;
    // The window as 16-byte pieces: [32 channels][4 rows][6 pieces] = 768 pieces, three per lane (nine 4-byte requests per lane and tile before:
    // 4020 -> 3762 us without them, ablation W3P_ABL=1).  Low-resolution columns (ox0 >> 1) - 4 .. + 19 -- the 18 the tile needs are columns
    // 3 .. 20 of them; the map width and every piece's first column are multiples of 4, so a piece is entirely inside the map or entirely
    // outside (the row's first tile: piece 0; its last tile: piece 5).
    unsigned lowoff[3];                                            // byte offset of piece tid + 256 j in tile 0
    unsigned lowflag = 0;                                          // bit j: piece 0 of a row, bit 3 + j: piece 5
    int lowrow[3] = {0, 0, 0};
    w3_v4i rlow = {0, 0, 0, 0}, rnz = {0, 0, 0, 0};
    if (has_low) {
        rlow = w3_make_rsrc(p.res_low + ((int64_t)n * p.cout + co0) * pl, 32u * (unsigned)pl * 4u);
        const int m0 = (oy_s >> 1) - 1, n0 = (ox_s >> 1) - 4;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int e = tid + 256 * j;
            const int ch = e / 24, rem = e - ch * 24;
            const int r = rem / 6, c = rem - r * 6;
            const int my = m0 + r;
            lowoff[j] = (unsigned)(ch * pl + my * wl + n0 + 4 * c) * 4u;           // (may wrap below zero for piece 0 of tile 0: masked by its edge bit)
            lowrow[j] = my;                                                        // window row of tile 0; a tile further down: + 2 t
            lowflag |= (c == 0 ? 1u : 0u) << j;
            lowflag |= (c == 5 ? 1u : 0u) << (3 + j);
        }
    }
    if (has_nz) rnz = w3_make_rsrc(p.ep.noise + (int64_t)(p.ep.noise_n > 1 ? n : 0) * plane, (unsigned)plane * 4u);
    const unsigned lds_lowt = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uintptr_t)(lowt + 256 * a));    // piece 64 a of a group of 256
    const unsigned lds_nzs = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uintptr_t)(nzs + 64 * a));
    auto issue_ep_dma = [&](int t) {
        const int ox0 = ox_s + tdx * t, oy0 = oy_s + tdy * t;
        if (has_low) {
            // (branch-free per piece: bit j of `edge` = this lane's piece j lies left of the row's first tile or right of its last one; a
            // window row outside the map is a flag too, not a sentinel offset: -16 is a real offset here)
            const unsigned edge = (ox0 == 0 ? lowflag : 0u) | (ox0 + 32 == p.w ? (lowflag >> 3) : 0u);
            const unsigned step = (unsigned)((tdx >> 1) * 4 + (tdy >> 1) * wl * 4) * (unsigned)t;       // bytes the window moves per tile
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int my = lowrow[j] + (tdy >> 1) * t;
                const unsigned off = (((edge >> j) & 1u) || my < 0 || my >= hl) ? OOB : lowoff[j] + step;
                w3_dma_b128(rlow, lds_lowt + 4096u * j, off, 0u);
            }
        }
        if (has_nz) {
            const int ny = oy0 + a, nx = ox0 + lane;
            const unsigned off = (lane < 32 && ny < p.h && nx < p.w) ? (unsigned)(ny * p.w + nx) * 4u : OOB;
            w3_dma_b32(rnz, lds_nzs, off, 0u);
        }
    };

    // ---- epilogue of one tile: output transform, exchange of the four rows through LDS, fused epilogue / ToRGB, stores ----
    const int blk = a & 1, orow = a >> 1;
    const int w0s = a == 1 ? 1 : (a == 2 ? 3 : (a == 3 ? 5 : -1));   // slot receiving my unit 0
    const int w1s = a == 0 ? 0 : (a == 1 ? 2 : (a == 2 ? 4 : -1));   // slot receiving my unit 1
    const int sa = a == 0 ? 1 : (a == 1 ? 0 : (a == 2 ? 1 : 2)), sb = a == 0 ? 3 : (a == 2 ? 5 : 4);
    const float sgn = a < 2 ? 1.f : -1.f;
    const float* pa = xch + sa * (NV * 64) + lane;
    const float* pb = xch + sb * (NV * 64) + lane;
    const bool do_ep = p.has_ep != 0;
    const float slope = !do_ep ? 1.f : (p.ep.act == MGF_ACT_LRELU ? p.ep.alpha : (p.ep.act == MGF_ACT_RELU ? 0.f : 1.f));
    const float gain = do_ep ? p.ep.gain : 1.f;
    const float ns = (do_ep && p.ep.noise) ? (p.ep.noise_strength ? *p.ep.noise_strength : 1.f) : 0.f;
    // (the wave index a -- and with it the own unit a & 1 and the two exchange slots -- is a compile-time value of four instantiations behind
    // one wave-uniform switch: with run-time slots every one of the 32 values carried its own scalar branch and a recomputed LDS address,
    // ~ 100 instructions and 64 branches per tile; now each store is `ds_write_b32 base, v offset:imm`)
    float* const xl = xch + lane;
    auto row_reduce = [&](auto wave_tag, float (&own)[NV]) {
        constexpr int A = decltype(wave_tag)::value, OWN = A & 1;
        constexpr int W0 = A == 1 ? 1 : (A == 2 ? 3 : (A == 3 ? 5 : -1)), W1 = A == 0 ? 0 : (A == 1 ? 2 : (A == 2 ? 4 : -1));
        // unit 0 goes to slot W0, unit 1 to slot W1; the own unit is written too where another wave needs it (waves 1 and 2).  Every value
        // leaves for LDS as soon as it exists: the other unit is never held in registers (they are what bounds the prefetch ring's depth)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
#pragma unroll
            for (int un = 0; un < 2; ++un) {
                constexpr int dummy = 0;
                (void)dummy;
                const int r = RGB ? v : un * 8 + (v >> 1);
                const int jj = RGB ? un : (v & 1);
                const float m0 = acc[0][r], m1 = acc[1][r], m2 = acc[2][r], m3 = acc[3][r];
                const float val = jj == 0 ? m0 + m1 + m2 : m1 - m2 + m3;       // (m3 = -M3, see transform)
                if (un == OWN) own[v] = val;
                const int slot = un == 0 ? W0 : W1;
                if (slot >= 0) xl[slot * (NV * 64) + v * 64] = val;
            }
        }
    };
    auto epilogue = [&](int t) {
        const int ox0 = ox_s + tdx * t, oy0 = oy_s + tdy * t;
        float own[NV];
        switch (a) {
            case 0: row_reduce(std::integral_constant<int, 0>{}, own); break;
            case 1: row_reduce(std::integral_constant<int, 1>{}, own); break;
            case 2: row_reduce(std::integral_constant<int, 2>{}, own); break;
            default: row_reduce(std::integral_constant<int, 3>{}, own); break;
        }
        const int oy = oy0 + 2 * ty + orow, ox = ox0 + 2 * tx + (RGB ? blk : 0);
        const bool ok_px = oy < p.h && ox < p.w;
        if (RGB) {
            const int rc = p.rgb_channels;
            const float* wvs = lowt;
            __syncthreads();
            float sum[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const float yv = pa[v * 64] + sgn * (own[v] + pb[v * 64]);
                const int cl = 4 * half + (v & 3) + 8 * (v >> 2);
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) sum[cc] += yv * wvs[cc * 32 + cl];
            }
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) sum[cc] += __shfl_xor(sum[cc], 32, 64);
            if (half == 0 && ok_px) {
                for (int cc = 0; cc < rc; ++cc) {
                    const float bb = p.rgb_bias ? p.rgb_bias[cc] : 0.f;
                    p.rgb_out[((int64_t)n * rc + cc) * plane + (int64_t)oy * p.w + ox] = sum[cc] + bb;
                }
            }
            return;
        }
        const int cob = co0 + blk * 16 + 4 * half;
        const unsigned voff = ok_px ? (unsigned)(cob * plane + oy * p.w + ox) * 4u : OOB;
        float2 rr[NR];
#pragma unroll
        for (int k = 0; k < NR; ++k) rr[k] = make_float2(0.f, 0.f);
        if (do_ep && p.ep.residual) {
            const __amdgpu_buffer_rsrc_t rres = __builtin_amdgcn_make_buffer_rsrc((void*)(p.ep.residual + (int64_t)n * p.y_batch), 0, p.cout * plane * 4, 0x00020000);
#pragma unroll
            for (int k = 0; k < NR; ++k)
                rr[k] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rres, voff, ((k & 3) + 8 * (k >> 2)) * plane * 4, 0));
        }
        __syncthreads();                                           // the exchange slots are complete (and, long since, the DMA'd operands)
        const int chl = cob - co0;
        float osv[NR], bvv[NR];
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const int cl = chl + (k & 3) + 8 * (k >> 2);
            osv[k] = obs[cl];
            bvv[k] = obs[64 + cl];
        }
        float nz0 = 0.f, nz1 = 0.f;
        if (has_nz) {
            const float2 nv = *reinterpret_cast<const float2*>(nzs + 64 * (2 * ty + orow) + 2 * tx);
            nz0 = nv.x * ns; nz1 = nv.y * ns;
        }
        if (has_low) {
            // two channel rows per step in packed fp32 (k and k + 1 are neighbouring channels, planes 96 floats apart): 234 us of this kernel
            // were interpolation arithmetic in scalar form
            const float wa = orow ? 0.75f : 0.25f, wb = 1.f - wa;
            const v2f wa2 = {wa, wa}, wb2 = {wb, wb}, q25 = {0.25f, 0.25f}, q75 = {0.75f, 0.75f};
#pragma unroll
            for (int k = 0; k < NR; k += 2) {
                const float* lp = lowt + (chl + (k & 3) + 8 * (k >> 2)) * 96 + (ty + orow) * 24 + tx + 3;
                const v2f a0 = {lp[0], lp[96]}, a1 = {lp[1], lp[97]}, a2 = {lp[2], lp[98]};
                const v2f b0 = {lp[24], lp[120]}, b1 = {lp[25], lp[121]}, b2 = {lp[26], lp[122]};
                const v2f c0 = wa2 * a0 + wb2 * b0, c1 = wa2 * a1 + wb2 * b1, c2 = wa2 * a2 + wb2 * b2;
                const v2f rx2 = q25 * c0 + q75 * c1, ry2 = q75 * c1 + q25 * c2;
                rr[k].x = rx2.x; rr[k + 1].x = rx2.y;
                rr[k].y = ry2.x; rr[k + 1].y = ry2.y;
            }
        }
        float2 vout[NR];
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            float v[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if constexpr (MASK) {
                    const float t = pa[(2 * k + q) * 64] + sgn * (own[2 * k + q] + pb[(2 * k + q) * 64]), m = q ? rr[k].y : rr[k].x;
                    const int r = p.mask_ring, px = ox + q;
                    v[q] = (oy >= r && oy < p.h - r && px >= r && px < p.w - r) ? (m > 0.f ? t : t * p.mask_slope) : 0.f;
                } else {
                float tt = (pa[(2 * k + q) * 64] + sgn * (own[2 * k + q] + pb[(2 * k + q) * 64])) * osv[k];
                tt += q ? nz1 : nz0;
                tt += bvv[k];
                { float ts = tt * slope, m; asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(tt), "v"(ts)); tt = m; }   // (slope in [0, 1]: max(t, slope t), one instruction instead of compare + select)
                tt = tt * gain + (q ? rr[k].y : rr[k].x);
                v[q] = tt;
                }
            }
            vout[k] = make_float2(v[0], v[1]);
        }
        typedef unsigned v2u __attribute__((ext_vector_type(2)));
        const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)(p.y + (int64_t)n * p.y_batch), 0, p.cout * plane * 4, 0x00020000);
#pragma unroll
        for (int k = 0; k < NR; ++k)
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, vout[k]), ry, voff, ((k & 3) + 8 * (k >> 2)) * plane * 4, 0);
    };

    // ToRGB variant (round 6): the projection behind the row exchange is cut into NCK parts, part c riding in chunk body c of the NEXT tile
    // between that body's MFMAs (its slot reads and their waits pass under matrix work of the same wave); only the row reduction and its
    // barrier stay at the tile's end, the last tile's parts run after the loop.  Measured on one box (tools/w3_top_micro.py, 32 x 1024^2):
    // 3034 / 3021 us against 3159 for the epilogue in one piece (-4 %).  The same split of the OTHER variant's epilogue (skip interpolation,
    // noise / bias / activation, 16 stores; operands double-buffered by tile parity) is correct and measures 1 - 2 % SLOWER (4035 / 3383
    // against 3967 / 3350 us with / without the fused skip): that stream's 200 vector instructions cost the same issue time wherever they
    // stand (profiles/r6_w3p_ablation.txt), and the compiler's interleaving puts LDS waits between the MFMAs.  Not adopted there.
    float own_d[NV];
    float rgb_b[3] = {0.f, 0.f, 0.f};
    if (RGB && p.rgb_bias)
        for (int cc = 0; cc < p.rgb_channels; ++cc) rgb_b[cc] = p.rgb_bias[cc];
    unsigned ep_voff = OOB;                                        // output offset of the tile whose parts are pending (out of range: none yet)
    float ep_sum[3] = {0.f, 0.f, 0.f};
    const __amdgpu_buffer_rsrc_t rrgb = __builtin_amdgcn_make_buffer_rsrc((void*)(RGB ? p.rgb_out + (int64_t)n * p.rgb_channels * plane : p.y), 0,
                                                                          RGB ? p.rgb_channels * plane * 4 : 0, 0x00020000);
    auto tile_reduce_rgb = [&](int t) {
        const int ox0 = ox_s + tdx * t, oy0 = oy_s + tdy * t;
        switch (a) {
            case 0: row_reduce(std::integral_constant<int, 0>{}, own_d); break;
            case 1: row_reduce(std::integral_constant<int, 1>{}, own_d); break;
            case 2: row_reduce(std::integral_constant<int, 2>{}, own_d); break;
            default: row_reduce(std::integral_constant<int, 3>{}, own_d); break;
        }
        const int oy = oy0 + 2 * ty + orow, ox = ox0 + 2 * tx + blk;
        ep_voff = (oy < p.h && ox < p.w) ? (unsigned)(oy * p.w + ox) * 4u : OOB;
        __syncthreads();                                           // the exchange slots are complete
    };
    auto ep_part_rgb = [&](const int k) {                          // k is a constant after unrolling; branch-free (see the call site)
        if (k == 0) { ep_sum[0] = 0.f; ep_sum[1] = 0.f; ep_sum[2] = 0.f; }
#pragma unroll
        for (int v = 2 * k; v < 2 * k + 2; ++v) {
            const float yv = pa[v * 64] + sgn * (own_d[v] + pb[v * 64]);
            const int cl = 4 * half + (v & 3) + 8 * (v >> 2);
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) ep_sum[cc] += yv * lowt[cc * 32 + cl];
        }
        if (k == NR - 1) {
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) ep_sum[cc] += __shfl_xor(ep_sum[cc], 32, 64);
            const unsigned so = half == 0 ? ep_voff : OOB;
#pragma unroll
            for (int cc = 0; cc < 3; ++cc)          // (a plane past rgb_channels lies beyond the resource's records: the store is dropped)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, ep_sum[cc] + rgb_b[cc]), rrgb, so, cc * plane * 4, 0);
        }
    };

    // ---- prologue: chunks 0 and 1 of tile 0 are parked, chunks 2 .. 1 + XD wait in the register ring ----
    // The ring is what keeps memory busy: a workgroup's chunk is 3.2 KB, and with one chunk in flight per workgroup (two workgroups per
    // CU) the whole chip has 1.6 MB outstanding -- 0.8 TB/s at 2 us of loaded latency, less than the layer reads.  XD chunks deep, a
    // load has XD chunk bodies (~ 3 000 cycles) to land before it is parked.
    // (depth: 4 chunks; 8 in the ToRGB variant, whose epilogue leaves the registers -- 32 x 1024^2, same box, two runs each: 3243 / 3312 us
    // with 8 against 3322 / 3348 with 4; in the other variant 8 measured no faster: 4135 / 3538 vs 4103 / 3498.  LDS-DMA staging into a ring of
    // 8 LDS buffers with hand-counted vmcnt -- no staging registers, no LDS stores, a whole tile of prefetch distance -- was built and
    // measured too: correct, and 3 - 5 % SLOWER than this register ring (4329 / 3749 / 3574 vs 4206 / 3675 / 3393 us on one box): four
    // `buffer_load_dword ... lds` with their M0 hand-over per chunk body cost more issue time than four register loads and two 2-dword
    // LDS stores)
    constexpr int XD = RGB ? W3P_XD_RGB : W3P_XD_PLAIN;
    static_assert(NCK % XD == 0, "ring slot = chunk index mod XD must be a compile-time value");
    float xq[XD][W3CK];
    float B[2][2][4];
    // (chunk g = c + 2 + XD of the flattened stream may lie in this tile, the next one or -- ring of 8 -- the one after: three tile offsets)
    unsigned voff_cur = tile_voff(0), voff_nxt = tile_voff(1), voff_n2 = tile_voff(2);
    auto load_ahead = [&](float (&dst)[W3CK], int g) {               // g: chunk index relative to the current tile's chunk 0 (compile-time)
        load_x(dst, g < NCK ? voff_cur : (g < 2 * NCK ? voff_nxt : voff_n2), g % NCK);
    };
    static_assert(2 + XD + NCK - 1 < 3 * NCK, "the ring reaches at most two tiles ahead");
    {
        float xa[W3CK], xb[W3CK];
        load_x(xa, voff_cur, 0);
        load_x(xb, voff_cur, 1);
#pragma unroll
        for (int d = 0; d < XD; ++d) load_ahead(xq[d], 2 + d);
        park_x(raw0, xa);
        park_x(raw1, xb);
        __syncthreads();
        transform(B[0], raw0);
        __syncthreads();                                           // chunk 0's body parks chunk 2 over raw0: every wave must have read chunk 0 from it
    }
    // ---- the strip: NCK chunk bodies + one epilogue per tile; the chunk pipeline does not stop at tile boundaries ----
    for (int t = 0; t < ntiles; ++t) {
#pragma unroll
        for (int c = 0; c < NCK; ++c) {
            __builtin_amdgcn_sched_barrier(0);
            // (every wave passed the barrier of chunk 0: the previous tile's epilogue is over.  In FRONT of this body's loads: the compiler
            // counts only its own loads, so a DMA younger than a load it waits for would be waited for as well)
            if (!RGB && c == 1) issue_ep_dma(t);
            transform(B[(c + 1) & 1], ((c + 1) & 1) ? raw1 : raw0);          // chunk c + 1 (of the next tile when c is the last)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                // (a tile's first MFMA per accumulator takes the constant 0 as its C operand: clearing 64 accumulator registers per tile with
                // v_mov costs as much matrix time as four of the tile's 64 MFMAs)
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[c][b].x, B[c & 1][0][b], c == 0 ? f32x16{} : acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[c][b].y, B[c & 1][1][b], acc[b], 0, 0, 0);
            }
            // ToRGB: the previous tile's projection, part c.  Unconditional -- in the strip's first tile the parts run on whatever the
            // registers hold and store through the out-of-range offset ep_voff starts with: a branch here would make the compiler merge its
            // vmcnt bookkeeping over both paths and drain the prefetch ring in every body
            if constexpr (RGB) ep_part_rgb(c);
            __builtin_amdgcn_sched_barrier(0);
            park_x((c & 1) ? raw1 : raw0, xq[c % XD]);                       // chunk c + 2, requested XD bodies ago
            load_ahead(xq[c % XD], c + 2 + XD);
            __syncthreads();
        }
        if constexpr (RGB) tile_reduce_rgb(t); else epilogue(t);
        voff_cur = voff_nxt;
        voff_nxt = voff_n2;
        voff_n2 = tile_voff(t + 3);
    }
    if constexpr (RGB) {                                           // the last tile's parts (nothing left to hide them under)
        if (ntiles > 0) {
#pragma unroll
            for (int k = 0; k < NR; ++k) ep_part_rgb(k);
        }
    }
}

}  // namespace

static int g_w3_forced_shape = 0;

extern "C" int mgf_winograd3_force_shape(int32_t shape) {
    MGF_REQUIRE(shape == 0 || shape == 21 || shape == 12 || shape == 11 || shape == 31, MGF_EINVAL,
                "winograd3_force_shape: 0 (auto), 21, 12, 11 or 31 = the persistent form wherever the layer's structure admits it (got %d)", shape);
    g_w3_forced_shape = shape;
    return MGF_OK;
}

static int launch_wino3(float* y, const float* x, const float* u, const float* in_scale, const float* out_scale, int32_t n, int32_t cin, int32_t h,
                        int32_t w, int32_t cout, int32_t out_scale_stride, const mgf_epilogue* ep, const float* rgb_w, const float* rgb_bias,
                        float* rgb_out, int32_t rgb_channels, mgf_stream_t stream, const float* res_low = nullptr, int64_t y_batch = 0,
                        int32_t y_choff = 0, bool batch_invariant = false, bool masked = false, int32_t mask_ring = 0, float mask_slope = 0.f) {
    const bool rgb = rgb_out != nullptr;
    MGF_REQUIRE((y || rgb) && x && u && n >= 1 && cin >= 1 && cout >= 1 && h >= 2 && w >= 2, MGF_EINVAL, "conv3x3_winograd3: bad arguments");
    MGF_REQUIRE(cin % W3CK == 0 && cout % 32 == 0, MGF_EUNSUPPORTED, "conv3x3_winograd3: cin must be a multiple of %d and cout of 32 (got %d, %d)",
                W3CK, cin, cout);
    MGF_REQUIRE(cin <= 1024, MGF_EUNSUPPORTED, "conv3x3_winograd3: at most 1024 input channels (got %d)", cin);
    const bool odd = (h % 2) || (w % 2);
    MGF_REQUIRE(!(odd && (rgb || res_low)), MGF_EUNSUPPORTED, "conv3x3_winograd3: the fused ToRGB / half-resolution residual need even map sides (got %dx%d)", h, w);
    MGF_REQUIRE(y_choff >= 0 && (y_batch == 0 || y_batch >= (int64_t)(y_choff + cout) * h * w), MGF_EINVAL, "conv3x3_winograd3: bad output slice");
    MGF_REQUIRE(odd || (y_batch % 2 == 0), MGF_EINVAL, "conv3x3_winograd3: y_batch must keep rows 8-byte aligned");
    MGF_REQUIRE(!(y_batch || y_choff) || !(rgb || res_low), MGF_EUNSUPPORTED, "conv3x3_winograd3: channel-slice outputs are for the plain launch");
    MGF_REQUIRE((int64_t)cin * h * w <= INT32_MAX / 4 && (int64_t)16 * cin * cout <= INT32_MAX / 4 && (int64_t)(y_choff + cout) * h * w <= INT32_MAX / 4,
                MGF_ETOOBIG, "conv3x3_winograd3: one sample / the weight planes must stay below 2 GiB (32-bit buffer offsets)");
    MGF_REQUIRE(((uintptr_t)u % 16) == 0 && (odd || ((uintptr_t)(rgb ? rgb_out : y) % 8) == 0), MGF_EINVAL, "conv3x3_winograd3: u must be 16-byte and the output 8-byte aligned");
    if (ep) {
        MGF_REQUIRE(ep->act == 0 || ep->act == MGF_ACT_LINEAR || ep->act == MGF_ACT_LRELU || ep->act == MGF_ACT_RELU, MGF_EUNSUPPORTED,
                    "conv3x3_winograd3: epilogue activation %d unsupported", ep->act);
        MGF_REQUIRE(ep->act != MGF_ACT_LRELU || (ep->alpha >= 0.f && ep->alpha <= 1.f), MGF_EUNSUPPORTED,
                    "conv3x3_winograd3: leaky-ReLU slope %g outside [0, 1] (the epilogue forms max(t, slope t))", (double)ep->alpha);
        MGF_REQUIRE(odd || !ep->residual || ((uintptr_t)ep->residual % 8) == 0, MGF_EINVAL, "conv3x3_winograd3: the residual must be 8-byte aligned");
        MGF_REQUIRE(odd || !ep->noise || ((uintptr_t)ep->noise % 8) == 0, MGF_EINVAL, "conv3x3_winograd3: the noise map must be 8-byte aligned");
    }
    if (rgb) {
        MGF_REQUIRE(cout == 32 && rgb_w && rgb_channels >= 1 && rgb_channels <= 3 && !ep, MGF_EUNSUPPORTED,
                    "conv3x3_winograd3_rgb: needs cout == 32, 1..3 projected channels and no epilogue (got cout %d, %d channels)", cout, rgb_channels);
    }
    // Shape: 32 channels x 32 tiles with 64 accumulators per wave and FOUR workgroups per CU.  Measured on the generator's conv1 layers
    // at 25 samples (tools/w3_phases.py; shapes 21 / 12 / 11, us): 64^2 2412 / 2297 / 2138, 128^2 2273 / 2408 / 2254, 256^2 2543 /
    // 2681 / 2525, 512^2 3078 / 3303 / 3011, 1024^2 - / 4376 / 3940 -- residency (latency hiding across workgroups) is worth more than
    // the instructions the wider shapes save.  MGF_W3_SHAPE = 21 | 12 | 11 or mgf_winograd3_force_shape pin a shape (tuning, tests).
    static const int env_forced = [] { const char* e = mgf_knob("MGF_W3_SHAPE"); return e ? atoi(e) : 0; }();
    // batch_invariant (mgf_wino3_batch_invariant_f32): the form follows the layer's shape alone, never the sample count or a pinned shape
    const int forced = batch_invariant ? 0 : (g_w3_forced_shape ? g_w3_forced_shape : env_forced);
    int shape = 11;
    // ... except where the 64-channel shape measures faster: deep K with enough workgroups left to fill the chip (the 128^2 x 256-channel
    // conv1 at 25 samples: 1969 vs 2097 us; at 64^2 x 512 its 6400 workgroups lose to 12800 of the small shape, 2151 vs 1998 us)
    // (round 3, 32 samples: 64^2 x 512 -- 8192 workgroups of the wide shape -- 2653 vs 2502 us for the small one; 128^2 x 256 -- 16384 -- 2485 vs
    // 2665: the wide shape needs ~ 12 800 workgroups, 25 rounds of the 512 the chip holds, before its smaller instruction count per MFMA wins)
    // (round 6: with its operands requested one chunk earlier -- the DEEP rings of the kernel -- the wide shape wins from ONE round of the chip's 512
    // two-per-CU slots on: tools/w3_shape_ab.py, us for shapes 21 / 11 at 512 channels 64^2: 296-306 / 322 at 4 samples (1024 workgroups), 588-591 /
    // 618-631 at 8, 1161-1172 / 1222-1231 at 16, 2253-2266 / 2423-2509 at 32; 32^2: 149 / 164 at 8 (512 workgroups), 286-295 / 309-315 at 16, 610-664 /
    // 657-777 at 32, but 107 / 99 at 4 (256 workgroups); 256 channels 128^2: 85 / 94 at one sample (512 workgroups) .. 2394-2432 / 2573-2583 at 32.
    // The threshold was 12 800 workgroups for the kernel that requested them one chunk ahead.)
    if (!batch_invariant && !forced && !rgb && !res_low && !odd && y_choff == 0 && cout % 64 == 0 && cin >= 256 &&
        (int64_t)n * mgf_cdiv(w, 32) * mgf_cdiv(h, 4) * (cout / 64) >= 512) shape = 21;
    if (forced == 21 && cout % 64 == 0 && !rgb) shape = 21;
    if (forced == 12 || forced == 11) shape = forced;
    const bool force_persist = forced == 31;
    const int cb = shape == 21 ? 2 : 1, tb = shape == 12 ? 2 : 1;
    Wino3Params p;
    p.y = y; p.x = x; p.u = u; p.in_scale = in_scale; p.out_scale = out_scale;
    p.n = n; p.cin = cin; p.h = h; p.w = w; p.cout = cout; p.os_stride = out_scale_stride;
    p.tiles_x = (int)mgf_cdiv(w, 32); p.tiles_y = (int)mgf_cdiv(h, 4 * tb); p.co_tiles = cout / (32 * cb);
    p.has_ep = ep != nullptr;
    if (ep) { p.ep = *ep; if (p.ep.act == 0) p.ep.act = MGF_ACT_LINEAR; } else { p.ep = mgf_epilogue{}; p.ep.gain = 1.f; }
    p.rgb_w = rgb_w; p.rgb_bias = rgb_bias; p.rgb_out = rgb_out; p.rgb_channels = rgb_channels;
    p.res_low = res_low;
    p.y_batch = y_batch ? y_batch : (int64_t)cout * h * w; p.y_choff = y_choff; p.odd = odd;
    p.strip_len = 0; p.strips_x = 0; p.vert = 0; p.strips_y = 0;
    p.mask_ring = mask_ring; p.mask_slope = mask_slope;
    MGF_REQUIRE(!masked || (batch_invariant && shape == 11 && !rgb && !res_low && ep && ep->residual), MGF_EINVAL,
                "conv3x3_winograd3: the masked epilogue is a batch-invariant one-block launch with a mask map");
    static const bool pieces_off = [] { const char* e = mgf_knob("MGF_W3_LOW_PIECES"); return e && e[0] == '0'; }();   // tuning hook (A/B runs)
    p.low_pieces = (res_low && !pieces_off && ((w >> 1) & 3) == 0 && ((uintptr_t)res_low & 15) == 0) ? 1 : 0;
    if (res_low) {
        MGF_REQUIRE(ep && !ep->residual && !rgb, MGF_EINVAL, "conv3x3_winograd3_up2res: needs an epilogue without a full-resolution residual");
        MGF_REQUIRE(shape == 11, MGF_EUNSUPPORTED, "conv3x3_winograd3_up2res: only the 32x32-tile shape takes the half-resolution residual");
        MGF_REQUIRE((int64_t)32 * (h / 2) * (w / 2) * 4 <= INT32_MAX, MGF_ETOOBIG, "conv3x3_winograd3_up2res: map too large");
    }
    // Persistent form (wino3p_conv_kernel): shallow K (cin 32 / 64), 32-channel tiles, even maps, whole strips of 32 tiles (or one tile row
    // when it is shorter), a dense output, and enough strips to fill the chip's 512 workgroup slots several times over.
    // MGF_W3_PERSIST=0 keeps the one-shot kernel (tuning / A-B runs).
    static const bool persist_off = [] { const char* e = mgf_knob("MGF_W3_PERSIST"); return e && e[0] == '0'; }();
    static const int strip_env = [] { const char* e = mgf_knob("MGF_W3_STRIP"); return e ? atoi(e) : 0; }();
    const int strip_len = strip_env > 0 ? std::min(strip_env, p.tiles_x) : std::min(p.tiles_x, 32);     // (1024^2 at 32 samples, us: strips of 4 / 8 / 16 / 32 tiles 3707 / 3536 / 3472 / 3428)
    // vertical strips where the tile rows divide into whole strips (MGF_W3_VERT=0: the horizontal walk, for A/B runs).  A strip is as long
    // as the launch can afford: 32 tiles when that still gives the chip's 512 workgroup slots four rounds of work (2048 workgroups), else 16,
    // 8 or 4 -- a single 1024^2 image (gradient mode, one target) is 2048 strips of 4 tiles, and the persistent form's resident weights and
    // cross-tile prefetch still beat the one-shot kernel there (strips of 4 / 8 / 16 / 32 at 32 samples: 3707 / 3536 / 3472 / 3428 us)
    static const bool vert_off = [] { const char* e = mgf_knob("MGF_W3_VERT"); return e && e[0] == '0'; }();
    int vlen = std::min(p.tiles_y, strip_env > 0 ? strip_env : 32);
    if (strip_env <= 0)
        while (vlen > 4 && vlen % 2 == 0 && p.tiles_y % vlen == 0 && (int64_t)n * p.tiles_x * (p.tiles_y / vlen) * p.co_tiles < 2048) vlen /= 2;
    const bool vert_ok = !vert_off && p.tiles_y % vlen == 0;
    const int64_t pcount = vert_ok ? (int64_t)n * p.tiles_x * (p.tiles_y / vlen) * p.co_tiles : (int64_t)n * (p.tiles_x / strip_len) * p.tiles_y * p.co_tiles;
    const bool persist = !persist_off && (!forced || force_persist) && shape == 11 && !odd && y_choff == 0 && p.y_batch == (int64_t)cout * h * w && cin == 32 &&
                         w % 32 == 0 && h % 4 == 0 && p.tiles_x % strip_len == 0 && (!rgb || cout == 32) &&
                         (force_persist || batch_invariant || pcount >= 2048);
    if (persist) {
        p.vert = vert_ok ? 1 : 0;
        if (p.vert) { p.strip_len = vlen; p.strips_x = p.tiles_x; p.strips_y = p.tiles_y / vlen; }
        else { p.strip_len = strip_len; p.strips_x = p.tiles_x / strip_len; p.strips_y = p.tiles_y; }
        int64_t pblocks = (int64_t)n * p.strips_x * p.strips_y * p.co_tiles;
        p.xcd_per = (int)((pblocks + 7) / 8);                      // XCD-contiguous order: channel tiles, then strips of one row, share an L2
        pblocks = (int64_t)p.xcd_per * 8;
        const size_t plds = (size_t)(2 * 4 * 256 + 6 * 16 * 64 + 3072 + 256 + 128) * sizeof(float);
        static bool pattr_set = false;
        if (!pattr_set) {
            hipError_t e = hipFuncSetAttribute((const void*)wino3p_conv_kernel<8, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
            if (e == hipSuccess) e = hipFuncSetAttribute((const void*)wino3p_conv_kernel<8, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
            if (e == hipSuccess) e = hipFuncSetAttribute((const void*)(wino3p_conv_kernel<8, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
            if (e != hipSuccess) { mgf_set_error("conv3x3_winograd3: cannot raise dynamic LDS: %s", hipGetErrorString(e)); return MGF_ELAUNCH; }
            pattr_set = true;
        }
        const char* pname = masked ? "wino3p_conv_kernel<8, false, true>" : (rgb ? "wino3p_conv_kernel<8, true>" : "wino3p_conv_kernel<8, false>");
        mgf_prof_external_begin((hipStream_t)stream, pname, 2.0 * 9 * cin * (double)cout * h * w * n,
                                4.0 * ((double)n * cin * h * w + 9.0 * cin * cout + (double)n * (rgb ? rgb_channels : cout) * h * w));
        const dim3 pgrid((unsigned)pblocks), pblk(256);
        hipStream_t pst = (hipStream_t)stream;
        if (masked) hipLaunchKernelGGL((wino3p_conv_kernel<8, false, true>), pgrid, pblk, plds, pst, p);
        else if (rgb) hipLaunchKernelGGL((wino3p_conv_kernel<8, true>), pgrid, pblk, plds, pst, p);
        else hipLaunchKernelGGL((wino3p_conv_kernel<8, false>), pgrid, pblk, plds, pst, p);
        mgf_prof_external_end((hipStream_t)stream);
        MGF_CHECK_LAUNCH("conv3x3_winograd3(persistent)");
        return MGF_OK;
    }
    int64_t blocks = (int64_t)n * p.tiles_x * p.tiles_y * p.co_tiles;
    MGF_REQUIRE(blocks <= INT32_MAX - 8, MGF_ETOOBIG, "conv3x3_winograd3: too many workgroups");
    static const char* xcd_env = mgf_knob("MGF_XCD");             // tuning hook (experiments only): 0 disables the XCD-aware order
    p.xcd_per = 0;
    // (also with ONE channel tile: a footprint row is 34 floats around a 32-float = 128-byte line, so its two halo floats pull in the
    // neighbours' lines; with horizontally adjacent tiles on one XCD those are L2 hits instead of a 3x fetch from fabric)
    if ((int64_t)16 * cin * cout * 4 <= (4 << 20) && blocks >= 16 && !(xcd_env && xcd_env[0] == '0')) {
        p.xcd_per = (int)((blocks + 7) / 8);
        blocks = (int64_t)p.xcd_per * 8;
    }
    // main loop: two footprint buffers + the styles; epilogue: 6 exchange slots (+ the ToRGB weights) over the same memory
    const size_t nv = cb * tb == 2 ? 32 : 16;
    static const size_t lds_pad = [] { const char* e = mgf_knob("MGF_W3_LDS_PAD"); return e ? (size_t)atol(e) : (size_t)0; }();   // tuning: fewer workgroups per CU
    const size_t lds = std::max<size_t>((size_t)(2 * 256 * (tb == 2 ? 8 : 4)) * sizeof(float),
                                        (size_t)(6 * nv * 64 + (res_low ? 3072 : 0) + 256 + 128) * sizeof(float)) + lds_pad;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)wino3_conv_kernel<2, 1, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)wino3_conv_kernel<1, 2, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)wino3_conv_kernel<1, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
        if (e != hipSuccess) { mgf_set_error("conv3x3_winograd3: cannot raise dynamic LDS: %s", hipGetErrorString(e)); return MGF_ELAUNCH; }
        attr_set = true;
    }
    // names as rocprofv3 prints the instantiations; algorithmic accounting of the direct form (what the launch replaces)
    const char* name = masked ? "wino3_conv_kernel<1, 1, false, true>" : rgb ? (shape == 12 ? "wino3_conv_kernel<1, 2, true>" : "wino3_conv_kernel<1, 1, true>")
                           : (shape == 21 ? "wino3_conv_kernel<2, 1, false>" : (shape == 12 ? "wino3_conv_kernel<1, 2, false>" : "wino3_conv_kernel<1, 1, false>"));
    mgf_prof_external_begin((hipStream_t)stream, name, 2.0 * 9 * cin * (double)cout * h * w * n,
                            4.0 * ((double)n * cin * h * w + 9.0 * cin * cout + (double)n * (rgb ? rgb_channels : cout) * h * w));
    const dim3 grid((unsigned)blocks), blk(256);
    hipStream_t st = (hipStream_t)stream;
    if (masked) hipLaunchKernelGGL((wino3_conv_kernel<1, 1, false, true>), grid, blk, lds, st, p);
    else if (rgb && shape == 12) hipLaunchKernelGGL((wino3_conv_kernel<1, 2, true>), grid, blk, lds, st, p);
    else if (rgb) hipLaunchKernelGGL((wino3_conv_kernel<1, 1, true>), grid, blk, lds, st, p);
    else if (shape == 21) hipLaunchKernelGGL((wino3_conv_kernel<2, 1, false>), grid, blk, lds, st, p);
    else if (shape == 12) hipLaunchKernelGGL((wino3_conv_kernel<1, 2, false>), grid, blk, lds, st, p);
    else hipLaunchKernelGGL((wino3_conv_kernel<1, 1, false>), grid, blk, lds, st, p);
    mgf_prof_external_end((hipStream_t)stream);
    MGF_CHECK_LAUNCH("conv3x3_winograd3");
    return MGF_OK;
}

extern "C" int mgf_conv3x3_winograd3_f32(float* y, const float* x, const float* u, const float* in_scale, const float* out_scale, int32_t n,
                                         int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t out_scale_stride, const mgf_epilogue* ep,
                                         mgf_stream_t stream) {
    return launch_wino3(y, x, u, in_scale, out_scale, n, cin, h, w, cout, out_scale_stride, ep, nullptr, nullptr, nullptr, 0, stream);
}

// The MDF discriminators' body layers (csrc/mdf.hip): plain form-3 launch whose kernel choice depends on (cin, h, w) only, so that a
// sample's result is the same bits whatever the batch it is launched in.
int mgf_wino3_batch_invariant_f32(float* y, const float* x, const float* u, int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout,
                                  const mgf_epilogue* ep, mgf_stream_t stream) {
    return launch_wino3(y, x, u, nullptr, nullptr, n, cin, h, w, cout, 0, ep, nullptr, nullptr, nullptr, 0, stream, nullptr, 0, 0, true);
}

// The MDF backward's body adjoints (csrc/mdf.hip): the same batch-invariant launch with the masked epilogue -- y = conv(x) * (mask > 0 ?
// 1 : slope) on ring `ring` of the frame, 0 outside it; mask has y's layout and is read where the residual would be.
int mgf_wino3_batch_invariant_masked_f32(float* y, const float* x, const float* u, const float* mask, int32_t n, int32_t c, int32_t h, int32_t w,
                                         int32_t ring, float slope, mgf_stream_t stream) {
    MGF_REQUIRE(mask && ring >= 0, MGF_EINVAL, "conv3x3_winograd3(masked): needs a mask map and a ring depth >= 0");
    mgf_epilogue ep{};
    ep.residual = mask;
    ep.act = MGF_ACT_LINEAR;
    ep.gain = 1.f;
    return launch_wino3(y, x, u, nullptr, nullptr, n, c, h, w, c, 0, &ep, nullptr, nullptr, nullptr, 0, stream, nullptr, 0, 0, true, true, ring, slope);
}

extern "C" int mgf_conv3x3_winograd3_slice_f32(float* y, const float* x, const float* u, const float* in_scale, const float* out_scale, int32_t n,
                                               int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t out_scale_stride, int64_t y_batch,
                                               int32_t y_choff, const mgf_epilogue* ep, mgf_stream_t stream) {
    return launch_wino3(y, x, u, in_scale, out_scale, n, cin, h, w, cout, out_scale_stride, ep, nullptr, nullptr, nullptr, 0, stream, nullptr, y_batch,
                        y_choff);
}

extern "C" int mgf_conv3x3_winograd3_up2res_f32(float* y, const float* x, const float* u, const float* in_scale, const float* out_scale,
                                                const float* residual_low, int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout,
                                                int32_t out_scale_stride, const mgf_epilogue* ep, mgf_stream_t stream) {
    MGF_REQUIRE(residual_low, MGF_EINVAL, "conv3x3_winograd3_up2res: null residual");
    return launch_wino3(y, x, u, in_scale, out_scale, n, cin, h, w, cout, out_scale_stride, ep, nullptr, nullptr, nullptr, 0, stream, residual_low);
}

extern "C" int mgf_conv3x3_winograd3_rgb_f32(float* rgb_out, const float* x, const float* u, const float* in_scale, const float* out_scale,
                                             const float* rgb_w, const float* rgb_bias, int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout,
                                             int32_t out_scale_stride, int32_t rgb_channels, mgf_stream_t stream) {
    MGF_REQUIRE(rgb_out, MGF_EINVAL, "conv3x3_winograd3_rgb: null output");
    return launch_wino3(nullptr, x, u, in_scale, out_scale, n, cin, h, w, cout, out_scale_stride, nullptr, rgb_w, rgb_bias, rgb_out, rgb_channels, stream);
}
