// The up-sampling half of a synthesis block in one launch: stride-2 transposed 3x3 conv (FP32 matrix cores, the tap-list kernel's MODE 1
// arithmetic: 9 taps into 4 output-parity accumulator sets) + the separable 4-tap blur with padding 1 + noise / bias / leaky ReLU / gain.
// Contract: include/mgf.h (mgf_tconv3x3s2_blur_f32).  Replaces conv_taps_kernel<1,2,1,true,10> + tconv_border_kernel + fir_up1_stream on
// the layers conv.tconv_blur_ok accepts: the [n, cout, 2h+1, 2w+1] intermediate t is never written to memory or read back.
//
// Strip walk.  A workgroup (4 waves) owns one 32-channel tile and one vertical strip of the input map and walks it top to bottom in steps
// of 8 input rows.  The 32 lanes of an MFMA pixel row are 32 input columns j0 - 1 .. j0 + 30 of which the strip OWNS the middle 30: lane l
// holds t columns 2j, 2j + 1 (j = j0 - 1 + l) in its parity accumulators, and the blur of an owned lane's two outputs needs t columns
// 2j - 1 .. 2j + 3, i.e. the odd column of lane l - 1 and both columns of lane l + 1 -- three DPP wave shifts, no LDS.  Input row h and
// column w (and everything outside the map) are staged as zeros, so row 2h / column 2w of t -- the border launch of the unfused path --
// fall out of the walk.
// A step produces t rows 16 s .. 16 s + 15 (wave v: rows 4 v .. 4 v + 3 of them); y row R needs t rows R - 1 .. R + 2, so the step emits
// y rows 16 s - 2 .. 16 s + 13 and the horizontally filtered rows 16 s + 13 .. 16 s + 15 are CARRIED in LDS to the next step.  The vertical
// pass goes through LDS one slice of 8 channels at a time (4 accumulator registers x 2 lane halves: 16 rows x 64 columns x 8 channels =
// 32 KB, placed over the conv's staging buffers, which are idle between two steps): horizontal pass from registers -> LDS -> barrier ->
// each wave reads 7 rows x 64 columns per channel (one float2 per lane, the lane halves on two channels), forms its 4 output rows, applies
// the epilogue and stores 240-byte row segments.
//
// Work split.  The units (sample, strip, channel tile, step) -- channel tile fastest among the items, so the tiles of one strip sit side
// by side -- form one flat list that is cut into equal contiguous ranges, one per resident workgroup (2 per CU); ranges are handed out so
// that each XCD walks one contiguous eighth of the list.  A range that begins in the middle of a strip first runs the step above it with
// its stores suppressed, which fills the carry (one extra step per workgroup, ~1.4 % at 1024^2).  No sum depends on where a range begins
// or on n: every output is the same chain of fmas whichever workgroup forms it.
// The register / LDS pipeline of the K loop is the tap-list kernel's (csrc/conv_taps.hip): chunks of 8 input channels, two LDS buffers,
// the loads of chunk i + 1 in flight behind the MFMAs of chunk i; the first chunk of the NEXT unit is requested behind the last MFMA phase
// and is in flight during the blur, whose stores in turn drain under the next unit's matrix work.
#include "mgf_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CK = 8;                       // input channels per K chunk
// Timing ablations (tools/tconv_blur_abl.sh; experiment builds only -- the results are wrong): 1 = no blur and no stores (staging and matrix
// phases alone), 2 = no halo columns (a strip owns all 32 lanes), 4 = the blur without its global stores.  Bits add.
#ifndef MGF_TB_ABL
#define MGF_TB_ABL 0
#endif
constexpr int OWN = (MGF_TB_ABL & 2) ? 32 : 30;          // owned input columns of a 32-lane strip
constexpr int FW = 33, FH = 9, CHS = FH * FW;             // footprint of a step: 9 input rows x 33 columns per channel
constexpr int XS = 10, WS = 3;              // per-lane staging slots: 8 * 297 = 2376 floats of x, 9 * 8 * 32 / 4 = 576 float4 of weights
constexpr int XS_REGION = XS * 256, BUF = XS_REGION + WS * 1024;          // floats per LDS buffer
constexpr int SLICE = 8 * 16 * 64;          // floats of one vertical-pass slice (over the two staging buffers)
constexpr int CARRY = 32 * 3 * 64;          // carried rows: [channel 32][row 3][column 64]
constexpr int LDS_FLOATS = 2 * BUF + CARRY + 64;
static_assert(SLICE <= 2 * BUF, "the slice lives in the staging buffers");
static_assert(LDS_FLOATS * 4 <= 80 * 1024, "two workgroups per CU");

struct Ones8 { float v[8]; };
__device__ const Ones8 g_ones8 = {{1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f}};

struct TBParams {
    float* y;
    const float* x;
    const float* wp;
    const float* in_scale;
    const float* out_scale;
    const float* f1d;
    float gain;
    int n, cin, h, w, cout_pad;
    int y_pitch, y_plane;
    int64_t y_batch, os_stride;
    mgf_epilogue ep;
    int strips, cot, steps;          // strips per map, channel tiles, steps per strip
    int total, per;                  // units in all, units per workgroup
};

struct Unit { int n, co0, j0, s; };

// (bound_ctrl: the lane without a source reads 0 -- lanes 0 and 63 are halo lanes whose results are never stored -- and the destination
// needs no initial value, i.e. no v_mov in front of every shift)
__device__ __forceinline__ float dpp_from_left(float v) {        // lane i <- lane i - 1 (wave_shr:1)
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float dpp_from_right(float v) {       // lane i <- lane i + 1 (wave_shl:1)
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x130, 0xf, 0xf, true));
}

__global__ __launch_bounds__(256, 2) void tconv_blur_kernel(TBParams p) {
    extern __shared__ float lds[];
    float* const carry = lds + 2 * BUF;
    float* const prm = carry + CARRY;                 // [0, 32): out_scale of the tile's channels, [32, 64): bias
    const int tid = threadIdx.x, tid_ = tid, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int plane = p.h * p.w;

    // contiguous range of units of this workgroup; workgroup b runs on XCD b % 8, which walks eighth b % 8 of the list
    const int vb = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
    const int g_begin = vb * p.per;
    int g_end = g_begin + p.per;
    if (g_end > p.total) g_end = p.total;
    if (g_begin >= g_end) return;
    const int u0 = g_begin - ((g_begin % p.steps) != 0 ? 1 : 0);       // the step above a mid-strip start: fills the carry, stores nothing

    auto decode = [&](int u, Unit& c) {
        const int item = u / p.steps;
        c.s = u - item * p.steps;
        const int ct = item % p.cot;
        const int r = item / p.cot;
        const int strip = r % p.strips;
        c.n = r / p.strips;
        c.co0 = ct * 32;
        c.j0 = strip * OWN;
        c.n = __builtin_amdgcn_readfirstlane(c.n); c.co0 = __builtin_amdgcn_readfirstlane(c.co0);
        c.j0 = __builtin_amdgcn_readfirstlane(c.j0); c.s = __builtin_amdgcn_readfirstlane(c.s);
    };

    // folded filter constants, as fir_up1_stream: f / f[0] horizontally (its last tap is exactly 1), f * f[0] * gain vertically
    float fx[3], fy[4];
    {
        const float f0 = p.f1d[0];
#pragma unroll
        for (int t = 0; t < 3; ++t) fx[t] = p.f1d[3 - t] / f0;
#pragma unroll
        for (int t = 0; t < 4; ++t) fy[t] = p.f1d[3 - t] * f0 * p.gain;
    }

    f32x16 acc[4][2];
    auto zero_acc = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[q][g][r] = 0.f;
    };
    zero_acc();

    // ---- staging (conv_taps.hip's scheme): one 32-bit byte offset per slot, fixed for the unit; padding slots carry an offset past the
    // buffer's size and arrive as zeros; the chunk's channel offset rides in the scalar operand ----
    unsigned xoff[XS];
    int woff[WS], wch[WS];
    __amdgpu_buffer_rsrc_t rx_l = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw_l = __builtin_amdgcn_make_buffer_rsrc((void*)p.wp, 0, (int)(4u * (unsigned)(9 * p.cin * p.cout_pad)), 0x00020000);
    __amdgpu_buffer_rsrc_t rs_l = __builtin_amdgcn_make_buffer_rsrc((void*)g_ones8.v, 0, 32, 0x00020000);
    const int sc_step = p.in_scale ? 4 : 0;
    auto setup_slots = [&](const Unit& c) {
        rx_l = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + (int64_t)c.n * p.cin * plane), 0, (int)(4u * (unsigned)(p.cin * plane)), 0x00020000);
        if (p.in_scale) rs_l = __builtin_amdgcn_make_buffer_rsrc((void*)(p.in_scale + (int64_t)c.n * p.cin), 0, 4 * p.cin, 0x00020000);
        // an opaque copy of the thread index: the slot coordinates below depend on it alone, and hoisted out of the unit loop they would
        // sit in ~ 40 registers across the matrix phases (they spill); recomputed per unit they cost ~ 150 vector instructions per step
        int tid = tid_;
        asm volatile("" : "+v"(tid));
#pragma unroll
        for (int j = 0; j < WS; ++j) {
            int i = tid + 256 * j;
            if (i >= 576) i = 575;                    // surplus slots re-read the last row into the padded LDS tail
            const int c4 = i & 7, rest = i >> 3;
            wch[j] = rest & 7;
            woff[j] = ((rest >> 3) * p.cin + wch[j]) * p.cout_pad + c.co0 + c4 * 4;
        }
        const int iy0 = c.s * 8 - 1, ix0 = c.j0 - 2;
#pragma unroll
        for (int j = 0; j < XS; ++j) {
            const int i = tid + 256 * j;
            const int ch = i / CHS, rem = i - ch * CHS;
            const int r = rem / FW, q = rem - r * FW;
            const int iy = iy0 + r, ix = ix0 + q;
            xoff[j] = (i < CK * CHS && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w) ? 4u * (unsigned)(ch * plane + iy * p.w + ix) : 0xFFFFFFF0u;
        }
    };
    float xr[XS];
    float4 wr[WS];
    float wsc[WS];
    auto load_chunk = [&](int c0) {
        const int xso = (int)(4u * (unsigned)(c0 * plane)), wso = (int)(4u * (unsigned)(c0 * p.cout_pad)), sso = c0 * sc_step;
#pragma unroll
        for (int j = 0; j < XS; ++j) xr[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx_l, xoff[j], xso, 0));
#pragma unroll
        for (int j = 0; j < WS; ++j) {
            wr[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rw_l, 4u * (unsigned)woff[j], wso, 0));
            wsc[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_l, 4u * (unsigned)wch[j], sso, 0));
        }
    };
    auto store_chunk = [&](float* buf) {
#pragma unroll
        for (int j = 0; j < XS; ++j) buf[tid + 256 * j] = xr[j];
        float* Wd = buf + XS_REGION;
#pragma unroll
        for (int j = 0; j < WS; ++j) {
            float4 v = wr[j];
            v.x *= wsc[j]; v.y *= wsc[j]; v.z *= wsc[j]; v.w *= wsc[j];       // the style rides on the weight rows (w * s)
            *reinterpret_cast<float4*>(Wd + (tid + 256 * j) * 4) = v;
        }
    };
    // MFMA phase of one chunk: operand fragments one tap ahead of the MFMAs that consume them, reads interleaved with the matrix stream
    const int pb0 = (wave * 2) * FW + l31, pb1 = pb0 + FW;
    auto mfma_chunk = [&](const float* buf) {
        auto toff = [](int t) { return ((t / 3) == 2 ? 0 : FW) + ((t % 3) == 2 ? 0 : 1); };
        const float* Xs = buf + half * CHS;
        const float* Ws = buf + XS_REGION + half * 32 + l31;
        float fa[2][CK / 2], fb[2][CK / 2][2];
        auto fetch = [&](int t, int set) {
#pragma unroll
            for (int kk = 0; kk < CK / 2; ++kk) {
                fa[set][kk] = Ws[(t * CK + 2 * kk) * 32];
                fb[set][kk][0] = Xs[2 * kk * CHS + pb0 + toff(t)];
                fb[set][kk][1] = Xs[2 * kk * CHS + pb1 + toff(t)];
            }
        };
        fetch(0, 0);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            if (t + 1 < 9) {
                fetch(t + 1, (t + 1) & 1);
#pragma unroll
                for (int i = 0; i < (CK / 2) * 3; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     // 1 MFMA
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);     // 1 DS read
                }
            }
            const int q = ((t / 3) == 1 ? 2 : 0) + ((t % 3) == 1 ? 1 : 0);      // parity set of tap t (kh == 1: odd rows, kw == 1: odd columns)
#pragma unroll
            for (int kk = 0; kk < CK / 2; ++kk)
#pragma unroll
                for (int g = 0; g < 2; ++g)
                    acc[q][g] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[t & 1][kk], fb[t & 1][kk][g], acc[q][g], 0, 0, 0);
        }
    };

    const bool has_noise = p.ep.noise != nullptr;
    const float ep_ns = has_noise ? (p.ep.noise_strength ? *p.ep.noise_strength : 1.0f) : 0.f;
    const float alpha = p.ep.act == MGF_ACT_LRELU ? p.ep.alpha : 1.0f, egain = p.ep.gain;
    const int out_h = 2 * p.h, out_w = 2 * p.w;

    // ---- blur + epilogue of one finished step ----
    auto blur = [&](const Unit& c, bool emit) {
        float2 nz[4];
        float* const S = lds;
        // vertical pass coordinates of this lane: t columns 2 l31, 2 l31 + 1 of the strip's 64 (one float2), output rows 16 s - 2 + 4 wave +
        // {0 .. 3}; the lane halves take the even / odd channel of a pair
        const int ycol = 2 * (c.j0 - 1) + 2 * l31;
        const bool col_ok = (MGF_TB_ABL & 2) ? (ycol >= 0 && ycol < out_w) : (l31 >= 1 && l31 < 31 && ycol < out_w);
        const int R0 = 16 * c.s - 2 + 4 * wave;
        float* const yb = p.y + (int64_t)c.n * p.y_batch + (int64_t)c.co0 * p.y_plane;
        // byte offset of this lane's four output pairs inside the plane of its channel of pair 0 (the pair's channel rides in the buffer
        // base); a masked output carries an offset past everything and the buffer store drops it (no branch, no 64-bit address arithmetic)
        uint32_t yo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = emit && col_ok && R0 + j >= 0 && R0 + j < out_h && !(MGF_TB_ABL & 4);
            yo[j] = ok ? 4u * (uint32_t)(half * p.y_plane + (R0 + j) * p.y_pitch + ycol) : 0xFFFFFFF0u;
        }
        // rows 0 .. 6 of this wave's window: S rows 4 wave - 3 + i -- for wave 0, i < 3: the carry
        const int laneS = (half * 16 + 4 * wave - 3) * 64 + 2 * l31, laneC = 2 * BUF + half * 192 + 2 * l31;
        const int laneLow = wave == 0 ? laneC : laneS;
        // horizontal pass addresses: lane (l31, half) writes the float2 of t columns 2 l31, 2 l31 + 1
        float* const Sw = S + ((4 * half) * 16 + 4 * wave) * 64 + 2 * l31;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const float E = acc[2 * a][g][4 * k + rr], O = acc[2 * a + 1][g][4 * k + rr];
                        const float Ol = dpp_from_left(O), Er = dpp_from_right(E), Or = dpp_from_right(O);
                        float he = __builtin_fmaf(fx[2], O, Er);
                        he = __builtin_fmaf(fx[1], E, he);
                        he = __builtin_fmaf(fx[0], Ol, he);
                        float ho = __builtin_fmaf(fx[2], Er, Or);
                        ho = __builtin_fmaf(fx[1], O, ho);
                        ho = __builtin_fmaf(fx[0], E, ho);
                        // (opaque: keeps the SLP vectoriser from pairing the two chains into v_pk_fma_f32 behind a pile of v_mov --
                        // packed float32 arithmetic is an anti-lever beside the other workgroup's MFMAs)
                        asm("" : "+v"(he), "+v"(ho));
                        *reinterpret_cast<float2*>(Sw + (rr * 16 + 2 * g + a) * 64) = make_float2(he, ho);
                    }
            if (k == 0) {
                // the noise of this lane's four outputs (one read per row and workgroup: every channel of the tile uses it),
                // requested behind the first horizontal pass -- not held across the K loop -- and consumed behind the barrier
#pragma unroll
                for (int j = 0; j < 4; ++j) nz[j] = make_float2(0.f, 0.f);
                if (has_noise) {
                    const int ycol = 2 * (c.j0 - 1) + 2 * l31;
                    const int R0 = 16 * c.s - 2 + 4 * wave;
                    const float* nb = p.ep.noise + (int64_t)(p.ep.noise_n > 1 ? c.n : 0) * out_h * out_w;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (l31 >= 1 && l31 < 31 && ycol < out_w && R0 + j >= 0 && R0 + j < out_h) {
                            const float* q = nb + (int64_t)(R0 + j) * out_w + ycol;
                            nz[j] = make_float2(q[0] * ep_ns, q[1] * ep_ns);
                        }
                }
            }
            __syncthreads();
            // channel pairs (2 it, 2 it + 1) of the slice, one per lane half; the reads of the next pair are issued in front of the
            // arithmetic of this one
            float2 Bn[7];
            float2 pn;
            auto fetch_rows = [&](int it) {
                const int lowoff = wave == 0 ? ((8 * k + 2 * it) * 3) * 64 : (2 * it * 16) * 64;
#pragma unroll
                for (int i = 0; i < 7; ++i)
                    Bn[i] = *reinterpret_cast<const float2*>(i < 3 ? lds + laneLow + lowoff + i * 64 : S + laneS + (2 * it * 16 + i) * 64);
                pn = make_float2(prm[8 * k + 2 * it + half], prm[32 + 8 * k + 2 * it + half]);
            };
            fetch_rows(0);
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                float2 B[7];
#pragma unroll
                for (int i = 0; i < 7; ++i) B[i] = Bn[i];
                const float dsc = pn.x, bia = pn.y;
                if (it + 1 < 4) fetch_rows(it + 1);
                const int ch = 8 * k + 2 * it;
                const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)(yb + (int64_t)ch * p.y_plane), 0, 8 * p.y_plane, 0x00020000);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float o0 = B[j].x * fy[0], o1 = B[j].y * fy[0];
                    o0 = __builtin_fmaf(B[j + 1].x, fy[1], o0); o1 = __builtin_fmaf(B[j + 1].y, fy[1], o1);
                    o0 = __builtin_fmaf(B[j + 2].x, fy[2], o0); o1 = __builtin_fmaf(B[j + 2].y, fy[2], o1);
                    o0 = __builtin_fmaf(B[j + 3].x, fy[3], o0); o1 = __builtin_fmaf(B[j + 3].y, fy[3], o1);
                    float v0 = __builtin_fmaf(o0, dsc, nz[j].x), v1 = __builtin_fmaf(o1, dsc, nz[j].y);
                    v0 += bia; v1 += bia;
                    v0 = __builtin_fmaxf(v0, v0 * alpha);       // leaky ReLU for 0 <= alpha <= 1 (host-checked); linear: alpha = 1
                    v1 = __builtin_fmaxf(v1, v1 * alpha);
                    v0 *= egain; v1 *= egain;
                    asm("" : "+v"(v0), "+v"(v1));               // (no v_pk_* pairing, as above)
                    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                    u32x2 pk = {__builtin_bit_cast(unsigned, v0), __builtin_bit_cast(unsigned, v1)};
                    __builtin_amdgcn_raw_buffer_store_b64(pk, ry, yo[j], 0, 0);
                }
            }
            __syncthreads();
            if (wave == 3) {
                // Rows 13 .. 15 of the slice become the carry of these 8 channels.  Only this wave writes those rows of S (and does so again
                // only in its own next horizontal pass, behind these reads), and wave 0 has read the old carry in front of the barrier.
                // Lane halves take rows i and i + 1 of the 8 x 3 row list, 32 float2 each.
#pragma unroll
                for (int e = 0; e < 12; ++e) {
                    const int row = 2 * e + half, cl = row / 3, i = row - 3 * cl;
                    const float2 v = *reinterpret_cast<const float2*>(S + (cl * 16 + 13 + i) * 64 + 2 * l31);
                    *reinterpret_cast<float2*>(carry + ((8 * k + cl) * 3 + i) * 64 + 2 * l31) = v;
                }
            }
            if (k == 3) __syncthreads();               // the next unit's first chunk is about to be stored over S: wave 3 has to be done reading
        }
    };

    Unit cur;
    decode(u0, cur);
    int b = 0;
    setup_slots(cur);
    load_chunk(0);
    store_chunk(lds);
    __syncthreads();
    const int nch = p.cin / CK;
    for (int u = u0;; ++u) {
        if (cur.s == 0 || u == u0) {                  // top of a strip (or of this workgroup's range): nothing above
            for (int i = tid; i < CARRY; i += 256) carry[i] = 0.f;
        }
        if (tid < 32) {
            prm[tid] = p.out_scale ? p.out_scale[(int64_t)cur.n * p.os_stride + cur.co0 + tid] : 1.0f;
            prm[32 + tid] = p.ep.bias ? p.ep.bias[cur.co0 + tid] : 0.f;
        }
        for (int c = 0; c + 1 < nch; ++c) {
            load_chunk((c + 1) * CK);
            mfma_chunk(lds + b * BUF);
            store_chunk(lds + (b ^ 1) * BUF);
            __syncthreads();
            b ^= 1;
        }
        const bool have_next = u + 1 < g_end;
        Unit nx = cur;
        if (have_next) {
            decode(u + 1, nx);
            setup_slots(nx);
            load_chunk(0);                            // in flight behind the last matrix phase and the blur
        }
        mfma_chunk(lds + b * BUF);
        __syncthreads();                              // the slice buffer lies over both staging buffers
        if (MGF_TB_ABL & 1) {
            if (p.gain == 12345.f) p.y[tid] = acc[0][0][0] + acc[1][1][5] + acc[2][0][10] + acc[3][1][15];      // (keeps the matrix phases alive)
        } else {
            blur(cur, u >= g_begin);
        }
        zero_acc();
        if (!have_next) break;
        store_chunk(lds);
        b = 0;
        __syncthreads();
        cur = nx;
    }
}

}  // namespace

extern "C" int mgf_tconv3x3s2_blur_f32(float* y, const float* x, const float* wp, const float* in_scale, const float* out_scale,
                                       const float* f1d, float gain, int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout,
                                       int32_t cout_pad, int64_t y_pitch, int64_t y_plane, int64_t y_batch, int64_t out_scale_stride,
                                       const mgf_epilogue* ep, mgf_stream_t stream) {
    MGF_REQUIRE(y && x && wp && f1d, MGF_EINVAL, "tconv3x3s2_blur: null pointer");
    MGF_REQUIRE(n >= 1 && cin >= 1 && h >= 1 && w >= 1 && cout >= 1 && cout_pad >= cout, MGF_EINVAL, "tconv3x3s2_blur: bad shape");
    MGF_REQUIRE(cin % CK == 0 && cout % 32 == 0 && cout_pad % 32 == 0, MGF_EUNSUPPORTED,
                "tconv3x3s2_blur: needs cin %% 8 == 0 and cout %% 32 == 0 (got %d, %d)", cin, cout);
    MGF_REQUIRE(y_pitch >= 2 * (int64_t)w && y_plane >= 2 * (int64_t)h * y_pitch && y_batch >= (int64_t)cout * y_plane, MGF_EINVAL,
                "tconv3x3s2_blur: output strides too small");
    MGF_REQUIRE(y_pitch % 2 == 0 && y_plane % 2 == 0 && y_batch % 2 == 0 && ((uintptr_t)y % 8) == 0, MGF_EUNSUPPORTED,
                "tconv3x3s2_blur: output needs even pitch / plane / batch strides and 8-byte alignment (column pairs are stored as float2)");
    // 32-bit byte offsets inside one sample's input and the weight image, 32-bit element offsets inside one channel tile of y
    MGF_REQUIRE((int64_t)cin * h * w < (1LL << 28) && (int64_t)9 * cin * cout_pad < (1LL << 28) && y_plane < (1LL << 28),
                MGF_ETOOBIG, "tconv3x3s2_blur: tensor too large");
    if (ep) {
        MGF_REQUIRE(!ep->residual, MGF_EUNSUPPORTED, "tconv3x3s2_blur: no residual port");
        MGF_REQUIRE(ep->act == 0 || ep->act == MGF_ACT_LINEAR || (ep->act == MGF_ACT_LRELU && ep->alpha >= 0.f && ep->alpha <= 1.f), MGF_EUNSUPPORTED,
                    "tconv3x3s2_blur: epilogue activation %d (slope %g) unsupported", ep->act, (double)ep->alpha);
    }
    TBParams p;
    p.y = y; p.x = x; p.wp = wp; p.in_scale = in_scale; p.out_scale = out_scale; p.f1d = f1d; p.gain = gain;
    p.n = n; p.cin = cin; p.h = h; p.w = w; p.cout_pad = cout_pad;
    p.y_pitch = (int)y_pitch; p.y_plane = (int)y_plane; p.y_batch = y_batch; p.os_stride = out_scale_stride;
    if (ep) { p.ep = *ep; if (p.ep.act == 0) p.ep.act = MGF_ACT_LINEAR; } else { p.ep = mgf_epilogue{}; p.ep.act = MGF_ACT_LINEAR; p.ep.gain = 1.f; }
    p.strips = (int)mgf_cdiv(w, OWN);
    p.cot = cout / 32;
    p.steps = (2 * h + 2 + 15) / 16;
    const int64_t total = (int64_t)n * p.strips * p.cot * p.steps;
    MGF_REQUIRE(total <= INT32_MAX - 4096, MGF_ETOOBIG, "tconv3x3s2_blur: too many work units");
    p.total = (int)total;
    // persistent: at most two workgroups per CU, in multiples of the 8 XCDs
    int64_t grid = (int64_t)MGF_NUM_CU * 2;
    if (total < grid) grid = mgf_cdiv(total, 8) * 8;
    p.per = (int)mgf_cdiv(total, grid);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)tconv_blur_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_FLOATS * 4);
        if (e != hipSuccess) { mgf_set_error("tconv3x3s2_blur: cannot raise dynamic LDS: %s", hipGetErrorString(e)); return MGF_ELAUNCH; }
        attr_set = true;
    }
    hipStream_t st = (hipStream_t)stream;
    // the transposed conv's own FLOPs; algorithmic bytes: x, weights, noise and y once
    const double flops = 2.0 * 9 * cin * (double)cout * h * w * n;
    const double bytes = 4.0 * ((double)n * cin * h * w + 9.0 * cin * cout + ((ep && ep->noise) ? (double)(ep->noise_n > 1 ? n : 1) * 4.0 * h * w : 0.0) +
                                (double)n * cout * 4.0 * h * w);
    mgf_prof_external_begin(st, "tconv_blur_kernel", flops, bytes);
    hipLaunchKernelGGL(tconv_blur_kernel, dim3((unsigned)grid), dim3(256), LDS_FLOATS * 4, st, p);
    mgf_prof_external_end(st);
    MGF_CHECK_LAUNCH("tconv3x3s2_blur");
    return MGF_OK;
}
