// The max pools of the LPIPS backbones (lpips/pretrained_networks.py), forward and backward: MaxPool2d(3, 2, ceil_mode=True) (SqueezeNet) with
// or without each window's winning tap, MaxPool2d(2 | 3, 2) floor mode (VGG, AlexNet).  The gradient of a window goes to its FIRST maximum in
// row-major order (torch's argmax rule); every output element is written by one lane, bit-reproducible.
//   mgf_maxpool3x3s2_ceil_f32 / _idx_f32           forward; _idx also stores the winning tap, one byte per output
//   mgf_maxpool3x3s2_ceil_bwd_f32 / _bwd_idx_f32   backward from the input map / from the stored taps
//   mgf_maxpool_s2_floor_f32 / _bwd_f32            floor mode, k = 2 | 3
// Contract: include/mgf.h.
#include "mgf_common.h"

namespace {

// a 3 x 3 window's tap as the idx forwards store it and maxpool3x3s2_bwd_idx_kernel reads it: row-major, 0..8
__host__ __device__ constexpr int pool_tap(int row, int col) { return 3 * row + col; }

// K x K window, stride 2, windows clipped at the bottom/right edge (ceil_mode partial windows).  A workgroup covers 4 output rows of one
// plane; a thread produces TWO adjacent outputs from a K x (K + 2) input window, so a wave reads 3 contiguous row segments (every byte
// of them used) and no index needs a division per element (one per workgroup row).  HBM-bound: in + out bytes once.
// IDX (K = 3): also the window's first maximum in row-major order as a tap index 0..8 (torch's rule for the gradient), one byte per
// output -- gradient mode's backward then needs neither the input map nor the 9-tap scan (mgf_maxpool3x3s2_ceil_bwd_idx_f32).
template <int K, bool IDX = false>
__global__ __launch_bounds__(256) void maxpool_kernel(float* y, const float* x, int nc, int in_h, int in_w, int out_h, int out_w,
                                                      uint8_t* idx = nullptr) {
    static_assert(!IDX || K == 3, "pool_tap numbers the taps of a 3 x 3 window");
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);              // (plane, output row) flattened
    if (row >= nc * out_h) return;
    const int pl = row / out_h, oy = row - pl * out_h;
    const float* xp = x + (int64_t)pl * in_h * in_w;
    float* yp = y + ((int64_t)pl * out_h + oy) * out_w;
    const int lane = threadIdx.x & 63;
    for (int ox = 2 * lane; ox < out_w; ox += 128) {
        float m0 = -3.0e38f, m1 = -3.0e38f;
        int t0 = 0, t1 = 0;
#pragma unroll
        for (int dy = 0; dy < K; ++dy) {
            const int iy = oy * 2 + dy;
            if (iy >= in_h) continue;
            const float* rp = xp + (int64_t)iy * in_w + 2 * ox;
            float v[K + 2];
#pragma unroll
            for (int dx = 0; dx < K + 2; ++dx) v[dx] = (2 * ox + dx < in_w) ? rp[dx] : -3.0e38f;
#pragma unroll
            for (int dx = 0; dx < K; ++dx) {
                if (IDX) {                                               // strict >: the first maximum wins; tap (0, 0) always exists
                    if (v[dx] > m0) { m0 = v[dx]; t0 = pool_tap(dy, dx); }
                    if (v[dx + 2] > m1) { m1 = v[dx + 2]; t1 = pool_tap(dy, dx); }
                } else {
                    m0 = fmaxf(m0, v[dx]); m1 = fmaxf(m1, v[dx + 2]);
                }
            }
        }
        yp[ox] = m0;
        if (IDX) idx[((int64_t)pl * out_h + oy) * out_w + ox] = (uint8_t)t0;
        if (ox + 1 < out_w) {
            yp[ox + 1] = m1;
            if (IDX) idx[((int64_t)pl * out_h + oy) * out_w + ox + 1] = (uint8_t)t1;
        }
    }
}

// 3x3 / stride-2 ceil-mode pool through LDS: 64 x 8 outputs per workgroup from a 129 x 17 input patch loaded by rows, two outputs per
// lane -- for maps wider than the 512 columns maxpool3x3s2_rows_kernel keeps in registers.  Same 2.9 TB/s as the row-per-wave form on
// the large maps (3.1 against 2.45 on 127^2): what the pool wants is neither -- see maxpool3x3s2_rows_kernel.
__global__ __launch_bounds__(256) void maxpool3x3s2_tiled_kernel(float* __restrict__ y, const float* __restrict__ x, int in_h, int in_w, int out_h,
                                                                 int out_w, int tiles_x, int tiles_y) {
    constexpr int TW = 64, TH = 8, PW = 2 * TW + 1, PH = 2 * TH + 1;
    __shared__ float patch[PH][PW + 1];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y;
    const int64_t pl = blockIdx.x / ((int64_t)tiles_x * tiles_y);
    const int ox0 = tx * TW, oy0 = ty * TH, ix0 = 2 * ox0, iy0 = 2 * oy0;
    const float* xp = x + pl * in_h * in_w;
    const float NEG = -3.0e38f;
    {
        const int cc = tid & 127, ix = ix0 + cc;
        const bool xin = ix < in_w;
#pragma unroll
        for (int r = tid >> 7; r < PH; r += 2) {
            const int iy = iy0 + r;
            patch[r][cc] = (xin && iy < in_h) ? xp[(int64_t)iy * in_w + ix] : NEG;
        }
        if (tid < PH) {                                              // the 129th column
            const int iy = iy0 + tid, ix2 = ix0 + 128;
            patch[tid][128] = (ix2 < in_w && iy < in_h) ? xp[(int64_t)iy * in_w + ix2] : NEG;
        }
    }
    __syncthreads();
    const int lx = tid & 63;
    if (ox0 + lx >= out_w) return;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int ly = (tid >> 6) + 4 * q;
        const int oy = oy0 + ly;
        if (oy >= out_h) break;
        float m = NEG;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, patch[2 * ly + dy][2 * lx + dx]);
        y[(pl * out_h + oy) * out_w + ox0 + lx] = m;
    }
}

// What the strided window costs (tools/maxpool_fwd_micro.py, 25 x 64 x 511^2): five overlapping 4-byte loads per row and output pair at
// a lane stride of 8 bytes ran at 2.9 TB/s, two non-overlapping ones (wrong results) at 4.4, without the stores still 2.9; a read-only
// stream reaches 6 TB/s (tools/probes/hbm_read.hip).  So:
// 3x3 / stride-2 ceil-mode pool, one wave per output row with every input element loaded ONCE per wave and fully coalesced: lane l holds
// the column-wise maximum of the row's three input rows at columns l, l + 64, ... (S slots), the stride-2 three-wide windows are
// then formed across lanes (two shuffles per slot; the last lanes of a slot take the next slot's first ones) and the even lanes store.
// IDX: also each window's first maximum in row-major order as a tap index (torch's gradient rule): the column maximum remembers its
// first row, and among the window's columns with the maximal value the smallest row, then the smallest column, wins.
template <int S, bool IDX = false>
__global__ __launch_bounds__(256) void maxpool3x3s2_rows_kernel(float* __restrict__ y, const float* __restrict__ x, int nc, int in_h, int in_w,
                                                                int out_h, int out_w, uint8_t* __restrict__ idx = nullptr) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);              // (plane, output row) flattened
    if (row >= nc * out_h) return;
    const int pl = row / out_h, oy = row - pl * out_h;
    const int lane = threadIdx.x & 63;
    const float* xp = x + (int64_t)pl * in_h * in_w + (int64_t)(2 * oy) * in_w;
    const float NEG = -3.0e38f;
    const bool r1 = 2 * oy + 1 < in_h, r2 = 2 * oy + 2 < in_h;
    float v[S + 1];
    int rw[IDX ? S + 1 : 1];                                         // IDX: first row of the column maximum
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int e = 64 * s + lane;
        const bool in = e < in_w;
        const float a = in ? xp[e] : NEG, b = (in && r1) ? xp[in_w + e] : NEG, c = (in && r2) ? xp[2 * in_w + e] : NEG;
        if (IDX) {
            float m = a; int r = 0;
            if (b > m) { m = b; r = 1; }
            if (c > m) { m = c; r = 2; }
            v[s] = m; rw[s] = r;
        } else {
            v[s] = fmaxf(fmaxf(a, b), c);
        }
    }
    v[S] = NEG;
    if (IDX) rw[S] = 0;
    float* yp = y + ((int64_t)pl * out_h + oy) * out_w;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const float t1 = __shfl(v[s], (lane + 1) & 63), n1 = __shfl(v[s + 1], (lane + 1) & 63);
        const float t2 = __shfl(v[s], (lane + 2) & 63), n2 = __shfl(v[s + 1], (lane + 2) & 63);
        const float c1 = lane < 63 ? t1 : n1, c2 = lane < 62 ? t2 : n2;
        const int ox = 32 * s + (lane >> 1);
        const bool st = !(lane & 1) && ox < out_w;
        if (IDX) {
            const int q1 = __shfl(rw[s], (lane + 1) & 63), p1 = __shfl(rw[s + 1], (lane + 1) & 63);
            const int q2 = __shfl(rw[s], (lane + 2) & 63), p2 = __shfl(rw[s + 1], (lane + 2) & 63);
            const int w1 = lane < 63 ? q1 : p1, w2 = lane < 62 ? q2 : p2;
            float m = v[s]; int r = rw[s], dx = 0;
            if (c1 > m || (c1 == m && w1 < r)) { m = c1; r = w1; dx = 1; }
            if (c2 > m || (c2 == m && w2 < r)) { m = c2; r = w2; dx = 2; }
            if (st) { yp[ox] = m; idx[((int64_t)pl * out_h + oy) * out_w + ox] = (uint8_t)pool_tap(r, dx); }
        } else {
            if (st) yp[ox] = fmaxf(fmaxf(v[s], c1), c2);
        }
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

// dx of the 3x3 / stride-2 ceil-mode pool from the forward's stored tap indices: one lane per 2 x 2 input block (2 bi, 2 bj) + {0,1}^2,
// whose elements sit at fixed taps (pool_tap(row, column)) of the <= 4 windows around it -- (0,0): tap (2,2) of window (bi-1, bj-1), (2,0) of
// (bi-1, bj), (0,2) of (bi, bj-1), (0,0) of (bi, bj); (0,1): (2,1) of (bi-1, bj), (0,1) of (bi, bj); (1,0): (1,2) of (bi, bj-1), (1,0) of
// (bi, bj); (1,1): (1,1) of (bi, bj) -- summed in ascending window order like torch.  No LDS, no input map: a stream of stores.
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
    if (t[0][0] == pool_tap(2, 2)) e00 += g[0][0];
    if (t[0][1] == pool_tap(2, 0)) e00 += g[0][1];
    if (t[1][0] == pool_tap(0, 2)) e00 += g[1][0];
    if (t[1][1] == pool_tap(0, 0)) e00 += g[1][1];
    if (t[0][1] == pool_tap(2, 1)) e01 += g[0][1];
    if (t[1][1] == pool_tap(0, 1)) e01 += g[1][1];
    if (t[1][0] == pool_tap(1, 2)) e10 += g[1][0];
    if (t[1][1] == pool_tap(1, 0)) e10 += g[1][1];
    if (t[1][1] == pool_tap(1, 1)) e11 += g[1][1];
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

// Kernel choice of the ceil-mode forward: the rows kernel for 64 <= in_w <= 512; else, without IDX, the tiled kernel once a row of tiles is
// half full and the tile count fits a grid (the idx forward has no tiled form); else the generic kernel.
template <bool IDX>
static int pool3x3s2_ceil_launch(const char* what, float* y, uint8_t* idx, const float* x, int32_t nc, int32_t in_h, int32_t in_w, int32_t out_h,
                                 int32_t out_w, hipStream_t st) {
    MGF_REQUIRE(y && (idx || !IDX) && x && nc >= 1 && in_h >= 1 && in_w >= 1, MGF_EINVAL, "%s: bad arguments", what);
    // ceil_mode output size; the last window must start inside the input (torch.nn.MaxPool2d rule)
    auto osz = [](int in) { int o = (in - 3 + 1) / 2 + 1; if ((o - 1) * 2 >= in) --o; return o; };
    MGF_REQUIRE(out_h == osz(in_h) && out_w == osz(in_w), MGF_EINVAL, "%s: output must be %dx%d (got %dx%d)", what, osz(in_h), osz(in_w), out_h,
                out_w);
    MGF_REQUIRE((int64_t)nc * out_h <= INT32_MAX - 4, MGF_ETOOBIG, "%s: too many rows", what);
    const dim3 row_grid((unsigned)mgf_cdiv((int64_t)nc * out_h, 4));
    static const int rows_env = [] { const char* e = mgf_knob("MGF_POOL_ROWS"); return e ? atoi(e) : -1; }();
    static const int tiled_env = [] { const char* e = mgf_knob("MGF_POOL_TILED"); return e ? atoi(e) : -1; }();
    const int64_t tiles = (int64_t)nc * mgf_cdiv(out_w, 64) * mgf_cdiv(out_h, 8);
    if (rows_env != 0 && in_w <= 512 && in_w >= 64) {
#define MGF_POOL_ROWS(SL) hipLaunchKernelGGL((maxpool3x3s2_rows_kernel<SL, IDX>), row_grid, dim3(256), 0, st, y, x, nc, in_h, in_w, out_h, out_w, idx)
        switch ((int)mgf_cdiv(in_w, 64)) {
            case 1: MGF_POOL_ROWS(1); break; case 2: MGF_POOL_ROWS(2); break; case 3: MGF_POOL_ROWS(3); break; case 4: MGF_POOL_ROWS(4); break;
            case 5: MGF_POOL_ROWS(5); break; case 6: MGF_POOL_ROWS(6); break; case 7: MGF_POOL_ROWS(7); break; default: MGF_POOL_ROWS(8); break;
        }
#undef MGF_POOL_ROWS
    } else if (!IDX && tiled_env != 0 && out_w >= 32 && tiles <= INT32_MAX) {
        hipLaunchKernelGGL(maxpool3x3s2_tiled_kernel, dim3((unsigned)tiles), dim3(256), 0, st, y, x, in_h, in_w, out_h, out_w,
                           (int)mgf_cdiv(out_w, 64), (int)mgf_cdiv(out_h, 8));
    } else {
        hipLaunchKernelGGL((maxpool_kernel<3, IDX>), row_grid, dim3(256), 0, st, y, x, nc, in_h, in_w, out_h, out_w, idx);
    }
    MGF_CHECK_LAUNCH(what);
    return MGF_OK;
}

extern "C" int mgf_maxpool3x3s2_ceil_f32(float* y, const float* x, int32_t nc, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                                         mgf_stream_t stream) {
    return pool3x3s2_ceil_launch<false>("maxpool", y, nullptr, x, nc, in_h, in_w, out_h, out_w, (hipStream_t)stream);
}

extern "C" int mgf_maxpool3x3s2_ceil_idx_f32(float* y, uint8_t* idx, const float* x, int32_t nc, int32_t in_h, int32_t in_w, int32_t out_h,
                                             int32_t out_w, mgf_stream_t stream) {
    return pool3x3s2_ceil_launch<true>("maxpool_idx", y, idx, x, nc, in_h, in_w, out_h, out_w, (hipStream_t)stream);
}

extern "C" int mgf_maxpool_s2_floor_f32(float* y, const float* x, int32_t nc, int32_t in_h, int32_t in_w, int32_t ksize, mgf_stream_t stream) {
    MGF_REQUIRE(y && x && nc >= 1 && (ksize == 2 || ksize == 3) && in_h >= ksize && in_w >= ksize, MGF_EINVAL, "maxpool_s2_floor: bad arguments");
    const int out_h = (in_h - ksize) / 2 + 1, out_w = (in_w - ksize) / 2 + 1;
    MGF_REQUIRE((int64_t)nc * out_h <= INT32_MAX - 4, MGF_ETOOBIG, "maxpool_s2_floor: too many rows");
    const dim3 grid((unsigned)mgf_cdiv((int64_t)nc * out_h, 4));
    if (ksize == 2) hipLaunchKernelGGL(maxpool_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, y, x, nc, in_h, in_w, out_h, out_w);
    else hipLaunchKernelGGL(maxpool_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, y, x, nc, in_h, in_w, out_h, out_w);
    MGF_CHECK_LAUNCH("maxpool_s2_floor");
    return MGF_OK;
}

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
