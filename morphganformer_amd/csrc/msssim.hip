// Multi-scale SSIM (Wang, Simoncelli, Bovik 2003, as the common libraries implement it) of the UNQUANTISED pixels p = 127.5 img + 127.5,
// q = 127.5 target + 127.5, value and gradient, float64 from the float32 loads on -- the definition is in include/mgf.h (mgf_msssim_f32).
//
// Unlike DSSIM (dssim.hip: dssim_cont_kernel) one pass cannot fuse value and gradient: ms = prod_j v_j^{w_j}, so the coefficient of every level's
// gradient, -scale w_j ms / (v_j c positions_j), needs ALL the level means first.  The launch sequence of one call, all on the caller's stream:
//   1. msssim_pool_kernel      level j -> level j + 1 of both images, 2 x 2 mean with torch's zero padding of an odd side, float64 in scratch
//                              (a shared target, t_batch_stride 0, is reduced once, not once per sample)
//   2. msssim_stats_kernel     per level: a workgroup owns 16 x 16 window positions, loads the 26 x 26 pixels under them, forms the separable
//                              Gaussian sums of p, q, pp, qq, pq (rows, then columns), cs (ssim on the last level) per position and ONE float64
//                              partial per workgroup, tree-summed in a fixed order
//   3. msssim_finish_kernel    partials -> v_j -> ms -> the value and the coefficients (zero where some v_j <= 0: ms = 0 with gradient 0 there)
//   4. msssim_grad_kernel      from the coarsest level to the finest: a workgroup owns 16 x 16 PIXELS, recomputes the statistics of the 26 x 26
//                              positions whose window touches them (36 x 36 pixels; two positions per thread from one 12-value register
//                              window in the row and the column pass), the three maps ga, gb, gc, runs the adjoint Gaussian filter
//                              over rows and columns, adds 1/4 of the parent level's gradient and writes float64 (inner levels) or float32 into
//                              dimg (level 0).  Every pixel has one owner: no atomics, and a second call gives the same bits.
// The gradient kernel's planes in float64 (pixels 2 x 36 x 37, row sums 5 x 36 x 27, maps 3 x 26 x 27) would be 77 KiB; the three maps reuse the
// pixel planes, which are dead once the row sums exist (each thread keeps its own pixel's p and q in registers): 58.8 KiB.
#include "mgf_common.h"
#include <math.h>

constexpr int MS_W = 11, MS_H = MS_W - 1, MS_MAXL = 5;
constexpr int MS_T = 16;                                         // tile side: positions (statistics) or pixels (gradient)
constexpr int MS_SR = MS_T + MS_H;                               // statistics: pixels per side under the tile's positions
constexpr int MS_GP = MS_T + MS_H, MS_GR = MS_GP + MS_H;         // gradient: positions, pixels per side around the tile's pixels

struct MsWin { double g[MS_W]; };                                // the normalised Gaussian taps, by value
struct MsPlan {                                                  // what the finish kernel needs of every level, by value (so a captured launch carries it)
    int64_t part_off[MS_MAXL];                                   // first partial of the level, in doubles from the partials' base
    int32_t tiles[MS_MAXL];
    double positions[MS_MAXL];
    double w[MS_MAXL];
    int32_t levels;
};

struct MsTerms { double s, ga, gb, gc; };
// cs (LAST: ssim = l cs) of one window position and its derivatives by mu_x (ga), E[pp] (gb) and E[pq] (gc)
template <bool LAST>
__device__ __forceinline__ MsTerms ms_terms(double ux, double uy, double exx, double eyy, double exy, double c1, double c2) {
    // the three products stand alone (no fma into the differences below): identical images must give numerator == denominator bit for bit
    const double mxx = __dmul_rn(ux, ux), myy = __dmul_rn(uy, uy), mxy = __dmul_rn(ux, uy);
    const double vx = exx - mxx, vy = eyy - myy, vxy = exy - mxy;
    const double a2 = 2.0 * vxy + c2, b2 = (vx + vy) + c2;
    const double cs = a2 / b2;                                   // (a true quotient: identical images give exactly 1)
    const double rb2 = 1.0 / b2;                                 // the derivatives share one reciprocal: gb = -gc / 2 exactly where cs = 1
    MsTerms t;
    t.s = cs;
    t.ga = 2.0 * (cs * ux - uy) * rb2;
    t.gb = -cs * rb2;
    t.gc = 2.0 * rb2;
    if (LAST) {
        const double a1 = 2.0 * mxy + c1, b1 = (mxx + myy) + c1;
        const double l = a1 / b1;
        t.s = l * cs;
        t.ga = cs * (2.0 * uy - 2.0 * l * ux) * (1.0 / b1) + l * t.ga;
        t.gb = l * t.gb;
        t.gc = l * t.gc;
    }
    return t;
}

__device__ __forceinline__ double ms_pixel(const float* p, int64_t i) { return 127.5 * (double)p[i] + 127.5; }
__device__ __forceinline__ double ms_pixel(const double* p, int64_t i) { return p[i]; }

// ---- 1. the pyramid: dst [planes, ho, wo] = 2 x 2 mean, stride 2, of src [planes, h, w] zero-padded by h % 2 rows / w % 2 columns in front
// (avg_pool2d(x, 2, 2, padding=[h % 2, w % 2]), the pad counted in the divisor); the planes of src are contiguous.
template <typename T>
__global__ __launch_bounds__(256) void msssim_pool_kernel(double* dst, const T* src, int64_t planes, int h, int w, int ho, int wo) {
    const int ph = h & 1, pw = w & 1;
    const int64_t total = planes * ho * wo;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % wo);
        const int64_t t = i / wo;
        const int y = (int)(t % ho);
        const int64_t pl = t / ho;
        const int64_t base = pl * h * w;
        const int r0 = 2 * y - ph, q0 = 2 * x - pw;              // r0 + 1 <= h - 1 and q0 + 1 <= w - 1 always; only the front pad is ever read
        double s = 0.0;
#pragma unroll
        for (int dr = 0; dr < 2; ++dr)
#pragma unroll
            for (int dq = 0; dq < 2; ++dq) {
                const int r = r0 + dr, q = q0 + dq;
                if (r >= 0 && q >= 0 && r < h && q < w) s += ms_pixel(src, base + (int64_t)r * w + q);
            }
        dst[i] = 0.25 * s;
    }
}

// ---- 2. statistics of one level.  grid = (tiles, c, n); part[(n c) tiles] of this level
template <typename T, bool LAST>
__global__ __launch_bounds__(256) void msssim_stats_kernel(double* part, const T* img, const T* tgt, int h, int w, int64_t t_stride, int tiles_x,
                                                           double c1, double c2, MsWin win) {
    __shared__ double px[MS_SR][MS_SR + 1], qx[MS_SR][MS_SR + 1];
    __shared__ double hs[5][MS_SR][MS_T + 1];
    __shared__ double red[256];
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int c = gridDim.y;
    const int64_t plane = (int64_t)h * w;
    const T* a = img + ((int64_t)blockIdx.z * c + blockIdx.y) * plane;
    const T* b = tgt + (int64_t)blockIdx.z * t_stride + (int64_t)blockIdx.y * plane;
    const int r0 = ty * MS_T, q0 = tx * MS_T;
    for (int i = threadIdx.x; i < MS_SR * MS_SR; i += 256) {
        const int r = i / MS_SR, q = i - r * MS_SR;
        const int rr = r0 + r, qq = q0 + q;
        double xv = 0.0, yv = 0.0;
        if (rr < h && qq < w) { xv = ms_pixel(a, (int64_t)rr * w + qq); yv = ms_pixel(b, (int64_t)rr * w + qq); }
        px[r][q] = xv; qx[r][q] = yv;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MS_SR * MS_T; i += 256) {
        const int r = i / MS_T, q = i - r * MS_T;
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
        for (int t = 0; t < MS_W; ++t) {
            const double xv = px[r][q + t], yv = qx[r][q + t], g = win.g[t];
            sx += g * xv; sy += g * yv; sxx += g * (xv * xv); syy += g * (yv * yv); sxy += g * (xv * yv);
        }
        hs[0][r][q] = sx; hs[1][r][q] = sy; hs[2][r][q] = sxx; hs[3][r][q] = syy; hs[4][r][q] = sxy;
    }
    __syncthreads();
    double acc = 0.0;
    const int vh = h - MS_H, vw = w - MS_H;                      // window positions per plane
    {
        const int r = threadIdx.x / MS_T, q = threadIdx.x - r * MS_T;       // 256 threads = the tile's 16 x 16 positions
        if (r0 + r < vh && q0 + q < vw) {
            double s[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                double v = 0.0;
#pragma unroll
                for (int u = 0; u < MS_W; ++u) v += win.g[u] * hs[k][r + u][q];
                s[k] = v;
            }
            acc = ms_terms<LAST>(s[0], s[1], s[2], s[3], s[4], c1, c2).s;
        }
    }
    acc = mgf_block_tree_sum_256(acc, red);
    if (threadIdx.x == 0) part[((int64_t)blockIdx.z * c + blockIdx.y) * gridDim.x + tile] = acc;
}

// ---- 3. grid = n: v_j = sum of the level's partials / positions; per channel ms = prod v_j^{w_j} where every v_j > 0, else 0;
// out = (accumulate ? out : 0) + out_scale * (1 - mean_c ms) as float32; coef[(n c) levels] = -coef_scale w_j ms / (v_j c positions_j), 0 on the
// clamped branch (the libraries' relu-then-power has gradient 0 * inf there; this one is defined as zero)
__global__ __launch_bounds__(256) void msssim_finish_kernel(float* out, double* coef, const double* part, int c, MsPlan plan, float out_scale,
                                                            double coef_scale, int accumulate) {
    __shared__ double red[256];
    double m = 0.0;
    for (int ch = 0; ch < c; ++ch) {
        double v[MS_MAXL];
        bool pos = true;
        double ms = 1.0;
        for (int j = 0; j < plan.levels; ++j) {
            const double* p = part + plan.part_off[j] * gridDim.x * c + ((int64_t)blockIdx.x * c + ch) * plan.tiles[j];
            double s = 0.0;
            for (int i = threadIdx.x; i < plan.tiles[j]; i += 256) s += p[i];
            v[j] = mgf_block_tree_sum_256(s, red) / plan.positions[j];
            if (!(v[j] > 0.0)) pos = false;
        }
        if (pos) {
            for (int j = 0; j < plan.levels; ++j) ms *= pow(v[j], plan.w[j]);
        } else {
            ms = 0.0;
        }
        m += ms;
        if (threadIdx.x == 0 && coef)
            for (int j = 0; j < plan.levels; ++j)
                coef[((int64_t)blockIdx.x * c + ch) * plan.levels + j] = pos ? -coef_scale * plan.w[j] * ms / (v[j] * (double)c * plan.positions[j]) : 0.0;
    }
    if (threadIdx.x == 0 && out) {
        const float val = (float)(1.0 - m / c) * out_scale;
        out[blockIdx.x] = accumulate ? out[blockIdx.x] + val : val;
    }
}

// ---- 4. gradient of one level.  grid = (tiles, c, n).  TOP: level 0 (float32 images, dimg float32 = 127.5 x the pixel gradient, write or accumulate);
// otherwise float64 levels in scratch.  parent: the next coarser level's gradient [n, c, hp, wp] or nullptr on the coarsest level.
template <typename T, bool LAST, bool TOP>
__global__ __launch_bounds__(256) void msssim_grad_kernel(void* dst, const T* img, const T* tgt, const double* parent, const double* coef, int level,
                                                          int levels, int h, int w, int hp, int wp, int64_t t_stride, int tiles_x, double c1,
                                                          double c2, MsWin win, int accumulate) {
    constexpr int PQ = MS_GR * (MS_GR + 1);                      // one pixel plane
    __shared__ double lds[2 * PQ + 5 * MS_GR * (MS_GP + 1)];
    double (*px)[MS_GR + 1] = (double (*)[MS_GR + 1])lds;
    double (*qx)[MS_GR + 1] = (double (*)[MS_GR + 1])(lds + PQ);
    double (*hs)[MS_GR][MS_GP + 1] = (double (*)[MS_GR][MS_GP + 1])(lds + 2 * PQ);
    double (*gm)[MS_GP][MS_GP + 1] = (double (*)[MS_GP][MS_GP + 1])lds;      // ga, gb, gc: over the pixel planes, once those are dead
    static_assert(3 * MS_GP * (MS_GP + 1) <= 2 * PQ, "the three maps must fit the two pixel planes they reuse");
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int c = gridDim.y;
    const int64_t plane = (int64_t)h * w;
    const int64_t pl = (int64_t)blockIdx.z * c + blockIdx.y;
    const T* a = img + pl * plane;
    const T* b = tgt + (int64_t)blockIdx.z * t_stride + (int64_t)blockIdx.y * plane;
    const int r0 = ty * MS_T - MS_H, q0 = tx * MS_T - MS_H;     // image coordinates of the region's first pixel AND of its first position
    const double k = coef[pl * levels + level];
    const int pr = threadIdx.x / MS_T, pq = threadIdx.x - pr * MS_T;         // this thread's pixel of the tile
    const int prr = r0 + MS_H + pr, pqq = q0 + MS_H + pq;
    const bool mine = prr < h && pqq < w;
    double own = 0.0;
    if (k != 0.0) {                                              // (block-uniform.)  k == 0: the clamped branch, or a weight of zero -- nothing to add
        for (int i = threadIdx.x; i < MS_GR * MS_GR; i += 256) {
            const int r = i / MS_GR, q = i - r * MS_GR;
            const int rr = r0 + r, qq = q0 + q;
            double xv = 0.0, yv = 0.0;
            if (rr >= 0 && rr < h && qq >= 0 && qq < w) { xv = ms_pixel(a, (int64_t)rr * w + qq); yv = ms_pixel(b, (int64_t)rr * w + qq); }
            px[r][q] = xv; qx[r][q] = yv;
        }
        __syncthreads();
        const double p_own = px[pr + MS_H][pq + MS_H], q_own = qx[pr + MS_H][pq + MS_H];
        // rows: a thread forms the sums of two neighbouring positions from one 12-pixel register window (12 + 12 LDS reads instead of 2 x 22);
        // consecutive lanes take consecutive rows (odd pitch: conflict-free)
        static_assert(MS_GP % 2 == 0, "positions are taken in pairs");
        for (int i = threadIdx.x; i < MS_GR * (MS_GP / 2); i += 256) {
            const int q = 2 * (i / MS_GR), r = i % MS_GR;
            double s0[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, s1[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int t = 0; t <= MS_W; ++t) {
                const double xv = px[r][q + t], yv = qx[r][q + t];
                const double xx = xv * xv, yy = yv * yv, xy = xv * yv;
                if (t < MS_W) {
                    const double g = win.g[t];
                    s0[0] += g * xv; s0[1] += g * yv; s0[2] += g * xx; s0[3] += g * yy; s0[4] += g * xy;
                }
                if (t > 0) {
                    const double g = win.g[t - 1];
                    s1[0] += g * xv; s1[1] += g * yv; s1[2] += g * xx; s1[3] += g * yy; s1[4] += g * xy;
                }
            }
#pragma unroll
            for (int n5 = 0; n5 < 5; ++n5) { hs[n5][r][q] = s0[n5]; hs[n5][r][q + 1] = s1[n5]; }
        }
        __syncthreads();                                         // px / qx are dead from here on: gm takes their place
        const int vh = h - MS_H, vw = w - MS_H;
        // columns: likewise two positions, one below the other, from a 12-value window of every row-sum plane
        for (int i = threadIdx.x; i < (MS_GP / 2) * MS_GP; i += 256) {
            const int r = 2 * (i / MS_GP), q = i % MS_GP;
            double s0[5], s1[5];
#pragma unroll
            for (int n5 = 0; n5 < 5; ++n5) {
                double v0 = 0.0, v1 = 0.0;
#pragma unroll
                for (int u = 0; u <= MS_W; ++u) {
                    const double v = hs[n5][r + u][q];
                    if (u < MS_W) v0 += win.g[u] * v;
                    if (u > 0) v1 += win.g[u - 1] * v;
                }
                s0[n5] = v0; s1[n5] = v1;
            }
            const int qq = q0 + q;
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const int rr = r0 + r + d;
                MsTerms t = {0.0, 0.0, 0.0, 0.0};
                if (rr >= 0 && rr < vh && qq >= 0 && qq < vw)    // positions that do not lie whole inside the image are masked, never clamped
                    t = d ? ms_terms<LAST>(s1[0], s1[1], s1[2], s1[3], s1[4], c1, c2) : ms_terms<LAST>(s0[0], s0[1], s0[2], s0[3], s0[4], c1, c2);
                gm[0][r + d][q] = t.ga; gm[1][r + d][q] = t.gb; gm[2][r + d][q] = t.gc;
            }
        }
        __syncthreads();
        // adjoint Gaussian filter: pixel (i, j) of the tile lies in the windows of positions (i .. i + 10, j .. j + 10) of the region, under tap
        // 10 - u of the position u steps on
        for (int i = threadIdx.x; i < MS_GP * MS_T; i += 256) {
            const int r = i / MS_T, q = i - r * MS_T;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                double v = 0.0;
#pragma unroll
                for (int t = 0; t < MS_W; ++t) v += win.g[MS_H - t] * gm[m][r][q + t];
                hs[m][r][q] = v;
            }
        }
        __syncthreads();
        if (mine) {
            double s[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                double v = 0.0;
#pragma unroll
                for (int u = 0; u < MS_W; ++u) v += win.g[MS_H - u] * hs[m][pr + u][pq];
                s[m] = v;
            }
            own = k * (s[0] + 2.0 * p_own * s[1] + q_own * s[2]);
        }
    }
    if (!mine) return;
    if (parent) {                                                // the adjoint of the 2 x 2 mean: 1/4 of the one parent pixel this pixel went into
        const int yr = (prr + (h & 1)) >> 1, yq = (pqq + (w & 1)) >> 1;
        own += 0.25 * parent[pl * hp * wp + (int64_t)yr * wp + yq];
    }
    const int64_t o = pl * plane + (int64_t)prr * w + pqq;
    if (TOP) {
        float* d = (float*)dst + o;
        const float g = (float)(127.5 * own);
        *d = accumulate ? *d + g : g;
    } else {
        ((double*)dst)[o] = own;
    }
}

// ---- host side
struct MsLayout {
    int levels, h[MS_MAXL], w[MS_MAXL], tiles_x[MS_MAXL], tiles[MS_MAXL];
    int64_t img_off[MS_MAXL], tgt_off[MS_MAXL], grad_off[MS_MAXL];        // in doubles; level 0 unused (the caller's float32 arrays)
    int64_t part_off, coef_off, total;                                   // part_off: base of the partials, plan.part_off[j] * n c from it
    int64_t part_rel[MS_MAXL];                                           // level j's partials start part_rel[j] * n * c doubles after part_off
    int bad_level;                                                       // first level whose side is below 11, or -1
};

static MsLayout ms_layout(int64_t n, int64_t c, int h, int w, int levels) {
    MsLayout L = {};
    L.levels = levels;
    L.bad_level = -1;
    int64_t off = 0, rel = 0;
    for (int j = 0; j < levels; ++j) {
        L.h[j] = j ? (L.h[j - 1] + 1) / 2 : h;
        L.w[j] = j ? (L.w[j - 1] + 1) / 2 : w;
        if ((L.h[j] < MS_W || L.w[j] < MS_W) && L.bad_level < 0) L.bad_level = j;
        L.tiles_x[j] = (int)mgf_cdiv(L.w[j] > MS_H ? L.w[j] - MS_H : 1, MS_T);
        L.tiles[j] = L.tiles_x[j] * (int)mgf_cdiv(L.h[j] > MS_H ? L.h[j] - MS_H : 1, MS_T);
        L.part_rel[j] = rel;
        rel += L.tiles[j];
        if (j) {
            const int64_t sz = n * c * L.h[j] * L.w[j];
            L.img_off[j] = off; off += sz;
            L.tgt_off[j] = off; off += sz;
            L.grad_off[j] = off; off += sz;
        }
    }
    L.part_off = off; off += rel * n * c;
    L.coef_off = off; off += n * c * levels;
    L.total = off;
    return L;
}

extern "C" int64_t mgf_msssim_scratch_bytes(int32_t n, int32_t c, int32_t h, int32_t w, int32_t levels) {
    if (n < 1 || c < 1 || levels < 1 || levels > MS_MAXL || h < MS_W || w < MS_W) return 0;
    const MsLayout L = ms_layout(n, c, h, w, levels);
    if (L.bad_level >= 0) return 0;
    return L.total * (int64_t)sizeof(double);
}

template <typename T, bool LAST>
static void ms_launch_stats(hipStream_t st, const MsLayout& L, int j, int n, int c, double* part, const T* img, const T* tgt, int64_t t_stride,
                            double c1, double c2, const MsWin& win) {
    hipLaunchKernelGGL((msssim_stats_kernel<T, LAST>), dim3(L.tiles[j], c, n), dim3(256), 0, st, part, img, tgt, L.h[j], L.w[j], t_stride,
                       L.tiles_x[j], c1, c2, win);
}

template <typename T, bool LAST, bool TOP>
static void ms_launch_grad(hipStream_t st, const MsLayout& L, int j, int n, int c, void* dst, const T* img, const T* tgt, const double* parent,
                           const double* coef, int64_t t_stride, double c1, double c2, const MsWin& win, int accumulate) {
    const int tiles_x = (int)mgf_cdiv(L.w[j], MS_T), tiles_y = (int)mgf_cdiv(L.h[j], MS_T);
    const bool has_parent = parent != nullptr;
    hipLaunchKernelGGL((msssim_grad_kernel<T, LAST, TOP>), dim3(tiles_x * tiles_y, c, n), dim3(256), 0, st, dst, img, tgt, parent, coef, j, L.levels,
                       L.h[j], L.w[j], has_parent ? L.h[j + 1] : 0, has_parent ? L.w[j + 1] : 0, t_stride, tiles_x, c1, c2, win, accumulate);
}

static int msssim_launch(const char* what, float* dimg, float* out, const float* img, const float* target, int32_t n, int32_t c, int32_t h,
                         int32_t w, int64_t t_batch_stride, const double* weights, int32_t levels, float data_range, float dimg_scale,
                         float out_scale, int32_t accumulate_dimg, int32_t accumulate_out, void* scratch, mgf_stream_t stream, bool grad) {
    MGF_REQUIRE((dimg || !grad) && (out || grad) && img && target && weights && scratch && n >= 1 && n <= 65535 && c >= 1 && c <= 65535 &&
                t_batch_stride >= 0, MGF_EINVAL, "%s: bad arguments (null pointer, or n / c outside 1..65535)", what);
    MGF_REQUIRE(levels >= 1 && levels <= MS_MAXL, MGF_EINVAL, "%s: levels must lie in 1..%d (got %d)", what, MS_MAXL, (int)levels);
    MGF_REQUIRE(h >= 1 && w >= 1, MGF_EINVAL, "%s: bad image size %dx%d", what, (int)h, (int)w);
    const MsLayout L = ms_layout(n, c, h, w, levels);
    MGF_REQUIRE(L.bad_level < 0, MGF_EINVAL, "%s: level %d of the %dx%d image is %dx%d, smaller than the 11x11 window (%d levels asked for)", what,
                L.bad_level, (int)h, (int)w, L.bad_level >= 0 ? L.h[L.bad_level] : 0, L.bad_level >= 0 ? L.w[L.bad_level] : 0, (int)levels);
    MGF_REQUIRE(data_range > 0.f && (uintptr_t)scratch % 8 == 0, MGF_EINVAL, "%s: data_range must be positive, scratch 8-byte aligned", what);
    const double c1 = (0.01 * (double)data_range) * (0.01 * (double)data_range), c2 = (0.03 * (double)data_range) * (0.03 * (double)data_range);
    MsWin win;
    double gs = 0.0;
    for (int i = 0; i < MS_W; ++i) { win.g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); gs += win.g[i]; }
    for (int i = 0; i < MS_W; ++i) win.g[i] /= gs;
    MsPlan plan = {};
    plan.levels = levels;
    for (int j = 0; j < levels; ++j) {                           // the weights are read NOW and travel by value
        plan.part_off[j] = L.part_rel[j];
        plan.tiles[j] = L.tiles[j];
        plan.positions[j] = (double)(L.h[j] - MS_H) * (double)(L.w[j] - MS_H);
        plan.w[j] = weights[j];
    }
    hipStream_t st = (hipStream_t)stream;
    double* S = (double*)scratch;
    const int nt = t_batch_stride ? n : 1;                       // a shared target has one pyramid
    // 1. pyramid
    for (int j = 1; j < levels; ++j) {
        const int64_t planes_i = (int64_t)n * c, planes_t = (int64_t)nt * c;
        const int64_t per = (int64_t)L.h[j] * L.w[j];
        if (j == 1) {
            hipLaunchKernelGGL(msssim_pool_kernel<float>, dim3(mgf_stream_grid(planes_i * per, 256, 1)), dim3(256), 0, st, S + L.img_off[1], img,
                               planes_i, L.h[0], L.w[0], L.h[1], L.w[1]);
            if (t_batch_stride == 0 || t_batch_stride == (int64_t)c * h * w) {
                hipLaunchKernelGGL(msssim_pool_kernel<float>, dim3(mgf_stream_grid(planes_t * per, 256, 1)), dim3(256), 0, st, S + L.tgt_off[1],
                                   target, planes_t, L.h[0], L.w[0], L.h[1], L.w[1]);
            } else {                                             // an unusual stride: sample by sample
                for (int i = 0; i < n; ++i)
                    hipLaunchKernelGGL(msssim_pool_kernel<float>, dim3(mgf_stream_grid((int64_t)c * per, 256, 1)), dim3(256), 0, st,
                                       S + L.tgt_off[1] + (int64_t)i * c * per, target + (int64_t)i * t_batch_stride, (int64_t)c, L.h[0], L.w[0],
                                       L.h[1], L.w[1]);
            }
        } else {
            hipLaunchKernelGGL(msssim_pool_kernel<double>, dim3(mgf_stream_grid(planes_i * per, 256, 1)), dim3(256), 0, st, S + L.img_off[j],
                               (const double*)(S + L.img_off[j - 1]), planes_i, L.h[j - 1], L.w[j - 1], L.h[j], L.w[j]);
            hipLaunchKernelGGL(msssim_pool_kernel<double>, dim3(mgf_stream_grid(planes_t * per, 256, 1)), dim3(256), 0, st, S + L.tgt_off[j],
                               (const double*)(S + L.tgt_off[j - 1]), planes_t, L.h[j - 1], L.w[j - 1], L.h[j], L.w[j]);
        }
    }
    // 2. statistics
    double* part = S + L.part_off;
    for (int j = 0; j < levels; ++j) {
        double* pj = part + L.part_rel[j] * n * c;
        const bool last = j == levels - 1;
        if (j == 0) {
            if (last) ms_launch_stats<float, true>(st, L, 0, n, c, pj, img, target, t_batch_stride, c1, c2, win);
            else ms_launch_stats<float, false>(st, L, 0, n, c, pj, img, target, t_batch_stride, c1, c2, win);
        } else {
            const int64_t ts = t_batch_stride ? (int64_t)c * L.h[j] * L.w[j] : 0;
            if (last) ms_launch_stats<double, true>(st, L, j, n, c, pj, S + L.img_off[j], S + L.tgt_off[j], ts, c1, c2, win);
            else ms_launch_stats<double, false>(st, L, j, n, c, pj, S + L.img_off[j], S + L.tgt_off[j], ts, c1, c2, win);
        }
    }
    // 3. value and coefficients
    double* coef = S + L.coef_off;
    hipLaunchKernelGGL(msssim_finish_kernel, dim3(n), dim3(256), 0, st, out, grad ? coef : (double*)nullptr, (const double*)part, (int)c, plan,
                       out_scale, (double)dimg_scale, accumulate_out);
    // 4. gradient, coarsest level first
    if (grad) {
        for (int j = levels - 1; j >= 0; --j) {
            const bool last = j == levels - 1;
            const double* parent = last ? nullptr : S + L.grad_off[j + 1];
            if (j == 0) {
                if (last) ms_launch_grad<float, true, true>(st, L, 0, n, c, dimg, img, target, parent, coef, t_batch_stride, c1, c2, win, accumulate_dimg);
                else ms_launch_grad<float, false, true>(st, L, 0, n, c, dimg, img, target, parent, coef, t_batch_stride, c1, c2, win, accumulate_dimg);
            } else {
                const int64_t ts = t_batch_stride ? (int64_t)c * L.h[j] * L.w[j] : 0;
                const double* ij = S + L.img_off[j];
                const double* tj = S + L.tgt_off[j];
                if (last) ms_launch_grad<double, true, false>(st, L, j, n, c, S + L.grad_off[j], ij, tj, parent, coef, ts, c1, c2, win, 0);
                else ms_launch_grad<double, false, false>(st, L, j, n, c, S + L.grad_off[j], ij, tj, parent, coef, ts, c1, c2, win, 0);
            }
        }
    }
    MGF_CHECK_LAUNCH(what);
    return MGF_OK;
}

extern "C" int mgf_msssim_f32(float* out, const float* img, const float* target, int32_t n, int32_t c, int32_t h, int32_t w, int64_t t_batch_stride,
                              const double* weights, int32_t levels, float data_range, float scale, int32_t accumulate, void* scratch,
                              mgf_stream_t stream) {
    return msssim_launch("msssim_f32", nullptr, out, img, target, n, c, h, w, t_batch_stride, weights, levels, data_range, 0.f, scale, 0, accumulate,
                         scratch, stream, false);
}

extern "C" int mgf_msssim_grad_f32(float* dimg, float* out, const float* img, const float* target, int32_t n, int32_t c, int32_t h, int32_t w,
                                   int64_t t_batch_stride, const double* weights, int32_t levels, float data_range, float scale,
                                   int32_t accumulate_dimg, int32_t accumulate_out, void* scratch, mgf_stream_t stream) {
    return msssim_launch("msssim_grad_f32", dimg, out, img, target, n, c, h, w, t_batch_stride, weights, levels, data_range, scale, 1.f,
                         accumulate_dimg, accumulate_out, scratch, stream, true);
}
