// DSSIM of two images, all device-side: the uint8 form of the literal loop's scripts (mgf_dssim_u8_f32) and the continuous form with its
// gradient (mgf_dssim_f32, mgf_dssim_grad_f32, gradient mode's pixel_term="dssim").  Float64 sums in a fixed order: one partial per workgroup,
// one finishing workgroup per sample (no atomics -> bit-reproducible).  Contract: include/mgf.h.
#include "mgf_common.h"

// ---- DSSIM of the uint8 images (`dssim`, 1024_example_SSIM.py:115-117 = lpips/__init__.py:54-55: (1 - compare_ssim(p0, p1, data_range=255,
// multichannel=True)) / 2, skimage's defaults: 7x7 uniform window, sample covariance, K1 = 0.01, K2 = 0.03, the window positions that lie
// whole inside the image, mean over positions then over channels).  Both images are quantised like the image the drivers save
// (misc.to_pil:115-116: rint(x * 127.5 + 127.5) clipped to 0..255), so the five window sums (x, y, xx, yy, xy over 49 pixels) are exact
// integers (< 2^22); the SSIM quotient and every sum above it are float64 in a fixed order.
// grid = (tiles, c, n); a workgroup owns 32 x 32 window positions of one channel plane and reads the 38 x 38 pixels under them.
constexpr int DS_T = 32, DS_W = 7, DS_R = DS_T + DS_W - 1;
__device__ __forceinline__ int ds_quant(float v) {
    v = rintf(__fadd_rn(__fmul_rn(v, 127.5f), 127.5f));
    return (int)fminf(fmaxf(v, 0.f), 255.f);
}
__global__ __launch_bounds__(256) void dssim_partial_kernel(double* part, const float* img, const float* tgt, int h, int w, int64_t t_stride,
                                                            int tiles_x, double c1, double c2) {
    __shared__ int xs[DS_R][DS_R + 1], ys[DS_R][DS_R + 1];
    __shared__ int hs[5][DS_R][DS_T + 1];
    __shared__ double red[256];
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int c = gridDim.y;
    const int64_t plane = (int64_t)h * w;
    const float* a = img + ((int64_t)blockIdx.z * c + blockIdx.y) * plane;
    const float* b = tgt + (int64_t)blockIdx.z * t_stride + (int64_t)blockIdx.y * plane;
    const int r0 = ty * DS_T, q0 = tx * DS_T;
    for (int i = threadIdx.x; i < DS_R * DS_R; i += 256) {
        const int r = i / DS_R, q = i - r * DS_R;
        const int rr = r0 + r, qq = q0 + q;
        int xv = 0, yv = 0;
        if (rr < h && qq < w) { xv = ds_quant(a[(int64_t)rr * w + qq]); yv = ds_quant(b[(int64_t)rr * w + qq]); }
        xs[r][q] = xv; ys[r][q] = yv;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < DS_R * DS_T; i += 256) {
        const int r = i / DS_T, q = i - r * DS_T;
        int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int t = 0; t < DS_W; ++t) {
            const int xv = xs[r][q + t], yv = ys[r][q + t];
            sx += xv; sy += yv; sxx += xv * xv; syy += yv * yv; sxy += xv * yv;
        }
        hs[0][r][q] = sx; hs[1][r][q] = sy; hs[2][r][q] = sxx; hs[3][r][q] = syy; hs[4][r][q] = sxy;
    }
    __syncthreads();
    double acc = 0.0;
    const int vh = h - (DS_W - 1), vw = w - (DS_W - 1);         // window positions per plane
    for (int i = threadIdx.x; i < DS_T * DS_T; i += 256) {
        const int r = i / DS_T, q = i - r * DS_T;
        if (r0 + r >= vh || q0 + q >= vw) continue;
        int s[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            int v = 0;
#pragma unroll
            for (int t = 0; t < DS_W; ++t) v += hs[k][r + t][q];
            s[k] = v;
        }
        // (not ds_terms below: its products are __dmul_rn, these contract into fmas -- other bits, and the scripts' values are pinned on these)
        constexpr double inv = 1.0 / (DS_W * DS_W), cov = (double)(DS_W * DS_W) / (DS_W * DS_W - 1);
        const double ux = s[0] * inv, uy = s[1] * inv, uxx = s[2] * inv, uyy = s[3] * inv, uxy = s[4] * inv;
        const double vx = cov * (uxx - ux * ux), vy = cov * (uyy - uy * uy), vxy = cov * (uxy - ux * uy);
        const double a1 = 2.0 * ux * uy + c1, a2 = 2.0 * vxy + c2, b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
        acc += (a1 * a2) / (b1 * b2);
    }
    acc = mgf_block_tree_sum_256(acc, red);
    if (threadIdx.x == 0) part[((int64_t)blockIdx.z * c + blockIdx.y) * gridDim.x + tile] = acc;
}

// grid = n: out = (accumulate ? out : 0) + scale * (1 - mean_c mean_positions S) / 2, the value as float32 like the script's FloatTensor (:159)
__global__ __launch_bounds__(256) void dssim_finish_kernel(float* out, const double* part, int c, int tiles, double positions, float scale,
                                                           int accumulate) {
    __shared__ double red[256];
    double m = 0.0;
    for (int ch = 0; ch < c; ++ch) {
        const double* p = part + ((int64_t)blockIdx.x * c + ch) * tiles;
        double v = 0.0;
        for (int i = threadIdx.x; i < tiles; i += 256) v += p[i];
        m += mgf_block_tree_sum_256(v, red) / positions;
    }
    if (threadIdx.x == 0) {
        const float v = (float)((1.0 - m / c) / 2.0) * scale;
        out[blockIdx.x] = accumulate ? out[blockIdx.x] + v : v;
    }
}

extern "C" int64_t mgf_dssim_scratch_bytes(int32_t n, int32_t c, int32_t h, int32_t w) {
    if (n < 1 || c < 1 || h < DS_W || w < DS_W) return 0;
    // one float64 partial per workgroup: 32 x 32 window positions (mgf_dssim_u8_f32) or 16 x 16 pixels (mgf_dssim_f32 / mgf_dssim_grad_f32,
    // below) -- the second count is never the smaller one, and one buffer serves all three
    const int64_t tiles = (int64_t)mgf_cdiv(h - (DS_W - 1), DS_T) * mgf_cdiv(w - (DS_W - 1), DS_T);
    const int64_t tiles_cont = (int64_t)mgf_cdiv(h, 16) * mgf_cdiv(w, 16);
    return (int64_t)n * c * (tiles > tiles_cont ? tiles : tiles_cont) * (int64_t)sizeof(double);
}

// What both launches check and the SSIM constants c1 = (K1 L)^2, c2 = (K2 L)^2.  `ptrs_ok`: the entry's own pointer and stride tests; `what`
// and the two notes keep every entry's messages as they were.
struct DsConst { double c1, c2; };
static int dssim_check(DsConst* k, const char* what, const char* args_note, const char* window_note, bool ptrs_ok, int32_t n, int32_t c, int32_t h,
                       int32_t w, float data_range, const void* scratch) {
    MGF_REQUIRE(ptrs_ok && scratch && n >= 1 && n <= 65535 && c >= 1 && c <= 65535, MGF_EINVAL, "%s: bad arguments%s", what, args_note);
    MGF_REQUIRE(h >= DS_W && w >= DS_W, MGF_EINVAL, "%s: the image is smaller than the 7x7 window%s", what, window_note);
    MGF_REQUIRE(data_range > 0.f && (uintptr_t)scratch % 8 == 0, MGF_EINVAL, "%s: data_range must be positive, scratch 8-byte aligned", what);
    k->c1 = (0.01 * (double)data_range) * (0.01 * (double)data_range);
    k->c2 = (0.03 * (double)data_range) * (0.03 * (double)data_range);
    return MGF_OK;
}

extern "C" int mgf_dssim_u8_f32(float* out, const float* img, const float* target, int32_t n, int32_t c, int32_t h, int32_t w,
                                int64_t t_batch_stride, float data_range, float scale, int32_t accumulate, void* scratch,
                                mgf_stream_t stream) {
    DsConst k;
    const int rc = dssim_check(&k, "dssim", "", " (skimage raises here)", out && img && target, n, c, h, w, data_range, scratch);
    if (rc != MGF_OK) return rc;
    const int tiles_y = (int)mgf_cdiv(h - (DS_W - 1), DS_T), tiles_x = (int)mgf_cdiv(w - (DS_W - 1), DS_T);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(dssim_partial_kernel, dim3(tiles_x * tiles_y, c, n), dim3(256), 0, st, (double*)scratch, img, target, h, w,
                       t_batch_stride, tiles_x, k.c1, k.c2);
    hipLaunchKernelGGL(dssim_finish_kernel, dim3(n), dim3(256), 0, st, out, (const double*)scratch, c, tiles_x * tiles_y,
                       (double)(h - (DS_W - 1)) * (double)(w - (DS_W - 1)), scale, accumulate);
    MGF_CHECK_LAUNCH("dssim");
    return MGF_OK;
}

// ---- The continuous DSSIM and its gradient (gradient mode's pixel_term="dssim"): the same function as above on the UNQUANTISED pixels
// p = 127.5 img + 127.5, q = 127.5 target + 127.5 (no rint, no clip -- the quantisation has gradient zero almost everywhere), float64 from the
// float32 loads on (the uxx - ux^2 cancellation costs 2e-4 on the gradient of a smooth image in float32).  With, per window position,
//   ga = dS/dux (through vx and vxy) = (2 uy A2 - 2 cov uy A1) / (B1 B2) - S (2 ux / B1 - 2 cov ux / B2)
//   gb = dS/duxx = -S cov / B2            gc = dS/duxy = 2 cov A1 / (B1 B2)
// the gradient at a pixel is -(127.5 / (2 c positions 49)) (sum ga + 2 p sum gb + q sum gc), the sums over the window positions whose window holds
// the pixel: three adjoint box filters.
// grid = (tiles, c, n); a workgroup owns 16 x 16 pixels of one channel plane: it loads the 28 x 28 pixels around them (6-pixel halo) as float32,
// forms the row sums and the five window sums of the 22 x 22 positions that touch its pixels, S / ga / gb / gc there (positions that do not lie
// whole inside the image are masked to zero, never clamped), and box-sums the three maps back over rows and columns.  Every pixel of dimg has
// one owner (no atomics); S is summed over the positions whose top-left pixel the tile owns, in a fixed order, into one float64 partial per
// tile for dssim_finish_kernel.  GRAD = false (mgf_dssim_f32) is the same code without the three maps, so both entry points give the same bits.
constexpr int DG_T = 16, DG_H = DS_W - 1, DG_P = DG_T + DG_H, DG_R = DG_P + DG_H;      // tile, halo, positions per side, pixels per side
struct DsTerms { double s, ga, gb, gc; };
__device__ __forceinline__ DsTerms ds_terms(double sx, double sy, double sxx, double syy, double sxy, double c1, double c2) {
    constexpr double inv = 1.0 / (DS_W * DS_W), cov = (double)(DS_W * DS_W) / (DS_W * DS_W - 1);
    const double ux = sx * inv, uy = sy * inv, uxx = sxx * inv, uyy = syy * inv, uxy = sxy * inv;
    // the three products stand alone (no fma into the differences and sums below): identical images must give A1 == B1 and A2 == B2 bit for bit
    const double mxx = __dmul_rn(ux, ux), myy = __dmul_rn(uy, uy), mxy = __dmul_rn(ux, uy);
    const double vx = cov * (uxx - mxx), vy = cov * (uyy - myy), vxy = cov * (uxy - mxy);
    const double a1 = 2.0 * mxy + c1, a2 = 2.0 * vxy + c2, b1 = (mxx + myy) + c1, b2 = (vx + vy) + c2;
    const double rb = 1.0 / (b1 * b2);
    DsTerms t;
    t.s = (a1 * a2) / (b1 * b2);
    t.ga = (2.0 * uy * a2 - 2.0 * cov * uy * a1) * rb - t.s * (2.0 * ux / b1 - 2.0 * cov * ux / b2);
    t.gb = -t.s * cov / b2;
    t.gc = 2.0 * cov * a1 * rb;
    return t;
}

template <bool GRAD>
__global__ __launch_bounds__(256) void dssim_cont_kernel(float* dimg, double* part, const float* img, const float* tgt, int h, int w,
                                                         int64_t t_stride, int tiles_x, double c1, double c2, double coef, int accumulate) {
    __shared__ float px[DG_R][DG_R + 1], qx[DG_R][DG_R + 1];
    __shared__ double hs[5][DG_R][DG_P + 1];                    // row sums of p, q, pp, qq, pq; later (GRAD) the row sums of ga, gb, gc
    __shared__ double gm[GRAD ? 3 : 1][GRAD ? DG_P : 1][GRAD ? DG_P + 1 : 1];
    __shared__ double red[256];
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int c = gridDim.y;
    const int64_t plane = (int64_t)h * w;
    const int64_t img_off = ((int64_t)blockIdx.z * c + blockIdx.y) * plane;
    const float* a = img + img_off;
    const float* b = tgt + (int64_t)blockIdx.z * t_stride + (int64_t)blockIdx.y * plane;
    const int r0 = ty * DG_T - DG_H, q0 = tx * DG_T - DG_H;     // image coordinates of the region's first pixel AND of its first position
    for (int i = threadIdx.x; i < DG_R * DG_R; i += 256) {
        const int r = i / DG_R, q = i - r * DG_R;
        const int rr = r0 + r, qq = q0 + q;
        float xv = 0.f, yv = 0.f;
        if (rr >= 0 && rr < h && qq >= 0 && qq < w) { xv = a[(int64_t)rr * w + qq]; yv = b[(int64_t)rr * w + qq]; }
        px[r][q] = xv; qx[r][q] = yv;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < DG_R * DG_P; i += 256) {
        const int r = i / DG_P, q = i - r * DG_P;
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
        for (int t = 0; t < DS_W; ++t) {
            const double xv = 127.5 * (double)px[r][q + t] + 127.5, yv = 127.5 * (double)qx[r][q + t] + 127.5;
            sx += xv; sy += yv; sxx += xv * xv; syy += yv * yv; sxy += xv * yv;
        }
        hs[0][r][q] = sx; hs[1][r][q] = sy; hs[2][r][q] = sxx; hs[3][r][q] = syy; hs[4][r][q] = sxy;
    }
    __syncthreads();
    double acc = 0.0;
    const int vh = h - DG_H, vw = w - DG_H;                     // window positions per plane
    for (int i = threadIdx.x; i < DG_P * DG_P; i += 256) {
        const int r = i / DG_P, q = i - r * DG_P;
        const int rr = r0 + r, qq = q0 + q;
        DsTerms t = {0.0, 0.0, 0.0, 0.0};
        if (rr >= 0 && rr < vh && qq >= 0 && qq < vw) {
            double s[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                double v = 0.0;
#pragma unroll
                for (int u = 0; u < DS_W; ++u) v += hs[k][r + u][q];
                s[k] = v;
            }
            t = ds_terms(s[0], s[1], s[2], s[3], s[4], c1, c2);
            if (r >= DG_H && q >= DG_H) acc += t.s;
        }
        if (GRAD) { gm[0][r][q] = t.ga; gm[1][r][q] = t.gb; gm[2][r][q] = t.gc; }
    }
    acc = mgf_block_tree_sum_256(acc, red);
    if (threadIdx.x == 0) part[((int64_t)blockIdx.z * c + blockIdx.y) * gridDim.x + tile] = acc;
    if (!GRAD) return;
    // adjoint box filter: pixel (i, j) of the tile lies in the windows of positions (i .. i + 6, j .. j + 6) of the region.  (The syncs of the
    // reduction above separate the last read of hs from these writes.)
    for (int i = threadIdx.x; i < DG_P * DG_T; i += 256) {
        const int r = i / DG_T, q = i - r * DG_T;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double v = 0.0;
#pragma unroll
            for (int t = 0; t < DS_W; ++t) v += gm[k][r][q + t];
            hs[k][r][q] = v;
        }
    }
    __syncthreads();
    {
        const int r = threadIdx.x / DG_T, q = threadIdx.x - r * DG_T;              // 256 threads = the tile's 16 x 16 pixels
        const int rr = r0 + DG_H + r, qq = q0 + DG_H + q;
        if (rr < h && qq < w) {
            double s[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                double v = 0.0;
#pragma unroll
                for (int u = 0; u < DS_W; ++u) v += hs[k][r + u][q];
                s[k] = v;
            }
            const double p = 127.5 * (double)px[r + DG_H][q + DG_H] + 127.5, t = 127.5 * (double)qx[r + DG_H][q + DG_H] + 127.5;
            const double g = coef * (s[0] + 2.0 * p * s[1] + t * s[2]);
            float* d = dimg + img_off + (int64_t)rr * w + qq;
            *d = accumulate ? *d + (float)g : (float)g;
        }
    }
}

static int dssim_cont_launch(const char* what, float* dimg, float* out, const float* img, const float* target, int32_t n, int32_t c, int32_t h,
                             int32_t w, int64_t t_batch_stride, float data_range, float dimg_scale, float out_scale, int32_t accumulate_dimg,
                             int32_t accumulate_out, void* scratch, mgf_stream_t stream, bool grad) {
    DsConst k;
    const int rc = dssim_check(&k, what, " (null pointer, or n / c outside 1..65535)", "",
                               (dimg || !grad) && (out || grad) && img && target && t_batch_stride >= 0, n, c, h, w, data_range, scratch);
    if (rc != MGF_OK) return rc;
    const int tiles_y = (int)mgf_cdiv(h, DG_T), tiles_x = (int)mgf_cdiv(w, DG_T);
    const double positions = (double)(h - DG_H) * (double)(w - DG_H);
    const double coef = -(double)dimg_scale * 127.5 / (2.0 * (double)c * positions * (double)(DS_W * DS_W));
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(tiles_x * tiles_y, c, n);
    if (grad)
        hipLaunchKernelGGL(dssim_cont_kernel<true>, grid, dim3(256), 0, st, dimg, (double*)scratch, img, target, h, w, t_batch_stride, tiles_x, k.c1,
                           k.c2, coef, accumulate_dimg);
    else
        hipLaunchKernelGGL(dssim_cont_kernel<false>, grid, dim3(256), 0, st, (float*)nullptr, (double*)scratch, img, target, h, w, t_batch_stride,
                           tiles_x, k.c1, k.c2, 0.0, 0);
    if (out)
        hipLaunchKernelGGL(dssim_finish_kernel, dim3(n), dim3(256), 0, st, out, (const double*)scratch, c, tiles_x * tiles_y, positions, out_scale,
                           accumulate_out);
    MGF_CHECK_LAUNCH(what);
    return MGF_OK;
}

extern "C" int mgf_dssim_f32(float* out, const float* img, const float* target, int32_t n, int32_t c, int32_t h, int32_t w, int64_t t_batch_stride,
                             float data_range, float scale, int32_t accumulate, void* scratch, mgf_stream_t stream) {
    return dssim_cont_launch("dssim_f32", nullptr, out, img, target, n, c, h, w, t_batch_stride, data_range, 0.f, scale, 0, accumulate, scratch, stream,
                             false);
}

extern "C" int mgf_dssim_grad_f32(float* dimg, float* out, const float* img, const float* target, int32_t n, int32_t c, int32_t h, int32_t w,
                                  int64_t t_batch_stride, float data_range, float scale, int32_t accumulate_dimg, int32_t accumulate_out,
                                  void* scratch, mgf_stream_t stream) {
    return dssim_cont_launch("dssim_grad_f32", dimg, out, img, target, n, c, h, w, t_batch_stride, data_range, scale, 1.f, accumulate_dimg,
                             accumulate_out, scratch, stream, true);
}
