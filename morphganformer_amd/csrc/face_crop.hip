// The aligned face crop of the ArcFace biometric term and its adjoint -- the definition is in include/mgf.h (mgf_face_crop_f32).
//
// Both kernels read the 2x3 matrices from device memory and derive S from them there: no launch parameter depends on their values, so a captured
// launch stays valid when the matrices are rewritten in place.  Coordinates, weights and sums are float64; the only float32 step is the store.
//
//   face_crop_kernel      a workgroup owns 16 crop pixels x 16 sub-sample rows: lane (p, j) sums row j (j < S) of pixel p's S x S bilinear samples for
//                         the three channels, the 16 rows are added by a 16-lane butterfly (a fixed order), lane j = 0 stores.
//   face_crop_bwd_kernel  a gather: a thread owns one source pixel, maps its 2 x 2 neighbourhood through M^-1 to a box of sub-sample indices and adds,
//                         rows then columns ascending, hat(x - px) hat(y - py) dy / S^2 of every sub-sample in the box (hat(t) = max(0, 1 - |t|) is the
//                         bilinear weight of tap px for a sample at x).  No atomics: two calls give the same bits.
#include "mgf_common.h"
#include <math.h>

namespace {

constexpr int kMaxS = 16;
constexpr double kMinDet = 1e-12;

struct CropMap {
    double a, b, tx, c, d, ty;     // (x, y) = (a u + b v + tx, c u + d v + ty)
    double det;
    int s;                         // sub-samples per side
};

__device__ __forceinline__ CropMap load_map(const double* m, int filter) {
    CropMap k;
    k.a = m[0]; k.b = m[1]; k.tx = m[2]; k.c = m[3]; k.d = m[4]; k.ty = m[5];
    k.det = k.a * k.d - k.b * k.c;
    k.s = 1;
    if (filter == MGF_CROP_AREA) {
        double r = ceil(sqrt(fabs(k.det)));
        k.s = r >= (double)kMaxS ? kMaxS : (r >= 1.0 ? (int)r : 1);     // a NaN compares false everywhere: 1
    }
    return k;
}

__global__ __launch_bounds__(256) void face_crop_kernel(float* y, const float* x, const double* mats, int64_t pixels, int h, int w, int size,
                                                        int64_t m_stride, int filter) {
    const int j = threadIdx.x & 15;
    const int64_t pix = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = pix < pixels;
    const int64_t per = (int64_t)size * size;
    const int64_t n = live ? pix / per : 0;
    const int v = live ? (int)((pix - n * per) / size) : 0, u = live ? (int)(pix - n * per - (int64_t)v * size) : 0;
    const CropMap k = load_map(mats + n * m_stride, filter);
    const int64_t plane = (int64_t)h * w;
    const float* xn = x + n * 3 * plane;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    if (live && j < k.s) {
        const double inv_s = 1.0 / k.s;
        const double vc = v + (j + 0.5) * inv_s - 0.5;
        for (int i = 0; i < k.s; ++i) {
            const double uc = u + (i + 0.5) * inv_s - 0.5;
            const double sx = k.a * uc + k.b * vc + k.tx, sy = k.c * uc + k.d * vc + k.ty;
            if (!(sx > -1.0 && sx < (double)w && sy > -1.0 && sy < (double)h)) continue;      // all four taps outside (or a NaN): zero
            const double fx0 = floor(sx), fy0 = floor(sy);
            const int x0 = (int)fx0, y0 = (int)fy0;                                               // in [-1, w - 1] x [-1, h - 1]
            const double wx1 = sx - fx0, wy1 = sy - fy0, wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
            const bool l = x0 >= 0, r = x0 + 1 < w, t = y0 >= 0, b = y0 + 1 < h;
            const int64_t o00 = (int64_t)y0 * w + x0;
            const double w00 = t && l ? wy0 * wx0 : 0.0, w01 = t && r ? wy0 * wx1 : 0.0, w10 = b && l ? wy1 * wx0 : 0.0, w11 = b && r ? wy1 * wx1 : 0.0;
            const int64_t i00 = t && l ? o00 : 0, i01 = t && r ? o00 + 1 : 0, i10 = b && l ? o00 + w : 0, i11 = b && r ? o00 + w + 1 : 0;
            acc0 += w00 * xn[i00] + w01 * xn[i01] + w10 * xn[i10] + w11 * xn[i11];
            acc1 += w00 * xn[plane + i00] + w01 * xn[plane + i01] + w10 * xn[plane + i10] + w11 * xn[plane + i11];
            acc2 += w00 * xn[2 * plane + i00] + w01 * xn[2 * plane + i01] + w10 * xn[2 * plane + i10] + w11 * xn[2 * plane + i11];
        }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        acc0 += __shfl_xor(acc0, o, 16);
        acc1 += __shfl_xor(acc1, o, 16);
        acc2 += __shfl_xor(acc2, o, 16);
    }
    if (live && j == 0) {
        const double norm = 1.0 / ((double)k.s * k.s);
        float* yn = y + n * 3 * per + (int64_t)v * size + u;
        yn[0] = (float)(acc0 * norm);
        yn[per] = (float)(acc1 * norm);
        yn[2 * per] = (float)(acc2 * norm);
    }
}

__global__ __launch_bounds__(256) void face_crop_bwd_kernel(float* dx, const float* dy, const double* mats, int64_t pixels, int h, int w, int size,
                                                            int64_t m_stride, int filter, int accumulate) {
    const int64_t plane = (int64_t)h * w, per = (int64_t)size * size;
    for (int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x; pix < pixels; pix += (int64_t)gridDim.x * 256) {
        const int64_t n = pix / plane;
        const int py = (int)((pix - n * plane) / w), px = (int)(pix - n * plane - (int64_t)py * w);
        const CropMap k = load_map(mats + n * m_stride, filter);
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
        if (fabs(k.det) >= kMinDet) {                                         // a singular matrix has no box (the host check refuses it)
            const int fine = size * k.s;                                      // sub-samples per side of the whole crop
            const double inv_s = 1.0 / k.s, rdet = 1.0 / k.det;
            // the crop coordinates of the corners (px -+ 1, py -+ 1): M^-1 is linear, so the extremes over the square are centre +- the absolute sums
            const double ex = px - k.tx, ey = py - k.ty;
            const double uc = (k.d * ex - k.b * ey) * rdet, vc = (k.a * ey - k.c * ex) * rdet;
            const double ru = (fabs(k.d) + fabs(k.b)) * fabs(rdet), rv = (fabs(k.a) + fabs(k.c)) * fabs(rdet);
            // (clamped to the crop below: a pixel away from the crop's footprint gets an empty box whatever the matrix, so up-sampling hard -- scale
            // 1e-3 -- leaves a handful of pixels with at most size^2 sub-samples each, less work than the typical face's 20 per pixel on all of them)
            // crop coordinate t -> sub-sample index (t + 0.5) S - 0.5; clamped as doubles first (fmax / fmin drop a NaN), so the casts are safe
            const double a_lo = fmax(floor((uc - ru + 0.5) * k.s - 0.5), 0.0), a_hi = fmin(ceil((uc + ru + 0.5) * k.s - 0.5), (double)(fine - 1));
            const double b_lo = fmax(floor((vc - rv + 0.5) * k.s - 0.5), 0.0), b_hi = fmin(ceil((vc + rv + 0.5) * k.s - 0.5), (double)(fine - 1));
            if (a_lo <= a_hi && b_lo <= b_hi) {
                const float* dyn = dy + n * 3 * per;
                const int a0 = (int)a_lo, a1 = (int)a_hi, b0 = (int)b_lo, b1 = (int)b_hi;
                for (int b = b0; b <= b1; ++b) {
                    const double tv = (b + 0.5) * inv_s - 0.5;
                    const int64_t row = (int64_t)(b / k.s) * size;
                    for (int a = a0; a <= a1; ++a) {
                        const double tu = (a + 0.5) * inv_s - 0.5;
                        const double hx = 1.0 - fabs(k.a * tu + k.b * tv + k.tx - px), hy = 1.0 - fabs(k.c * tu + k.d * tv + k.ty - py);
                        if (hx > 0.0 && hy > 0.0) {
                            const double wgt = hx * hy;
                            const int64_t o = row + a / k.s;
                            acc0 += wgt * dyn[o];
                            acc1 += wgt * dyn[per + o];
                            acc2 += wgt * dyn[2 * per + o];
                        }
                    }
                }
            }
        }
        const double norm = 1.0 / ((double)k.s * k.s);
        float* d = dx + n * 3 * plane + (int64_t)py * w + px;
        if (accumulate) {
            d[0] = (float)((double)d[0] + acc0 * norm);
            d[plane] = (float)((double)d[plane] + acc1 * norm);
            d[2 * plane] = (float)((double)d[2 * plane] + acc2 * norm);
        } else {
            d[0] = (float)(acc0 * norm);
            d[plane] = (float)(acc1 * norm);
            d[2 * plane] = (float)(acc2 * norm);
        }
    }
}

int check_args(const char* what, const void* p, const void* q, const double* m, int32_t n, int32_t h, int32_t w, int32_t size, int32_t m_count,
               int32_t filter) {
    MGF_REQUIRE(p && q && m && n >= 1 && h >= 1 && w >= 1 && size >= 1, MGF_EINVAL, "%s: bad arguments", what);
    MGF_REQUIRE(m_count == 1 || m_count == n, MGF_EINVAL, "%s: %d matrices for %d images (one shared matrix, or one per image)", what, m_count, n);
    MGF_REQUIRE(filter == MGF_CROP_AREA || filter == MGF_CROP_BILINEAR, MGF_EINVAL, "%s: unknown filter %d", what, filter);
    MGF_REQUIRE((int64_t)size * kMaxS < (int64_t)1 << 30 && (int64_t)n * size * size / 16 < (int64_t)1 << 31, MGF_ETOOBIG, "%s: crop too large",
                what);
    return MGF_OK;
}

}  // namespace

extern "C" int mgf_face_crop_check(const double* matrices, int32_t count, int32_t filter) {
    MGF_REQUIRE(matrices && count >= 1, MGF_EINVAL, "face_crop_check: bad arguments");
    MGF_REQUIRE(filter == MGF_CROP_AREA || filter == MGF_CROP_BILINEAR, MGF_EINVAL, "face_crop_check: unknown filter %d", filter);
    for (int32_t i = 0; i < count; ++i) {
        const double* m = matrices + 6 * i;
        bool finite = true;
        for (int e = 0; e < 6; ++e) finite = finite && isfinite(m[e]);
        MGF_REQUIRE(finite, MGF_EINVAL, "face_crop_check: matrix %d has a non-finite entry", i);
        const double det = fabs(m[0] * m[4] - m[1] * m[3]);
        MGF_REQUIRE(det >= kMinDet, MGF_EINVAL, "face_crop_check: matrix %d is singular (|det| = %g)", i, det);
        MGF_REQUIRE(filter != MGF_CROP_AREA || ceil(sqrt(det)) <= (double)kMaxS, MGF_EINVAL,
                    "face_crop_check: matrix %d shrinks by %g per side, the area filter takes at most %d sub-samples per side", i, sqrt(det), kMaxS);
    }
    return MGF_OK;
}

extern "C" int mgf_face_crop_f32(float* y, const float* x, const double* matrices, int32_t n, int32_t h, int32_t w, int32_t size, int32_t m_count,
                                 int32_t filter, mgf_stream_t stream) {
    int rc = check_args("face_crop", y, x, matrices, n, h, w, size, m_count, filter);
    if (rc != MGF_OK) return rc;
    const int64_t pixels = (int64_t)n * size * size;
    hipLaunchKernelGGL(face_crop_kernel, dim3((unsigned)mgf_cdiv(pixels, 16)), dim3(256), 0, (hipStream_t)stream, y, x, matrices, pixels, (int)h,
                       (int)w, (int)size, (int64_t)(m_count == 1 ? 0 : 6), (int)filter);
    MGF_CHECK_LAUNCH("face_crop");
    return MGF_OK;
}

extern "C" int mgf_face_crop_bwd_f32(float* dx, const float* dy, const double* matrices, int32_t n, int32_t h, int32_t w, int32_t size,
                                     int32_t m_count, int32_t filter, int32_t accumulate, mgf_stream_t stream) {
    int rc = check_args("face_crop_bwd", dx, dy, matrices, n, h, w, size, m_count, filter);
    if (rc != MGF_OK) return rc;
    const int64_t pixels = (int64_t)n * h * w;
    hipLaunchKernelGGL(face_crop_bwd_kernel, dim3(mgf_stream_grid(pixels, 256, 1)), dim3(256), 0, (hipStream_t)stream, dx, dy, matrices, pixels,
                       (int)h, (int)w, (int)size, (int64_t)(m_count == 1 ? 0 : 6), (int)filter, (int)(accumulate != 0));
    MGF_CHECK_LAUNCH("face_crop_bwd");
    return MGF_OK;
}
