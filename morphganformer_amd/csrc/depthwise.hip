// Depthwise (groups == channels) convolutions of the MobileFaceNet embedder (backbones/mobilefacenet.py:16-85): contract in include/mgf.h
// (mgf_dwconv_f32, mgf_dwconv_bwd_data_f32).  One filter per channel: 9 or 49 multiply-adds per output and no reduction over channels, so
// these are streams over maps that sit in L2 / the infinity cache, not GEMMs -- plain VALU kernels, no LDS, no atomics, every sum in a
// fixed order (a sample's bits do not depend on the batch or on the grid).
//   3x3 / pad 1 / stride 1 | 2 forward: one lane per output COLUMN walks DW_ROWS output rows with the 3 x 3 input window in registers
//     (3 - stride rows carried over, `stride` rows loaded per output row); neighbouring lanes are neighbouring columns, so every load
//     and store of a wave is one contiguous row segment.
//   7x7 / pad 0 forward (the GDC head: a 7 x 7 map -> 1 x 1): one wave per plane, lane = filter tap, a butterfly sum per output.
//   data gradient (all three): one lane per input element gathers the <= ceil(k / stride)^2 outputs that saw it.
#include "mgf_common.h"

namespace {

constexpr int DW_ROWS = 4;      // output rows per lane of the 3x3 forward

__device__ __forceinline__ float dw_prelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// y = prelu_c(scale_c * conv3x3_pad1_stride_S(x)_c + shift_c);  x [planes, ih, iw], y [planes, oh, ow], w [c][9]
template <int S>
__global__ __launch_bounds__(256) void dw3x3_kernel(float* __restrict__ y, const float* __restrict__ x, const float* __restrict__ w,
                                                    const float* __restrict__ scale, const float* __restrict__ shift,
                                                    const float* __restrict__ slope, int c, int ih, int iw, int oh, int ow, int chunks,
                                                    int64_t items) {
    constexpr int KEEP = 3 - S;                    // window rows shared by consecutive output rows
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % ow);
        const int64_t r = i / ow;
        const int chunk = (int)(r % chunks);
        const int64_t pl = r / chunks;
        const int ch = (int)(pl % c);
        const float* xp = x + pl * ih * iw;
        float* yp = y + pl * oh * ow;
        float wv[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wv[k] = w[ch * 9 + k];
        const float sc = scale ? scale[ch] : 1.f, sh = shift ? shift[ch] : 0.f;
        const bool act = slope != nullptr;
        const float sl = act ? slope[ch] : 1.f;
        const int ixc = ox * S;                    // centre column: always inside the map
        const bool has_l = ixc >= 1, has_r = ixc + 1 < iw;
        const int oy0 = chunk * DW_ROWS;
        const int oy1 = oy0 + DW_ROWS < oh ? oy0 + DW_ROWS : oh;
        float win[3][3];
        auto load_row = [&](int k, int iy) {
            if (iy >= 0 && iy < ih) {
                const float* row = xp + (int64_t)iy * iw + ixc;
                win[k][0] = has_l ? row[-1] : 0.f;
                win[k][1] = row[0];
                win[k][2] = has_r ? row[1] : 0.f;
            } else {
                win[k][0] = win[k][1] = win[k][2] = 0.f;
            }
        };
#pragma unroll
        for (int k = 0; k < KEEP; ++k) load_row(k, oy0 * S - 1 + k);
        for (int oy = oy0; oy < oy1; ++oy) {
#pragma unroll
            for (int k = KEEP; k < 3; ++k) load_row(k, oy * S - 1 + k);
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) acc += wv[k] * win[k / 3][k % 3];
            float v = acc * sc + sh;
            if (act) v = dw_prelu(v, sl);
            yp[(int64_t)oy * ow + ox] = v;
#pragma unroll
            for (int k = 0; k < KEEP; ++k) {
                win[k][0] = win[k + S][0]; win[k][1] = win[k + S][1]; win[k][2] = win[k + S][2];
            }
        }
    }
}

// 7x7 / pad 0 / stride 1: one wave per plane, lane t < 49 holds tap (t / 7, t % 7); every output is a wave sum in butterfly order
__global__ __launch_bounds__(256) void dw7x7_kernel(float* __restrict__ y, const float* __restrict__ x, const float* __restrict__ w,
                                                    const float* __restrict__ scale, const float* __restrict__ shift,
                                                    const float* __restrict__ slope, int c, int ih, int iw, int oh, int ow, int64_t planes) {
    const int lane = threadIdx.x & 63;
    const bool live = lane < 49;
    const int kh = live ? lane / 7 : 0, kw = live ? lane % 7 : 0;
    for (int64_t pl = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); pl < planes; pl += (int64_t)gridDim.x * 4) {
        const int ch = (int)(pl % c);
        const float* xp = x + pl * ih * iw;
        const float wv = live ? w[ch * 49 + lane] : 0.f;
        const float sc = scale ? scale[ch] : 1.f, sh = shift ? shift[ch] : 0.f;
        for (int oy = 0; oy < oh; ++oy)
            for (int ox = 0; ox < ow; ++ox) {
                const float a = wave_sum(live ? wv * xp[(int64_t)(oy + kh) * iw + ox + kw] : 0.f);
                if (lane == 0) {
                    float v = a * sc + sh;
                    if (slope) v = dw_prelu(v, slope[ch]);
                    y[pl * oh * ow + (int64_t)oy * ow + ox] = v;
                }
            }
    }
}

// dx[iy, ix] = m_in * scale_c * sum_{oy, ox} w_c[iy + P - S oy][ix + P - S ox] * m_out[oy, ox] * dy[oy, ox] over the outputs whose K x K
// window holds (iy, ix), in (oy, ox) order.  m_out = (y > 0 ? 1 : slope_c) from the layer's own post-activation y (NULL: 1),
// m_in = (x_act > 0 ? 1 : x_slope_c) from the post-activation map the layer read (the PReLU in front of it; NULL: 1).
template <int K, int S, int P>
__global__ __launch_bounds__(256) void dw_bwd_kernel(float* __restrict__ dx, const float* __restrict__ dy, const float* __restrict__ w,
                                                     const float* __restrict__ scale, const float* __restrict__ y,
                                                     const float* __restrict__ slope, const float* __restrict__ x_act,
                                                     const float* __restrict__ x_slope, int c, int ih, int iw, int oh, int ow,
                                                     int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ix = (int)(i % iw);
        const int64_t r = i / iw;
        const int iy = (int)(r % ih);
        const int64_t pl = r / ih;
        const int ch = (int)(pl % c);
        const float* wc = w + ch * (K * K);
        const float* gp = dy + pl * oh * ow;
        const float* yp = y ? y + pl * oh * ow : nullptr;
        const float sl = y ? slope[ch] : 1.f;
        const int ty = iy + P - (K - 1), tx = ix + P - (K - 1);
        const int oy_lo = ty > 0 ? (ty + S - 1) / S : 0, ox_lo = tx > 0 ? (tx + S - 1) / S : 0;
        const int oy_hi = (iy + P) / S < oh - 1 ? (iy + P) / S : oh - 1;
        const int ox_hi = (ix + P) / S < ow - 1 ? (ix + P) / S : ow - 1;
        float acc = 0.f;
        for (int oy = oy_lo; oy <= oy_hi; ++oy) {
            const int kh = iy + P - oy * S;
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                const int kw = ix + P - ox * S;
                float g = gp[(int64_t)oy * ow + ox];
                if (yp) g = yp[(int64_t)oy * ow + ox] > 0.f ? g : g * sl;
                acc += wc[kh * K + kw] * g;
            }
        }
        if (scale) acc = acc * scale[ch];
        if (x_act) acc = x_act[i] > 0.f ? acc : acc * x_slope[ch];
        dx[i] = acc;
    }
}

// 3x3 pad 1 stride 1 | 2 and 7x7 pad 0 stride 1; 0 = not a geometry these kernels serve
int dw_geometry(int kh, int kw, int stride, int pad) {
    if (kh == 3 && kw == 3 && pad == 1 && (stride == 1 || stride == 2)) return stride;
    if (kh == 7 && kw == 7 && pad == 0 && stride == 1) return 7;
    return 0;
}

}  // namespace

#define MGF_DW_CHECK_GEOMETRY(name)                                                                                                        \
    MGF_REQUIRE(n >= 1 && c >= 1 && in_h >= 1 && in_w >= 1, MGF_EINVAL, name ": n, c, in_h, in_w must be positive (got %d, %d, %d, %d)",  \
                n, c, in_h, in_w);                                                                                                         \
    const int geo = dw_geometry(kh, kw, stride, pad);                                                                                     \
    MGF_REQUIRE(geo != 0, MGF_EINVAL, name ": kernel %dx%d stride %d pad %d is not built (3x3 pad 1 stride 1|2, 7x7 pad 0 stride 1)", kh, \
                kw, stride, pad);                                                                                                          \
    MGF_REQUIRE(in_h + 2 * pad >= kh && in_w + 2 * pad >= kw, MGF_EINVAL, name ": a %dx%d map gives an empty output under a %dx%d kernel " \
                "with pad %d", in_h, in_w, kh, kw, pad);                                                                                   \
    const int oh = (in_h + 2 * pad - kh) / stride + 1, ow = (in_w + 2 * pad - kw) / stride + 1;                                          \
    const int64_t planes = (int64_t)n * c

extern "C" int mgf_dwconv_f32(float* y, const float* x, const float* w, const float* scale, const float* shift, const float* slope, int32_t n,
                              int32_t c, int32_t in_h, int32_t in_w, int32_t kh, int32_t kw, int32_t stride, int32_t pad,
                              mgf_stream_t stream) {
    MGF_REQUIRE(y && x && w, MGF_EINVAL, "dwconv: y, x and w must not be NULL");
    MGF_DW_CHECK_GEOMETRY("dwconv");
    hipStream_t st = (hipStream_t)stream;
    if (geo == 7) {
        const int64_t blocks = mgf_cdiv(planes, 4);
        hipLaunchKernelGGL(dw7x7_kernel, dim3((unsigned)(blocks < MGF_NUM_CU * 8 ? blocks : MGF_NUM_CU * 8)), dim3(256), 0, st, y, x, w, scale,
                           shift, slope, c, in_h, in_w, oh, ow, planes);
    } else {
        const int chunks = (int)mgf_cdiv(oh, DW_ROWS);
        const int64_t items = planes * chunks * ow;
        const dim3 grid(mgf_stream_grid(items, 256, 1));
        if (geo == 1)
            hipLaunchKernelGGL(dw3x3_kernel<1>, grid, dim3(256), 0, st, y, x, w, scale, shift, slope, c, in_h, in_w, oh, ow, chunks, items);
        else
            hipLaunchKernelGGL(dw3x3_kernel<2>, grid, dim3(256), 0, st, y, x, w, scale, shift, slope, c, in_h, in_w, oh, ow, chunks, items);
    }
    MGF_CHECK_LAUNCH("dwconv");
    return MGF_OK;
}

extern "C" int mgf_dwconv_bwd_data_f32(float* dx, const float* dy, const float* w, const float* scale, const float* y, const float* slope,
                                       const float* x_act, const float* x_slope, int32_t n, int32_t c, int32_t in_h, int32_t in_w,
                                       int32_t kh, int32_t kw, int32_t stride, int32_t pad, mgf_stream_t stream) {
    MGF_REQUIRE(dx && dy && w, MGF_EINVAL, "dwconv_bwd_data: dx, dy and w must not be NULL");
    MGF_REQUIRE((y == nullptr) == (slope == nullptr), MGF_EINVAL, "dwconv_bwd_data: y and slope come together (the layer's own PReLU)");
    MGF_REQUIRE((x_act == nullptr) == (x_slope == nullptr), MGF_EINVAL,
                "dwconv_bwd_data: x_act and x_slope come together (the PReLU in front of the layer)");
    MGF_DW_CHECK_GEOMETRY("dwconv_bwd_data");
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = planes * in_h * in_w;
    const dim3 grid(mgf_stream_grid(total, 256, 1));
    if (geo == 1)
        hipLaunchKernelGGL((dw_bwd_kernel<3, 1, 1>), grid, dim3(256), 0, st, dx, dy, w, scale, y, slope, x_act, x_slope, c, in_h, in_w, oh, ow,
                           total);
    else if (geo == 2)
        hipLaunchKernelGGL((dw_bwd_kernel<3, 2, 1>), grid, dim3(256), 0, st, dx, dy, w, scale, y, slope, x_act, x_slope, c, in_h, in_w, oh, ow,
                           total);
    else
        hipLaunchKernelGGL((dw_bwd_kernel<7, 1, 0>), grid, dim3(256), 0, st, dx, dy, w, scale, y, slope, x_act, x_slope, c, in_h, in_w, oh, ow,
                           total);
    MGF_CHECK_LAUNCH("dwconv_bwd_data");
    return MGF_OK;
}
