// Block mean in front of the LPIPS backbone (PerceptualLoss(pool_above=N); projection_example_v1.py:148-155) and its adjoint.
//   mgf_block_mean_f32          out[p, Y, X] = (1 / f^2) sum_{dy < f} sum_{dx < f} x[p, Y f + dy, X f + dx]
//   mgf_block_mean_adjoint_f32  dx[p, y, x] (+)= dy[p, y / f, x / f] / f^2 where y / f < gh and x / f < gw, (+)= 0 elsewhere
// Both are pure HBM streams: grid-stride loops over a work list sized by the tensor, at most MGF_NUM_CU x 8 workgroups, no LDS, no atomics.
// The vector bodies (f = 2, 4, 8; the contiguous tensor 16-byte aligned with w % 4 == 0) move one float4 per lane and row; the scalar bodies
// take any f, width and alignment, one element of the contiguous tensor per lane.
//
// Summation order of the forward (one order, every body): a block's columns are cut into runs of four from the left (the last run holds
// f % 4 columns when that is not 0; f = 2 is one run of two).  Within a row a run is summed left to right, ((a + b) + c) + d; a run is
// accumulated over the block's rows from the top, c_j = ((q_j0 + q_j1) + q_j2) + ...; the runs are added from the left, s = ((c_0 + c_1) + c_2)
// + ...; out = s / f^2 (one correctly rounded division; a multiplication by the exact 1 / f^2 for a power of two).  Nothing in it depends on
// the grid, on the plane count or on which body ran.
#include "mgf_common.h"

#include <limits.h>

namespace {

constexpr int BP_BLOCK = 256;

__device__ __forceinline__ float run_of(const float4& v) { return ((v.x + v.y) + v.z) + v.w; }

// ---- forward, vector bodies: item = (output row, float4 column of the input row)
template <int F>
__global__ __launch_bounds__(BP_BLOCK) void block_mean_vec_kernel(float* __restrict__ out, const float* __restrict__ x, int items, int w4) {
    const int stride = gridDim.x * BP_BLOCK;
    const int64_t w = (int64_t)w4 * 4;
    for (int i = blockIdx.x * BP_BLOCK + threadIdx.x; i < items; i += stride) {
        const int row = i / w4, c4 = i - row * w4;                  // row = p * (h / F) + Y: the block's first input row is row * F
        const float* src = x + (int64_t)row * F * w + (int64_t)c4 * 4;
        float4 v[F];
#pragma unroll
        for (int dy = 0; dy < F; ++dy) v[dy] = *reinterpret_cast<const float4*>(src + dy * w);
        if constexpr (F == 2) {                                     // two blocks per float4, each one run of two
            const float a = (v[0].x + v[0].y) + (v[1].x + v[1].y);
            const float b = (v[0].z + v[0].w) + (v[1].z + v[1].w);
            *reinterpret_cast<float2*>(out + (int64_t)row * (w4 * 2) + c4 * 2) = make_float2(a / 4.f, b / 4.f);
        } else {
            float c = run_of(v[0]);
#pragma unroll
            for (int dy = 1; dy < F; ++dy) c = c + run_of(v[dy]);
            if constexpr (F == 4) {
                out[(int64_t)row * w4 + c4] = c / 16.f;
            } else {                                                // F == 8: lanes 2k and 2k + 1 hold the block's two runs (items and stride are even)
                const float other = __shfl_xor(c, 1, 64);
                if ((c4 & 1) == 0) out[(int64_t)row * (w4 / 2) + c4 / 2] = (c + other) / 64.f;
            }
        }
    }
}

// ---- forward, scalar body: item = output pixel
__global__ __launch_bounds__(BP_BLOCK) void block_mean_scalar_kernel(float* __restrict__ out, const float* __restrict__ x, int items, int wo, int f) {
    const int stride = gridDim.x * BP_BLOCK;
    const int64_t w = (int64_t)wo * f;
    const float ff = (float)(f * f);
    for (int i = blockIdx.x * BP_BLOCK + threadIdx.x; i < items; i += stride) {
        const int row = i / wo, X = i - row * wo;
        const float* src = x + (int64_t)row * f * w + (int64_t)X * f;
        float s = 0.f;
        for (int j = 0; j < f; j += 4) {
            const int len = f - j < 4 ? f - j : 4;
            float c = 0.f;
            for (int dy = 0; dy < f; ++dy) {
                const float* r = src + dy * w + j;
                float q = r[0];
                for (int k = 1; k < len; ++k) q = q + r[k];
                c = dy == 0 ? q : c + q;
            }
            s = j == 0 ? c : s + c;
        }
        out[i] = s / ff;
    }
}

// ---- adjoint, vector bodies: item = float4 of dx
template <int F>
__global__ __launch_bounds__(BP_BLOCK) void block_mean_adjoint_vec_kernel(float* __restrict__ dx, const float* __restrict__ dy, int items, int w4, int h,
                                                                           int gh, int gw, int64_t pitch, int64_t plane, int accumulate) {
    const int stride = gridDim.x * BP_BLOCK;
    constexpr float FF = (float)(F * F);
    for (int i = blockIdx.x * BP_BLOCK + threadIdx.x; i < items; i += stride) {
        const int row = i / w4, c4 = i - row * w4;                  // row = p * h + y
        const int p = row / h, y = row - p * h;
        const int Y = y / F, X0 = (c4 * 4) / F;
        float4* dst = reinterpret_cast<float4*>(dx) + i;
        const bool any = Y < gh && X0 < gw;
        if (!any) {
            if (!accumulate) *dst = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;                                               // accumulate: the uncovered pixels stay as they are
        }
        const float* g = dy + (int64_t)p * plane + (int64_t)Y * pitch;
        float4 add;
        bool hi = true;                                             // F == 2: columns 2, 3 belong to block X0 + 1, which the crop may exclude
        if constexpr (F == 2) {
            const float a = g[X0] / FF;
            hi = X0 + 1 < gw;
            const float b = hi ? g[X0 + 1] / FF : 0.f;
            add = make_float4(a, a, b, b);
        } else {
            const float a = g[X0] / FF;
            add = make_float4(a, a, a, a);
        }
        if (accumulate) {
            const float4 o = *dst;
            *dst = make_float4(o.x + add.x, o.y + add.y, hi ? o.z + add.z : o.z, hi ? o.w + add.w : o.w);
        } else {
            *dst = add;
        }
    }
}

// ---- adjoint, scalar body: item = element of dx
__global__ __launch_bounds__(BP_BLOCK) void block_mean_adjoint_scalar_kernel(float* __restrict__ dx, const float* __restrict__ dy, int items, int w, int h,
                                                                              int f, int gh, int gw, int64_t pitch, int64_t plane, int accumulate) {
    const int stride = gridDim.x * BP_BLOCK;
    const float ff = (float)(f * f);
    for (int i = blockIdx.x * BP_BLOCK + threadIdx.x; i < items; i += stride) {
        const int row = i / w, xx = i - row * w;
        const int p = row / h, y = row - p * h;
        const int Y = y / f, X = xx / f;
        if (Y < gh && X < gw) {
            const float a = dy[(int64_t)p * plane + (int64_t)Y * pitch + X] / ff;
            dx[i] = accumulate ? dx[i] + a : a;
        } else if (!accumulate) {
            dx[i] = 0.f;
        }
    }
}

int check_geometry(const char* name, int32_t planes, int32_t h, int32_t w, int32_t f) {
    MGF_REQUIRE(planes >= 1 && h >= 1 && w >= 1, MGF_EINVAL, "%s: planes, h and w must be >= 1 (got %d, %d, %d)", name, planes, h, w);
    MGF_REQUIRE(f >= 2, MGF_EINVAL, "%s: the block side f must be >= 2 (got %d)", name, f);
    MGF_REQUIRE(h % f == 0 && w % f == 0, MGF_EINVAL, "%s: %d x %d is not a whole number of %d x %d blocks", name, h, w, f, f);
    MGF_REQUIRE((int64_t)planes * h * w <= INT32_MAX, MGF_EINVAL, "%s: %d planes of %d x %d exceed the 32-bit index range", name, planes, h, w);
    return MGF_OK;
}

inline bool aligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

}  // namespace

extern "C" int mgf_block_mean_f32(float* out, const float* x, int32_t planes, int32_t h, int32_t w, int32_t f, mgf_stream_t stream) {
    MGF_REQUIRE(out && x, MGF_EINVAL, "block_mean: out and x must not be NULL");
    if (int rc = check_geometry("block_mean", planes, h, w, f)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int rows = planes * (h / f);                              // output rows; <= planes * h * w / f^2
    const bool vec = (f == 2 || f == 4 || f == 8) && w % 4 == 0 && aligned(x, 16) && (f != 2 || aligned(out, 8));
    if (vec) {
        const int w4 = w / 4, items = rows * w4;
        const dim3 grid(mgf_stream_grid(items, BP_BLOCK, 1)), block(BP_BLOCK);
        if (f == 2) hipLaunchKernelGGL(block_mean_vec_kernel<2>, grid, block, 0, st, out, x, items, w4);
        else if (f == 4) hipLaunchKernelGGL(block_mean_vec_kernel<4>, grid, block, 0, st, out, x, items, w4);
        else hipLaunchKernelGGL(block_mean_vec_kernel<8>, grid, block, 0, st, out, x, items, w4);
    } else {
        const int wo = w / f, items = rows * wo;
        hipLaunchKernelGGL(block_mean_scalar_kernel, dim3(mgf_stream_grid(items, BP_BLOCK, 1)), dim3(BP_BLOCK), 0, st, out, x, items, wo, (int)f);
    }
    MGF_CHECK_LAUNCH("block_mean");
    return MGF_OK;
}

extern "C" int mgf_block_mean_adjoint_f32(float* dx, const float* dy, int32_t planes, int32_t h, int32_t w, int32_t f, int32_t gh, int32_t gw,
                                          int64_t dy_row_pitch, int64_t dy_plane_stride, int32_t accumulate, mgf_stream_t stream) {
    MGF_REQUIRE(dx && dy, MGF_EINVAL, "block_mean_adjoint: dx and dy must not be NULL");
    if (int rc = check_geometry("block_mean_adjoint", planes, h, w, f)) return rc;
    MGF_REQUIRE(gh >= 1 && gw >= 1 && gh <= h / f && gw <= w / f, MGF_EINVAL,
                "block_mean_adjoint: dy's extent %d x %d must lie in 1..%d x 1..%d (dx is %d x %d, f = %d)", gh, gw, h / f, w / f, h, w, f);
    MGF_REQUIRE(dy_row_pitch >= gw && (planes == 1 || dy_plane_stride >= (int64_t)(gh - 1) * dy_row_pitch + gw), MGF_EINVAL,
                "block_mean_adjoint: dy's row pitch %lld / plane stride %lld cannot hold %d planes of %d x %d", (long long)dy_row_pitch,
                (long long)dy_plane_stride, planes, gh, gw);
    hipStream_t st = (hipStream_t)stream;
    const int rows = planes * h;
    const bool vec = (f == 2 || f == 4 || f == 8) && w % 4 == 0 && aligned(dx, 16);
    if (vec) {
        const int w4 = w / 4, items = rows * w4;
        const dim3 grid(mgf_stream_grid(items, BP_BLOCK, 1)), block(BP_BLOCK);
#define BP_ADJ(F) hipLaunchKernelGGL(block_mean_adjoint_vec_kernel<F>, grid, block, 0, st, dx, dy, items, w4, (int)h, (int)gh, (int)gw, \
                                     (int64_t)dy_row_pitch, (int64_t)dy_plane_stride, (int)accumulate)
        if (f == 2) BP_ADJ(2);
        else if (f == 4) BP_ADJ(4);
        else BP_ADJ(8);
#undef BP_ADJ
    } else {
        const int items = rows * w;
        hipLaunchKernelGGL(block_mean_adjoint_scalar_kernel, dim3(mgf_stream_grid(items, BP_BLOCK, 1)), dim3(BP_BLOCK), 0, st, dx, dy, items, (int)w,
                           (int)h, (int)f, (int)gh, (int)gw, (int64_t)dy_row_pitch, (int64_t)dy_plane_stride, (int)accumulate);
    }
    MGF_CHECK_LAUNCH("block_mean_adjoint");
    return MGF_OK;
}
