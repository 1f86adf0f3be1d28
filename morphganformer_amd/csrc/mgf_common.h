// Shared host/device helpers for the gfx950 kernels.  CDNA4 only: wave = 64 lanes, 256 CUs in 8 XCDs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/mgf.h"

#define MGF_WAVE 64
#define MGF_NUM_CU 256
#define MGF_NUM_XCD 8

void mgf_set_error(const char* fmt, ...);

#define MGF_REQUIRE(cond, code, ...)            \
    do {                                         \
        if (!(cond)) {                           \
            mgf_set_error(__VA_ARGS__);          \
            return (code);                       \
        }                                        \
    } while (0)

#define MGF_CHECK_LAUNCH(name)                                                        \
    do {                                                                              \
        hipError_t e_ = hipGetLastError();                                            \
        if (e_ != hipSuccess) {                                                       \
            mgf_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));      \
            return MGF_ELAUNCH;                                                       \
        }                                                                             \
    } while (0)

static inline int64_t mgf_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Dispatch knobs (tile shapes, split-K thresholds, kernel choices).  In the product library every knob IS its measured default:
// mgf_knob() returns nullptr at compile time and the `static const` it initialises folds to the constant -- nothing reads the environment.
// Only the experiment library of tools/build_exp.sh (-DMGF_TUNING_HOOKS, exp_build/, never the product's object cache) looks the name up,
// so that tools/*_micro.py can sweep a knob without a rebuild.
#ifdef MGF_TUNING_HOOKS
#include <stdlib.h>
static inline const char* mgf_knob(const char* name) { return getenv(name); }
#else
static inline constexpr const char* mgf_knob(const char*) { return nullptr; }
#endif

// Grid size for a grid-stride streaming kernel: enough workgroups to fill 256 CUs x 8, no more.
static inline int mgf_stream_grid(int64_t work_items, int block, int per_thread) {
    int64_t g = mgf_cdiv(work_items, (int64_t)block * per_thread);
    int64_t cap = (int64_t)MGF_NUM_CU * 8;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

// instrumentation hooks of mgf_conv_profile_begin/end for convolution kernels outside conv_taps.hip (no-ops unless profiling is on)
void mgf_prof_external_begin(hipStream_t st, const char* name, double flops, double bytes);
void mgf_prof_external_end(hipStream_t st);

// form-3 Winograd launch whose kernel choice depends on the layer's shape only (wino3.hip; the MDF body layers of mdf.hip)
int mgf_wino3_batch_invariant_f32(float* y, const float* x, const float* u, int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout,
                                  const mgf_epilogue* ep, mgf_stream_t stream);
// ... with the masked epilogue of the MDF backward: y = conv_pad1(x, u) * (mask > 0 ? 1 : slope) on ring `ring`, 0 outside (cin = cout = c)
int mgf_wino3_batch_invariant_masked_f32(float* y, const float* x, const float* u, const float* mask, int32_t n, int32_t c, int32_t h, int32_t w,
                                         int32_t ring, float slope, mgf_stream_t stream);

#ifdef __HIPCC__
// Sum over the 64 lanes of a wave (DPP/bpermute butterflies emitted by the compiler for __shfl_xor).
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Sum over the 256 threads of a workgroup in a fixed order (wave butterflies, then the four waves in index order) through four slots of
// LDS; every thread gets the result.  The first barrier lets `sh` still be read from a previous call.
template <typename T>
__device__ __forceinline__ T mgf_block_sum_256(T v, T* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
// The same sum as a halving tree over 256 slots of LDS (`t`: the thread's index 0..255): another order than mgf_block_sum_256, the one the
// float64 partial sums of DSSIM, MS-SSIM and MDF are pinned to.  Every thread gets the result; `red` is free again on return.
template <typename T>
__device__ __forceinline__ T mgf_block_tree_sum_256(T v, T* red, int t = threadIdx.x) {
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const T r = red[0];
    __syncthreads();
    return r;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { T u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
    return v;
}
#endif
