// The coupling of reference-based latent de-morphing (gradient mode, demorph.py): generator rows that are linear mixes of latent parameters.
//   mgf_latent_mix_f32       rows[b, i]    = sum_p coef[b, p] * params[p, i]                              float32, every product rounded, p order
//   mgf_latent_mix_bwd_f32   dparams[p, i] = f32( sum_b (f64(row_weight[b]) * f64(coef[b, p])) * f64(drows[b, i]) )   float64, b order, one rounding
//   mgf_joint_losses_f32     the three one-candidate loss slots of mgf_select_best as row-weighted sums of the per-row slots (float64, b order),
//                            and the per-row totals of the step for the trace
// At most 8 rows and 8 parameters (the coefficient matrix sits in LDS); no atomics, fixed summation order, and no contraction:
// every product and sum is spelled with a rounding intrinsic, so the results equal the stated expressions bit for bit.  The latent is 544 floats
// in z and 9 792 in W+: a handful of workgroups; any numel >= 1 works (float4 body where the rows are 16-byte aligned, else scalar).
#include "mgf_common.h"

#include <math.h>

namespace {

constexpr int MIX_MAX = 8;

__device__ __forceinline__ float mix_one(const float* c, const float* __restrict__ params, int n_params, int64_t numel, int64_t i) {
    float acc = __fmul_rn(c[0], params[i]);
    for (int p = 1; p < n_params; ++p) acc = __fadd_rn(acc, __fmul_rn(c[p], params[(int64_t)p * numel + i]));
    return acc;
}

__global__ __launch_bounds__(256) void latent_mix_kernel(float* __restrict__ rows, const float* __restrict__ params, const float* __restrict__ coef,
                                                         int n_rows, int n_params, int64_t numel, int vec) {
    __shared__ float c[MIX_MAX * MIX_MAX];
    if (threadIdx.x < n_rows * n_params) c[threadIdx.x] = coef[threadIdx.x];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * 256, tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (vec) {
        const int64_t n4 = numel >> 2;
        for (int64_t q = tid; q < n4; q += stride) {
            for (int b = 0; b < n_rows; ++b) {              // (the parameters are read once per row: a few KB, from the cache)
                const float* cb = c + b * n_params;
                float4 x = reinterpret_cast<const float4*>(params)[q], a;
                a.x = __fmul_rn(cb[0], x.x); a.y = __fmul_rn(cb[0], x.y); a.z = __fmul_rn(cb[0], x.z); a.w = __fmul_rn(cb[0], x.w);
                for (int p = 1; p < n_params; ++p) {
                    x = reinterpret_cast<const float4*>(params + (int64_t)p * numel)[q];
                    a.x = __fadd_rn(a.x, __fmul_rn(cb[p], x.x)); a.y = __fadd_rn(a.y, __fmul_rn(cb[p], x.y));
                    a.z = __fadd_rn(a.z, __fmul_rn(cb[p], x.z)); a.w = __fadd_rn(a.w, __fmul_rn(cb[p], x.w));
                }
                reinterpret_cast<float4*>(rows + (int64_t)b * numel)[q] = a;
            }
        }
    } else {
        for (int64_t i = tid; i < numel; i += stride)
            for (int b = 0; b < n_rows; ++b) rows[(int64_t)b * numel + i] = mix_one(c + b * n_params, params, n_params, numel, i);
    }
}

__global__ __launch_bounds__(256) void latent_mix_bwd_kernel(float* __restrict__ dparams, const float* __restrict__ drows,
                                                             const float* __restrict__ coef, const float* __restrict__ row_weight, int n_rows,
                                                             int n_params, int64_t numel, int vec) {
    __shared__ double wc[MIX_MAX * MIX_MAX];            // wc[b, p] = f64(row_weight[b]) * f64(coef[b, p])
    if (threadIdx.x < n_rows * n_params) {
        const int b = threadIdx.x / n_params;
        wc[threadIdx.x] = __dmul_rn(row_weight ? (double)row_weight[b] : 1.0, (double)coef[threadIdx.x]);
    }
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * 256, tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (vec) {
        const int64_t n4 = numel >> 2;
        for (int64_t q = tid; q < n4; q += stride) {
            for (int p = 0; p < n_params; ++p) {
                float4 g = reinterpret_cast<const float4*>(drows)[q];
                double ax = __dmul_rn(wc[p], (double)g.x), ay = __dmul_rn(wc[p], (double)g.y);
                double az = __dmul_rn(wc[p], (double)g.z), aw = __dmul_rn(wc[p], (double)g.w);
                for (int b = 1; b < n_rows; ++b) {
                    const double w = wc[b * n_params + p];
                    g = reinterpret_cast<const float4*>(drows + (int64_t)b * numel)[q];
                    ax = __dadd_rn(ax, __dmul_rn(w, (double)g.x)); ay = __dadd_rn(ay, __dmul_rn(w, (double)g.y));
                    az = __dadd_rn(az, __dmul_rn(w, (double)g.z)); aw = __dadd_rn(aw, __dmul_rn(w, (double)g.w));
                }
                float4 o;
                o.x = (float)ax; o.y = (float)ay; o.z = (float)az; o.w = (float)aw;
                reinterpret_cast<float4*>(dparams + (int64_t)p * numel)[q] = o;
            }
        }
    } else {
        for (int64_t i = tid; i < numel; i += stride)
            for (int p = 0; p < n_params; ++p) {
                double acc = __dmul_rn(wc[p], (double)drows[i]);
                for (int b = 1; b < n_rows; ++b) acc = __dadd_rn(acc, __dmul_rn(wc[b * n_params + p], (double)drows[(int64_t)b * numel + i]));
                dparams[(int64_t)p * numel + i] = (float)acc;
            }
    }
}

// one thread: a dozen scalar operations on the loss slots
__global__ void joint_losses_kernel(float* __restrict__ p_joint, double* __restrict__ w_joint, float* __restrict__ mse_joint,
                                    double* __restrict__ row_totals, const float* __restrict__ p_loss, const double* __restrict__ w_loss,
                                    const float* __restrict__ mse_loss, const float* __restrict__ row_weight, double lamda, float beta,
                                    const int32_t* __restrict__ step, const int32_t* __restrict__ valid, int n_rows, int steps_total) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int s = *step;
    if (s >= steps_total || s < 0) return;
    double pj = 0.0, wj = 0.0, mj = 0.0;
    for (int b = 0; b < n_rows; ++b) {
        const double rw = row_weight ? (double)row_weight[b] : 1.0;
        if (p_loss) { const double t = __dmul_rn(rw, (double)p_loss[b]); pj = b ? __dadd_rn(pj, t) : t; }
        if (w_loss) { const double t = __dmul_rn(rw, w_loss[b]); wj = b ? __dadd_rn(wj, t) : t; }
        if (mse_loss) { const double t = __dmul_rn(rw, (double)mse_loss[b]); mj = b ? __dadd_rn(mj, t) : t; }
    }
    if (p_joint) *p_joint = (float)pj;
    if (w_joint) *w_joint = wj;
    if (mse_joint) *mse_joint = (float)mj;
    if (row_totals) {
        const int ok = valid ? valid[s] : 1;
        for (int b = 0; b < n_rows; ++b) {
            // mgf_select_best's expression for one row: the same evaluation order and promotions
            double total = 0.0;
            if (p_loss) total = __dadd_rn(total, (double)p_loss[b]);
            if (w_loss) total = __dadd_rn(total, __dmul_rn(lamda, w_loss[b]));
            if (mse_loss) total = __dadd_rn(total, (double)__fmul_rn(beta, mse_loss[b]));
            row_totals[(int64_t)b * steps_total + s] = ok ? total : __longlong_as_double(0x7ff8000000000000LL);
        }
    }
}

// [a, a + na) and [b, b + nb) bytes share an address
inline bool mix_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

inline int mix_grid(int64_t numel, int vec) {
    const int64_t g = mgf_cdiv(vec ? numel >> 2 : numel, 256);
    return (int)(g < 1 ? 1 : (g > 64 ? 64 : g));
}

}  // namespace

extern "C" int mgf_latent_mix_f32(float* rows, const float* params, const float* coef, int32_t n_rows, int32_t n_params, int64_t numel,
                                  mgf_stream_t stream) {
    MGF_REQUIRE(rows && params && coef, MGF_EINVAL, "latent_mix: rows, params and coef must not be NULL");
    MGF_REQUIRE(n_rows >= 1 && n_rows <= MIX_MAX && n_params >= 1 && n_params <= MIX_MAX, MGF_EINVAL,
                "latent_mix: n_rows and n_params must lie in 1..%d (got %d, %d)", MIX_MAX, n_rows, n_params);
    MGF_REQUIRE(numel >= 1, MGF_EINVAL, "latent_mix: numel must be >= 1 (got %lld)", (long long)numel);
    const int64_t rb = (int64_t)n_rows * numel * 4, pb = (int64_t)n_params * numel * 4, cb = (int64_t)n_rows * n_params * 4;
    MGF_REQUIRE(!mix_overlap(rows, rb, params, pb) && !mix_overlap(rows, rb, coef, cb), MGF_EINVAL,
                "latent_mix: rows must not alias params or coef (every row reads every parameter)");
    const int vec = (numel & 3) == 0 && ((((uintptr_t)rows | (uintptr_t)params) & 15) == 0);
    hipLaunchKernelGGL(latent_mix_kernel, dim3(mix_grid(numel, vec)), dim3(256), 0, (hipStream_t)stream, rows, params, coef, (int)n_rows,
                       (int)n_params, numel, vec);
    MGF_CHECK_LAUNCH("latent_mix");
    return MGF_OK;
}

extern "C" int mgf_latent_mix_bwd_f32(float* dparams, const float* drows, const float* coef, const float* row_weight, int32_t n_rows,
                                      int32_t n_params, int64_t numel, mgf_stream_t stream) {
    MGF_REQUIRE(dparams && drows && coef, MGF_EINVAL, "latent_mix_bwd: dparams, drows and coef must not be NULL");
    MGF_REQUIRE(n_rows >= 1 && n_rows <= MIX_MAX && n_params >= 1 && n_params <= MIX_MAX, MGF_EINVAL,
                "latent_mix_bwd: n_rows and n_params must lie in 1..%d (got %d, %d)", MIX_MAX, n_rows, n_params);
    MGF_REQUIRE(numel >= 1, MGF_EINVAL, "latent_mix_bwd: numel must be >= 1 (got %lld)", (long long)numel);
    const int64_t rb = (int64_t)n_rows * numel * 4, pb = (int64_t)n_params * numel * 4, cb = (int64_t)n_rows * n_params * 4;
    MGF_REQUIRE(!mix_overlap(dparams, pb, drows, rb) && !mix_overlap(dparams, pb, coef, cb) && !mix_overlap(dparams, pb, row_weight, n_rows * 4),
                MGF_EINVAL, "latent_mix_bwd: dparams must not alias drows, coef or row_weight (every parameter reads every row)");
    const int vec = (numel & 3) == 0 && ((((uintptr_t)dparams | (uintptr_t)drows) & 15) == 0);
    hipLaunchKernelGGL(latent_mix_bwd_kernel, dim3(mix_grid(numel, vec)), dim3(256), 0, (hipStream_t)stream, dparams, drows, coef, row_weight,
                       (int)n_rows, (int)n_params, numel, vec);
    MGF_CHECK_LAUNCH("latent_mix_bwd");
    return MGF_OK;
}

extern "C" int mgf_joint_losses_f32(float* p_joint, double* w_joint, float* mse_joint, double* row_totals, const float* p_loss,
                                    const double* w_loss, const float* mse_loss, const float* row_weight, double lamda, float beta,
                                    const int32_t* step, const int32_t* valid, int32_t n_rows, int32_t steps_total, mgf_stream_t stream) {
    MGF_REQUIRE(step, MGF_EINVAL, "joint_losses: the step counter must not be NULL");
    MGF_REQUIRE(n_rows >= 1 && n_rows <= MIX_MAX && steps_total >= 1, MGF_EINVAL, "joint_losses: n_rows must lie in 1..%d and steps_total be >= 1 (got %d, %d)",
                MIX_MAX, n_rows, steps_total);
    MGF_REQUIRE((!p_joint) == (!p_loss) && (!w_joint) == (!w_loss) && (!mse_joint) == (!mse_loss), MGF_EINVAL,
                "joint_losses: a joint slot and its per-row slot come together or not at all");
    MGF_REQUIRE(p_loss || w_loss || mse_loss, MGF_EINVAL, "joint_losses: no loss slot given");
    MGF_REQUIRE(!mix_overlap(p_joint, 4, p_loss, n_rows * 4) && !mix_overlap(mse_joint, 4, mse_loss, n_rows * 4) &&
                !mix_overlap(w_joint, 8, w_loss, n_rows * 8) && !mix_overlap(p_joint, 4, mse_loss, n_rows * 4) &&
                !mix_overlap(mse_joint, 4, p_loss, n_rows * 4), MGF_EINVAL,
                "joint_losses: a joint slot must not alias a per-row slot (the row totals read the rows after the joint slots are written)");
    hipLaunchKernelGGL(joint_losses_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p_joint, w_joint, mse_joint, row_totals, p_loss, w_loss,
                       mse_loss, row_weight, lamda, beta, step, valid, (int)n_rows, (int)steps_total);
    MGF_CHECK_LAUNCH("joint_losses");
    return MGF_OK;
}
