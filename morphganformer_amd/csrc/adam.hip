// torch.optim.Adam.step() of gradient mode, device-resident (1024_example_wing_loss_perceptual_sqz_MSE.py:146,181-184; amsgrad off,
// weight_decay optional as L2 like torch, 1024_example_MSE.py:117): the learning rate comes from a table indexed by the device step counter,
// a step past the end or marked invalid ("no face": `continue` before optimizer.step()) changes nothing, and the optimizer's own step count
// lives on the device and only advances when a step is taken.
//   mgf_adam_step_f32          one workgroup, for latent-sized parameters; advances the count itself
//   mgf_adam_elementwise_f32   any number of workgroups; the count is advanced by a launch of its own behind the update
//   mgf_adam_sets_f32          the same over n_sets slices, each with its own count, step counter and `valid` row
// All three run ONE statement of the update (adam_update), so a tensor that two of them accept gets the same bits from both.
// Contract: include/mgf.h (mgf_adam_step_f32, mgf_adam_elementwise_f32, "Per-target noise maps": mgf_adam_sets_f32).
#include "mgf_common.h"

#include <math.h>

namespace {

// Elements first, first + stride, ... of one parameter.  Returns the new step count, 0 when no step is taken (uniform over the launch).
__device__ __forceinline__ int adam_update(float* param, float* m, float* v, const int32_t* t_ctr, const float* grad, const float* lr_table,
                                           const int32_t* step, const int32_t* valid, int64_t numel, int steps_total, float beta1, float beta2,
                                           float eps, float weight_decay, int64_t first, int64_t stride) {
    const int s = *step;
    if (s >= steps_total || (valid && valid[s] == 0)) return 0;
    const int t = *t_ctr + 1;
    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
    const float step_size = (float)((double)lr_table[s] / bc1);
    const float bc2_sqrt = (float)sqrt(bc2);
    for (int64_t i = first; i < numel; i += stride) {
        float g = grad[i];
        if (weight_decay != 0.f) g += weight_decay * param[i];
        const float mi = m[i] + (g - m[i]) * (1.f - beta1);                 // exp_avg.lerp_(grad, 1 - beta1)
        const float vi = v[i] * beta2 + (1.f - beta2) * g * g;
        m[i] = mi;
        v[i] = vi;
        param[i] -= step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
    }
    return t;
}

// One workgroup: every lane has read the count before lane 0 writes the new one.
__global__ __launch_bounds__(256) void adam_step_kernel(float* param, float* m, float* v, int32_t* t_ctr, const float* grad, const float* lr_table,
                                                        const int32_t* step, const int32_t* valid, int64_t numel, int steps_total, float beta1,
                                                        float beta2, float eps, float weight_decay) {
    const int t = adam_update(param, m, v, t_ctr, grad, lr_table, step, valid, numel, steps_total, beta1, beta2, eps, weight_decay, threadIdx.x, 256);
    __syncthreads();
    if (t && threadIdx.x == 0) *t_ctr = t;
}

// Slice blockIdx.y of n_sets: its own optimizer count, step counter and `valid` row (one slice: n_sets = 1, strides 0).  No block may see
// the new count: adam_sets_advance_kernel writes it behind this launch.
__global__ __launch_bounds__(256) void adam_sets_kernel(float* param, float* m, float* v, const int32_t* t_ctr, const float* grad, const float* lr_table,
                                                        const int32_t* step, int64_t step_stride, const int32_t* valid, int64_t valid_stride,
                                                        int64_t numel, int64_t set_stride, int steps_total, float beta1, float beta2, float eps,
                                                        float weight_decay) {
    const int64_t t = blockIdx.y, o = t * set_stride;
    adam_update(param + o, m + o, v + o, t_ctr + t, grad + o, lr_table, step + t * step_stride, valid ? valid + t * valid_stride : nullptr,
                numel, steps_total, beta1, beta2, eps, weight_decay, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256);
}

__global__ void adam_sets_advance_kernel(int32_t* t_ctr, const int32_t* step, int64_t step_stride, const int32_t* valid, int64_t valid_stride,
                                         int n_sets, int steps_total) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_sets) return;
    const int s = step[t * step_stride];
    if (s >= steps_total || (valid && valid[t * valid_stride + s] == 0)) return;
    t_ctr[t] = t_ctr[t] + 1;
}

void launch_adam_sets(float* param, float* m, float* v, int32_t* t_ctr, const float* grad, const float* lr_table, const int32_t* step,
                      int64_t step_stride, const int32_t* valid, int64_t valid_stride, int64_t numel, int n_sets, int64_t set_stride, int steps_total,
                      float beta1, float beta2, float eps, float weight_decay, hipStream_t st) {
    hipLaunchKernelGGL(adam_sets_kernel, dim3(mgf_stream_grid(numel, 256, 4), n_sets), dim3(256), 0, st, param, m, v, (const int32_t*)t_ctr, grad,
                       lr_table, step, step_stride, valid, valid_stride, numel, set_stride, steps_total, beta1, beta2, eps, weight_decay);
    hipLaunchKernelGGL(adam_sets_advance_kernel, dim3((n_sets + 255) / 256), dim3(256), 0, st, t_ctr, step, step_stride, valid, valid_stride, n_sets,
                       steps_total);
}

}  // namespace

extern "C" int mgf_adam_step_f32(float* param, float* exp_avg, float* exp_avg_sq, int32_t* adam_t, const float* grad, const float* lr_table,
                                 const int32_t* step, const int32_t* valid, int64_t numel, int32_t steps_total, float beta1, float beta2,
                                 float eps, float weight_decay, mgf_stream_t stream) {
    MGF_REQUIRE(param && exp_avg && exp_avg_sq && adam_t && grad && lr_table && step, MGF_EINVAL, "adam_step: null pointer");
    MGF_REQUIRE(numel >= 1 && steps_total >= 1, MGF_EINVAL, "adam_step: bad sizes");
    MGF_REQUIRE(numel <= (1 << 20), MGF_EUNSUPPORTED, "adam_step: single-workgroup kernel for latent-sized parameters (numel <= 2^20)");
    hipLaunchKernelGGL(adam_step_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, param, exp_avg, exp_avg_sq, adam_t, grad, lr_table, step,
                       valid, numel, steps_total, beta1, beta2, eps, weight_decay);
    MGF_CHECK_LAUNCH("adam_step");
    return MGF_OK;
}

extern "C" int mgf_adam_elementwise_f32(float* param, float* exp_avg, float* exp_avg_sq, int32_t* adam_t, const float* grad, const float* lr_table,
                                        const int32_t* step, const int32_t* valid, int64_t numel, int32_t steps_total, float beta1, float beta2,
                                        float eps, float weight_decay, mgf_stream_t stream) {
    MGF_REQUIRE(param && exp_avg && exp_avg_sq && adam_t && grad && lr_table && step, MGF_EINVAL, "adam_elementwise: null pointer");
    MGF_REQUIRE(numel >= 1 && steps_total >= 1, MGF_EINVAL, "adam_elementwise: bad sizes");
    launch_adam_sets(param, exp_avg, exp_avg_sq, adam_t, grad, lr_table, step, 0, valid, 0, numel, 1, numel, steps_total, beta1, beta2, eps,
                     weight_decay, (hipStream_t)stream);
    MGF_CHECK_LAUNCH("adam_elementwise");
    return MGF_OK;
}

extern "C" int mgf_adam_sets_f32(float* param, float* exp_avg, float* exp_avg_sq, int32_t* adam_t, const float* grad, const float* lr_table,
                                 const int32_t* step, int64_t step_stride, const int32_t* valid, int64_t valid_stride, int64_t numel, int32_t n_sets,
                                 int64_t set_stride, int32_t steps_total, float beta1, float beta2, float eps, float weight_decay,
                                 mgf_stream_t stream) {
    MGF_REQUIRE(param && exp_avg && exp_avg_sq && adam_t && grad && lr_table && step, MGF_EINVAL, "adam_sets: null pointer");
    MGF_REQUIRE(numel >= 1 && steps_total >= 1, MGF_EINVAL, "adam_sets: bad sizes");
    MGF_REQUIRE(n_sets >= 1 && n_sets <= 65535, MGF_EINVAL, "adam_sets: n_sets must lie in 1..65535 (got %d)", n_sets);
    MGF_REQUIRE(set_stride >= numel, MGF_EINVAL, "adam_sets: set_stride %lld is smaller than a slice (%lld)", (long long)set_stride, (long long)numel);
    MGF_REQUIRE(step_stride >= 0 && valid_stride >= 0, MGF_EINVAL, "adam_sets: negative stride");
    launch_adam_sets(param, exp_avg, exp_avg_sq, adam_t, grad, lr_table, step, step_stride, valid, valid_stride, numel, n_sets, set_stride,
                     steps_total, beta1, beta2, eps, weight_decay, (hipStream_t)stream);
    MGF_CHECK_LAUNCH("adam_sets");
    return MGF_OK;
}
