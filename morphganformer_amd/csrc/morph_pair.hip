// Two-identity term of morph refinement (gradient mode): the part of the pair objective that does NOT collapse to a single blended target.
//   mgf_embed_pair_loss_f32   loss[i] (+)= gamma ((1 - a_i) d_a + a_i d_b) + delta |d_a - d_b|,  d_t = d(emb[i], t_t)
//                             demb[i]   = d(that value) / d emb[i]           (optional)
//                             trace[i][row][0..1] = (d_a, d_b) as float64    (optional; row = the device step counter)
// metric 0: d = mean_c (e - t)^2;  metric 1: d = 1 - <e, t> / (max(|e|, 1e-8) max(|t|, 1e-8)) (torch.nn.functional.cosine_similarity).
// One workgroup per sample: float32 loads, float64 arithmetic, fixed summation order (a thread's elements in index order, wave butterflies, the
// four waves in index order), no atomics -- the style of mgf_wing_loss_f64 / mgf_dssim_grad_f32.  Any width >= 1: a thread strides over the row,
// so widths past 256 take further passes of the same loop.
#include "mgf_common.h"

#include <math.h>

namespace {

constexpr double PAIR_COS_EPS = 1e-8;

__global__ __launch_bounds__(256) void embed_pair_loss_kernel(float* __restrict__ loss, float* __restrict__ demb, double* __restrict__ trace,
                                                              const float* __restrict__ emb, const float* __restrict__ ta,
                                                              const float* __restrict__ tb, const float* __restrict__ alpha, int width,
                                                              int64_t t_stride, double gamma, double delta, int metric, int accumulate,
                                                              const int32_t* __restrict__ step, int trace_rows) {
    __shared__ double sh[4];
    const int s = blockIdx.x;
    const float* e = emb + (int64_t)s * width;
    const float* a = ta + (int64_t)s * t_stride;
    const float* b = tb + (int64_t)s * t_stride;
    // metric 0: v0 = sum (e - a)^2, v1 = sum (e - b)^2.   metric 1: v0 = <e,a>, v1 = <e,b>, v2 = <e,e>, v3 = <a,a>, v4 = <b,b>
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0;
    for (int i = threadIdx.x; i < width; i += 256) {
        const double x = (double)e[i], p = (double)a[i], q = (double)b[i];
        if (metric == 0) {
            const double da = x - p, db = x - q;
            v0 += da * da;
            v1 += db * db;
        } else {
            v0 += x * p;
            v1 += x * q;
            v2 += x * x;
            v3 += p * p;
            v4 += q * q;
        }
    }
    v0 = mgf_block_sum_256(v0, sh);
    v1 = mgf_block_sum_256(v1, sh);
    double d_a, d_b;
    // d(d_t)/d e[i] = ce_t * e[i] + ct_t * t[i] + c0_t * (e[i] - t[i])
    double ce_a = 0.0, ct_a = 0.0, ce_b = 0.0, ct_b = 0.0, c0 = 0.0;
    if (metric == 0) {
        d_a = v0 / (double)width;
        d_b = v1 / (double)width;
        c0 = 2.0 / (double)width;
    } else {
        v2 = mgf_block_sum_256(v2, sh);
        v3 = mgf_block_sum_256(v3, sh);
        v4 = mgf_block_sum_256(v4, sh);
        const double re = sqrt(v2);
        const double ne = fmax(re, PAIR_COS_EPS), na = fmax(sqrt(v3), PAIR_COS_EPS), nb = fmax(sqrt(v4), PAIR_COS_EPS);
        d_a = 1.0 - v0 / (ne * na);
        d_b = 1.0 - v1 / (ne * nb);
        // the clamp passes a gradient to |e| only where it is not active; d|e|/de at e = 0 is 0 (torch's subgradient)
        const double dn = (re >= PAIR_COS_EPS && re > 0.0) ? 1.0 / re : 0.0;
        ct_a = -1.0 / (ne * na);
        ct_b = -1.0 / (ne * nb);
        ce_a = v0 / (ne * ne * na) * dn;
        ce_b = v1 / (ne * ne * nb) * dn;
    }
    const double al = (double)alpha[s];
    const double diff = d_a - d_b;
    const double sg = diff > 0.0 ? 1.0 : (diff < 0.0 ? -1.0 : 0.0);          // d|x|/dx at 0 is 0, as in torch
    const double wa = gamma * (1.0 - al) + delta * sg, wb = gamma * al - delta * sg;
    if (threadIdx.x == 0) {
        const double val = gamma * ((1.0 - al) * d_a + al * d_b) + delta * fabs(diff);
        loss[s] = (accumulate ? loss[s] : 0.f) + (float)val;
        if (trace) {
            int row = *step;
            row = row < 0 ? 0 : (row > trace_rows - 1 ? trace_rows - 1 : row);
            double* tr = trace + ((int64_t)s * trace_rows + row) * 2;
            tr[0] = d_a;
            tr[1] = d_b;
        }
    }
    if (demb) {
        float* g = demb + (int64_t)s * width;
        for (int i = threadIdx.x; i < width; i += 256) {
            const double x = (double)e[i], p = (double)a[i], q = (double)b[i];
            const double ga = ce_a * x + ct_a * p + c0 * (x - p);
            const double gb = ce_b * x + ct_b * q + c0 * (x - q);
            g[i] = (float)(wa * ga + wb * gb);
        }
    }
}

}  // namespace

extern "C" int mgf_embed_pair_loss_f32(float* loss, float* demb, double* trace, const float* emb, const float* ta, const float* tb,
                                       const float* alpha, int32_t n, int32_t width, int64_t t_batch_stride, float gamma, float delta,
                                       int32_t metric, int32_t accumulate, const int32_t* step, int32_t trace_rows, mgf_stream_t stream) {
    MGF_REQUIRE(loss && emb && ta && tb && alpha, MGF_EINVAL, "embed_pair_loss: loss, emb, ta, tb and alpha must not be NULL");
    MGF_REQUIRE(n >= 1 && width >= 1, MGF_EINVAL, "embed_pair_loss: n and width must be >= 1 (got %d, %d)", n, width);
    MGF_REQUIRE(metric == 0 || metric == 1, MGF_EINVAL, "embed_pair_loss: metric must be 0 (mse) or 1 (cosine), got %d", metric);
    MGF_REQUIRE(t_batch_stride == 0 || t_batch_stride >= width, MGF_EINVAL,
                "embed_pair_loss: the targets' batch stride must be 0 (shared) or >= width (got %lld for width %d)", (long long)t_batch_stride, width);
    MGF_REQUIRE(!trace || (step && trace_rows >= 1), MGF_EINVAL, "embed_pair_loss: a trace needs the step counter and trace_rows >= 1");
    MGF_REQUIRE(demb != emb && (const float*)demb != ta && (const float*)demb != tb, MGF_EINVAL,
                "embed_pair_loss: demb must not alias emb, ta or tb (the gradient pass reads them again)");
    hipLaunchKernelGGL(embed_pair_loss_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, loss, demb, trace, emb, ta, tb, alpha, (int)width,
                       (int64_t)t_batch_stride, (double)gamma, (double)delta, (int)metric, (int)accumulate, step, (int)trace_rows);
    MGF_CHECK_LAUNCH("embed_pair_loss");
    return MGF_OK;
}
