// The recombination step of the evolution-strategy projection loop (evolution.py): after a generation of the literal loop is scored, the mean
// moves to a weighted average of its best mu candidates.
//   mgf_es_recombine_f32   mean[i] = f32( f64(mean[i]) + mean_lr * (S[i] - f64(mean[i])) ),  S[i] = sum_{r<m} (weights[r] / wsum) * f64(cand[j_r, i])
// j_0, j_1, ... are the generation's valid candidates (finite total) by total ascending, ties to the smaller index; m = min(mu, valid ones).
// Every workgroup ranks the generation for itself in LDS (each lane counts the candidates that beat its own: at most ES_MAX_BATCH^2 / 256
// comparisons per lane, nothing to exchange between workgroups), then takes its share of a grid-stride pass over numel.  float64 throughout,
// r order, no atomics and no contraction: every product, quotient and sum is spelled with a rounding intrinsic, so the result equals the stated
// expression bit for bit.  Everything is read from device memory: no host synchronisation, capturable.
#include "mgf_common.h"

#include <math.h>

namespace {

constexpr int ES_MAX_BATCH = 1024;      // candidates per generation (include/mgf.h states it): 8 KB of totals + 8 KB of weights + 4 KB of indices in LDS
constexpr int ES_THREADS = 256;

__global__ __launch_bounds__(ES_THREADS) void es_recombine_kernel(float* __restrict__ mean, const float* __restrict__ cand,
                                                                  const double* __restrict__ totals, const int32_t* __restrict__ step0,
                                                                  const double* __restrict__ weights, int mu, int batch, int steps_total,
                                                                  int64_t numel, double mean_lr, int32_t* __restrict__ used) {
    __shared__ double tot[ES_MAX_BATCH];        // the generation's totals
    __shared__ double wn[ES_MAX_BATCH];         // weights[r] / wsum, r < m
    __shared__ int elite[ES_MAX_BATCH];         // elite[r] = j_r
    __shared__ int n_valid;
    const int s0 = *step0;
    if (s0 < 0 || s0 >= steps_total) return;    // (uniform over the grid: nothing is written)
    const int n = min(batch, steps_total - s0);
    for (int j = threadIdx.x; j < n; j += ES_THREADS) tot[j] = totals[s0 + j];
    __syncthreads();
    // rank: the number of valid candidates in front of candidate j in (total, index) order.  Unique, so elite[] has one writer per entry
    for (int j = threadIdx.x; j < n; j += ES_THREADS) {
        const double tj = tot[j];
        const bool ok = isfinite(tj);
        int rank = 0, v = 0;
        for (int i = 0; i < n; ++i) {
            const double ti = tot[i];
            const bool oki = isfinite(ti);
            v += oki;
            rank += oki && (ti < tj || (ti == tj && i < j));
        }
        if (ok && rank < mu) elite[rank] = j;
        if (j == 0) n_valid = v;
    }
    __syncthreads();
    const int m = min(mu, n_valid);
    if (blockIdx.x == 0 && threadIdx.x == 0 && used) used[s0 / batch] = m;
    if (m == 0) return;                         // (uniform over the grid: the mean stays)
    double wsum = weights[0];                   // every lane the same m - 1 additions in r order: cheaper than a round through LDS and a barrier
    for (int r = 1; r < m; ++r) wsum = __dadd_rn(wsum, weights[r]);
    for (int r = threadIdx.x; r < m; r += ES_THREADS) wn[r] = __ddiv_rn(weights[r], wsum);
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * ES_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * ES_THREADS + threadIdx.x; i < numel; i += stride) {
        double S = __dmul_rn(wn[0], (double)cand[(int64_t)elite[0] * numel + i]);
        for (int r = 1; r < m; ++r) S = __dadd_rn(S, __dmul_rn(wn[r], (double)cand[(int64_t)elite[r] * numel + i]));
        const double x = (double)mean[i];
        mean[i] = (float)__dadd_rn(x, __dmul_rn(mean_lr, __dsub_rn(S, x)));
    }
}

// [a, a + na) and [b, b + nb) bytes share an address
inline bool es_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

}  // namespace

extern "C" int mgf_es_recombine_f32(float* mean, const float* cand, const double* totals, const int32_t* step0, const double* weights,
                                    int32_t mu, int32_t batch, int32_t steps_total, int64_t numel, double mean_lr, int32_t* used,
                                    mgf_stream_t stream) {
    MGF_REQUIRE(mean && cand && totals && step0 && weights, MGF_EINVAL,
                "es_recombine: mean, cand, totals, step0 and weights must not be NULL");
    MGF_REQUIRE(batch >= 1 && batch <= ES_MAX_BATCH, MGF_EINVAL, "es_recombine: batch must lie in 1..%d (got %d)", ES_MAX_BATCH, batch);
    MGF_REQUIRE(mu >= 1 && mu <= batch, MGF_EINVAL, "es_recombine: mu must lie in 1..batch (got %d, batch %d)", mu, batch);
    MGF_REQUIRE(numel >= 1 && steps_total >= 1, MGF_EINVAL, "es_recombine: numel and steps_total must be >= 1 (got %lld, %d)",
                (long long)numel, steps_total);
    MGF_REQUIRE(!es_overlap(mean, numel * 4, cand, (int64_t)batch * numel * 4), MGF_EINVAL,
                "es_recombine: mean must not overlap cand (every element of the mean reads the elite candidates)");
    const int64_t g = mgf_cdiv(numel, ES_THREADS);
    hipLaunchKernelGGL(es_recombine_kernel, dim3((int)(g > 64 ? 64 : g)), dim3(ES_THREADS), 0, (hipStream_t)stream, mean, cand, totals, step0,
                       weights, (int)mu, (int)batch, (int)steps_total, numel, mean_lr, used);
    MGF_CHECK_LAUNCH("es_recombine");
    return MGF_OK;
}
