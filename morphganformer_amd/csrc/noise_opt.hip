// Noise-map optimisation of gradient mode: the per-layer noise inputs as parameters next to the latent.
//   mgf_noise_grad_f32             dnoise[p] (+)= strength * sum_c dpre[c, p]                (the layer's pre-activation gradient, channel sum)
//   mgf_noise_regularize(_grad)_f32  noise_regularize of the drivers (1024_example_wing_loss_perceptual_sqz_MSE.py:32-52) and its gradient
//   mgf_noise_normalize_f32        noise_normalize_ (:55-60): x <- (x - mean) / std, std unbiased
//   mgf_noise_sets_*               the same three over SETS (one target's maps each; a map table that holds for every set) in a
//                                  launch count that depends on neither the number of sets nor of maps; the per-element bodies are shared
// (The maps' Adam step, mgf_adam_elementwise_f32 / mgf_adam_sets_f32, lives with the latent's in adam.hip.)
// float32 in and out, float64 accumulation, fixed summation order (block partials in caller scratch, folded by a fixed tree), no atomics.
#include "mgf_common.h"

#include <math.h>

namespace {

constexpr int NO_PARTS = 256;          // at most this many block partials per reduction (one per thread of the block that folds them)

// ---------------------------------------------------------------------------------------------- d noise
// block = PQ pixel groups x S channel slices (PQ * S = 256); a thread sums its slice's channels in index order for V consecutive pixels,
// the slices are then added in index order.  S > 1 only where the map is too small to fill the chip with one thread per pixel group.
template <int V, int S>
__device__ __forceinline__ void noise_grad_body(float* __restrict__ dnoise, const float* __restrict__ dpre, const float* __restrict__ strength,
                                                int c, int64_t hw, int accumulate) {
    constexpr int PQ = 256 / S;
    __shared__ double part[S > 1 ? S : 1][PQ][V];
    const int pq = threadIdx.x % PQ, sl = threadIdx.x / PQ;
    const int64_t groups = hw / V;
    const int64_t q = (int64_t)blockIdx.x * PQ + pq;
    const bool live = q < groups;
    const int per = (c + S - 1) / S;
    const int c0 = sl * per, c1 = min(c, c0 + per);
    double acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.0;
    if (live) {
        const float* src = dpre + q * V;
        int ch = c0;
        if (V == 4) {
            for (; ch + 4 <= c1; ch += 4) {                                   // four loads in flight, added in channel order
                float4 t[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) t[u] = *reinterpret_cast<const float4*>(src + (int64_t)(ch + u) * hw);
#pragma unroll
                for (int u = 0; u < 4; ++u) { acc[0] += (double)t[u].x; acc[1 % V] += (double)t[u].y; acc[2 % V] += (double)t[u].z; acc[3 % V] += (double)t[u].w; }
            }
            for (; ch < c1; ++ch) {
                const float4 t = *reinterpret_cast<const float4*>(src + (int64_t)ch * hw);
                acc[0] += (double)t.x; acc[1 % V] += (double)t.y; acc[2 % V] += (double)t.z; acc[3 % V] += (double)t.w;
            }
        } else {
            for (; ch < c1; ++ch) acc[0] += (double)src[(int64_t)ch * hw];
        }
    }
    if (S > 1) {
#pragma unroll
        for (int j = 0; j < V; ++j) part[sl][pq][j] = acc[j];
        __syncthreads();
        if (sl != 0) return;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            double s = part[0][pq][j];
            for (int k = 1; k < S; ++k) s += part[k][pq][j];
            acc[j] = s;
        }
    }
    if (!live) return;
    const double k = (double)strength[0];
    float* dst = dnoise + q * V;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float g = (float)(k * acc[j]);
        dst[j] = accumulate ? dst[j] + g : g;
    }
}

// Sample blockIdx.y of dpre [n, c, hw], into that sample's own map (one map: n = 1).
template <int V, int S>
__global__ __launch_bounds__(256) void noise_sets_grad_kernel(float* __restrict__ dnoise, int64_t dnoise_stride, const float* __restrict__ dpre,
                                                              const float* __restrict__ strength, int c, int64_t hw, int accumulate) {
    noise_grad_body<V, S>(dnoise + (int64_t)blockIdx.y * dnoise_stride, dpre + (int64_t)blockIdx.y * c * hw, strength, c, hw, accumulate);
}

template <int V, int S>
void launch_noise_grad(float* dnoise, const float* dpre, const float* strength, int c, int64_t hw, int accumulate, hipStream_t st, int n,
                       int64_t dnoise_stride) {
    const int64_t groups = hw / V;
    const int grid = (int)mgf_cdiv(groups, 256 / S);
    hipLaunchKernelGGL((noise_sets_grad_kernel<V, S>), dim3(grid, n), dim3(256), 0, st, dnoise, dnoise_stride, dpre, strength, c, hw, accumulate);
}

// The slice form for n samples of a layer of c channels and hw pixels (vec: float4 loads are possible).
void choose_noise_grad(bool vec, float* dnoise, const float* dpre, const float* strength, int c, int64_t hw, int accumulate, hipStream_t st,
                       int n, int64_t dnoise_stride) {
    if (vec) {
        const int64_t groups = hw / 4;
        if (groups >= 65536 || c < 16) launch_noise_grad<4, 1>(dnoise, dpre, strength, c, hw, accumulate, st, n, dnoise_stride);
        else if (groups >= 16384 || c < 64) launch_noise_grad<4, 4>(dnoise, dpre, strength, c, hw, accumulate, st, n, dnoise_stride);
        else launch_noise_grad<4, 16>(dnoise, dpre, strength, c, hw, accumulate, st, n, dnoise_stride);
    } else {
        if (c < 64) launch_noise_grad<1, 1>(dnoise, dpre, strength, c, hw, accumulate, st, n, dnoise_stride);
        else launch_noise_grad<1, 16>(dnoise, dpre, strength, c, hw, accumulate, st, n, dnoise_stride);
    }
}

// ---------------------------------------------------------------------------------------------- regulariser
// One level of the pyramid, side s: block partials of  a = sum x[y,x] x[y,x-1]  and  b = sum x[y,x] x[y-1,x]  (indices modulo s: the rolls
// wrap), one thread per 2 x 2 block, and -- when `next` is given -- the block means, the next level's map.
template <typename T>
__device__ __forceinline__ void reg_level_fwd_body(double* __restrict__ partials, double* __restrict__ next, const T* __restrict__ x, int s, double* sh) {
    const int half = s >> 1;
    const int64_t blocks = (int64_t)half * half;
    double a = 0.0, b = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < blocks; i += (int64_t)gridDim.x * 256) {
        const int by = (int)(i / half), bx = (int)(i % half);
        const int y0 = 2 * by, x0 = 2 * bx;
        const int ym = (y0 + s - 1) % s, xm = (x0 + s - 1) % s;
        const T* r0 = x + (int64_t)y0 * s;
        const T* r1 = r0 + s;
        const T* ru = x + (int64_t)ym * s;
        const double v00 = (double)r0[x0], v01 = (double)r0[x0 + 1], v10 = (double)r1[x0], v11 = (double)r1[x0 + 1];
        const double l0 = (double)r0[xm], l1 = (double)r1[xm], u0 = (double)ru[x0], u1 = (double)ru[x0 + 1];
        a += v00 * l0 + v01 * v00 + v10 * l1 + v11 * v10;
        b += v00 * u0 + v01 * u1 + v10 * v00 + v11 * v01;
        if (next) next[i] = (v00 + v01 + v10 + v11) * 0.25;
    }
    a = mgf_block_sum_256(a, sh);
    b = mgf_block_sum_256(b, sh);
    if (threadIdx.x == 0) { partials[2 * blockIdx.x] = a; partials[2 * blockIdx.x + 1] = b; }
}

template <typename T>
__global__ __launch_bounds__(256) void reg_level_fwd_kernel(double* __restrict__ partials, double* __restrict__ next, const T* __restrict__ x, int s) {
    __shared__ double sh[4];
    reg_level_fwd_body<T>(partials, next, x, s, sh);
}

struct RegLevels {
    int32_t levels;
    int32_t side[16];
    int32_t nparts[16];
};

// One workgroup: fold every level's partials, stats[l] = {mean of the column product, mean of the row product}, and
// value (+)= scale * sum_l (A_l^2 + B_l^2) when `value` is given.
// Level l of one map: fold its `nparts` partials, stats[l] = {A, B}; returns A^2 + B^2 (every thread).
__device__ __forceinline__ double reg_finish_level(double* __restrict__ stats, const double* __restrict__ partials, int l, int nparts, int side,
                                                   double* sh) {
    const double* p = partials + (int64_t)l * NO_PARTS * 2;
    const bool in = (int)threadIdx.x < nparts;
    const double a = mgf_block_sum_256(in ? p[2 * threadIdx.x] : 0.0, sh);
    const double b = mgf_block_sum_256(in ? p[2 * threadIdx.x + 1] : 0.0, sh);
    const double n = (double)side * (double)side;
    const double A = a / n, B = b / n;
    if (threadIdx.x == 0) { stats[2 * l] = A; stats[2 * l + 1] = B; }
    return A * A + B * B;
}

__global__ __launch_bounds__(256) void reg_finish_kernel(double* __restrict__ stats, float* value, const double* __restrict__ partials, RegLevels lv,
                                                         double scale, int accumulate) {
    __shared__ double sh[4];
    double reg = 0.0;
    for (int l = 0; l < lv.levels; ++l) reg += reg_finish_level(stats, partials, l, lv.nparts[l], lv.side[l], sh);
    if (value && threadIdx.x == 0) {
        const float v = (float)(scale * reg);
        *value = accumulate ? *value + v : v;
    }
}

// Gradient of one level, one thread per element:  g = 2A/N (left + right) + 2B/N (upper + lower) + 1/4 g_parent[y/2, x/2]  (the block
// mean's adjoint); inner levels keep g in float64 scratch, the finest level writes dx (+)= scale * g.
template <typename T>
__device__ __forceinline__ void reg_level_bwd_body(double* __restrict__ gcur, float* __restrict__ dx, const T* __restrict__ x,
                                                   const double* __restrict__ gparent, const double* __restrict__ stats, int s,
                                                   double scale, int accumulate) {
    const double n = (double)s * (double)s;
    const double ka = 2.0 * stats[0] / n, kb = 2.0 * stats[1] / n;
    const int64_t total = (int64_t)s * s;
    const int half = s >> 1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / s), xx = (int)(i % s);
        const int ym = (y + s - 1) % s, yp = (y + 1) % s, xm = (xx + s - 1) % s, xp = (xx + 1) % s;
        double g = ka * ((double)x[(int64_t)y * s + xm] + (double)x[(int64_t)y * s + xp])
                 + kb * ((double)x[(int64_t)ym * s + xx] + (double)x[(int64_t)yp * s + xx]);
        if (gparent) g += 0.25 * gparent[(int64_t)(y >> 1) * half + (xx >> 1)];
        if (dx) {
            const float v = (float)(scale * g);
            dx[i] = accumulate ? dx[i] + v : v;
        } else {
            gcur[i] = g;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void reg_level_bwd_kernel(double* __restrict__ gcur, float* __restrict__ dx, const T* __restrict__ x,
                                                            const double* __restrict__ gparent, const double* __restrict__ stats, int s,
                                                            double scale, int accumulate) {
    reg_level_bwd_body<T>(gcur, dx, x, gparent, stats, s, scale, accumulate);
}

int reg_levels(int32_t side, RegLevels* lv) {
    if (side < 2 || side > 32768 || (side & (side - 1))) return 0;
    int l = 0;
    for (int32_t s = side;; s >>= 1) {
        lv->side[l] = s;
        const int64_t blocks = (int64_t)(s / 2) * (s / 2);
        int64_t g = mgf_cdiv(blocks, 256);
        lv->nparts[l] = (int)(g > NO_PARTS ? NO_PARTS : g);
        ++l;
        if (s <= 8) break;
    }
    lv->levels = l;
    return l;
}

// scratch, in doubles: partials [levels][NO_PARTS][2] | stats [levels][2] | the maps of levels 1.. | the gradients of levels 1..
int64_t reg_pyramid_doubles(const RegLevels& lv) {
    int64_t t = 0;
    for (int l = 1; l < lv.levels; ++l) t += (int64_t)lv.side[l] * lv.side[l];
    return t;
}

int reg_forward(const float* x, const RegLevels& lv, double* scratch, hipStream_t st) {
    double* partials = scratch;
    double* xp = scratch + (int64_t)lv.levels * NO_PARTS * 2 + (int64_t)lv.levels * 2;
    const double* cur = nullptr;
    for (int l = 0; l < lv.levels; ++l) {
        double* next = l + 1 < lv.levels ? xp : nullptr;
        double* pl = partials + (int64_t)l * NO_PARTS * 2;
        if (l == 0)
            hipLaunchKernelGGL(reg_level_fwd_kernel<float>, dim3(lv.nparts[l]), dim3(256), 0, st, pl, next, x, lv.side[l]);
        else
            hipLaunchKernelGGL(reg_level_fwd_kernel<double>, dim3(lv.nparts[l]), dim3(256), 0, st, pl, next, cur, lv.side[l]);
        cur = xp;
        if (next) xp += (int64_t)lv.side[l + 1] * lv.side[l + 1];
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- normalise
__device__ __forceinline__ bool step_is_live(const int32_t* step, const int32_t* valid, int steps_total) {
    if (!step) return true;
    const int s = *step;
    return s < steps_total && !(valid && valid[s] == 0);
}

// Block bx of gx: its partial sums of x and x^2 (the partial count and a thread's summation order depend on gx).
__device__ __forceinline__ void norm_partial_body(double* __restrict__ partials, const float* __restrict__ x, int64_t numel, int bx, int gx, double* sh) {
    double s = 0.0, q = 0.0;
    for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < numel; i += (int64_t)gx * 256) {
        const double v = (double)x[i];
        s += v;
        q += v * v;
    }
    s = mgf_block_sum_256(s, sh);
    q = mgf_block_sum_256(q, sh);
    if (threadIdx.x == 0) { partials[2 * bx] = s; partials[2 * bx + 1] = q; }
}

// Block bx of gx: fold the partials and normalise its share of the elements (elementwise: gx changes no bit).
__device__ __forceinline__ void norm_apply_body(float* __restrict__ x, const double* __restrict__ partials, int nparts, int64_t numel, int bx, int gx,
                                                double* sh) {
    const bool in = (int)threadIdx.x < nparts;
    const double s = mgf_block_sum_256(in ? partials[2 * threadIdx.x] : 0.0, sh);
    const double q = mgf_block_sum_256(in ? partials[2 * threadIdx.x + 1] : 0.0, sh);
    const double n = (double)numel;
    const double mean = s / n;
    const double var = (q - s * mean) / (n - 1.0);                            // unbiased, torch's default
    const double inv = 1.0 / sqrt(var);
    for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < numel; i += (int64_t)gx * 256)
        x[i] = (float)(((double)x[i] - mean) * inv);
}

__global__ __launch_bounds__(256) void norm_partial_kernel(double* __restrict__ partials, const float* __restrict__ x, int64_t numel) {
    __shared__ double sh[4];
    norm_partial_body(partials, x, numel, blockIdx.x, gridDim.x, sh);
}

__global__ __launch_bounds__(256) void norm_apply_kernel(float* __restrict__ x, const double* __restrict__ partials, int nparts, int64_t numel,
                                                         const int32_t* step, const int32_t* valid, int steps_total) {
    __shared__ double sh[4];
    if (!step_is_live(step, valid, steps_total)) return;                     // (uniform over the grid)
    norm_apply_body(x, partials, nparts, numel, blockIdx.x, gridDim.x, sh);
}

// ---------------------------------------------------------------------------------------------- sets
// A set is one target's maps: map m has side tab.side[m] and starts tab.off[m] floats into the set, set t starts t * set_stride floats after
// set 0.  The table travels by value in the kernel arguments (nothing is copied to the device).  A JOB is one (set, map); its scratch has
// the per-map entry's layout (partials | stats | map pyramid | gradient pyramid) and starts tab.sc[m] doubles into the set's scratch.
constexpr int SETS_MAX_MAPS = 32;

struct SetTable {
    int32_t n_maps;
    int32_t side[SETS_MAX_MAPS];
    int64_t off[SETS_MAX_MAPS];
    int64_t sc[SETS_MAX_MAPS];
};

// The maps that have a pyramid level of the launch's side.
struct LevelJobs {
    int32_t n;
    uint8_t map[SETS_MAX_MAPS];
};

__host__ __device__ __forceinline__ int map_levels(int side) {
    int l = 1;
    for (int s = side; s > 8; s >>= 1) ++l;
    return l;
}

// Offset of level l >= 1 inside a map's pyramid (levels 1.. back to back).
__host__ __device__ __forceinline__ int64_t pyramid_offset(int side, int l) {
    int64_t o = 0;
    for (int k = 1; k < l; ++k) o += (int64_t)(side >> k) * (side >> k);
    return o;
}

__host__ __device__ __forceinline__ int level_parts(int s) {
    const int64_t g = ((int64_t)(s / 2) * (s / 2) + 255) / 256;
    return (int)(g > NO_PARTS ? NO_PARTS : g);
}

struct JobScratch {
    double* partials;
    double* stats;
    double* xpyr;
    double* gpyr;
};

__device__ __forceinline__ JobScratch job_scratch(double* sc, int side) {
    const int levels = map_levels(side);
    JobScratch j;
    j.partials = sc;
    j.stats = sc + (int64_t)levels * NO_PARTS * 2;
    j.xpyr = j.stats + (int64_t)levels * 2;
    j.gpyr = j.xpyr + pyramid_offset(side, levels);
    return j;
}

// grid (partials of side s, sets x jobs.n): level `s` of every job that has one, each with the per-map kernel's grid.
__global__ __launch_bounds__(256) void reg_sets_fwd_kernel(double* __restrict__ scratch, const float* __restrict__ x, SetTable tab, LevelJobs jobs,
                                                           int64_t set_stride, int64_t set_doubles, int s) {
    __shared__ double sh[4];
    const int t = blockIdx.y / jobs.n, m = jobs.map[blockIdx.y % jobs.n];
    const int side = tab.side[m], levels = map_levels(side);
    int l = 0;
    for (int q = side; q > s; q >>= 1) ++l;
    const JobScratch js = job_scratch(scratch + (int64_t)t * set_doubles + tab.sc[m], side);
    double* partials = js.partials + (int64_t)l * NO_PARTS * 2;
    double* next = l + 1 < levels ? js.xpyr + pyramid_offset(side, l + 1) : nullptr;
    if (l == 0)
        reg_level_fwd_body<float>(partials, next, x + (int64_t)t * set_stride + tab.off[m], s, sh);
    else
        reg_level_fwd_body<double>(partials, next, js.xpyr + pyramid_offset(side, l), s, sh);
}

// One workgroup per job: its levels' statistics, and f32(scale * reg) of the map into the set's value row (vals[m], behind the jobs' scratch).
__global__ __launch_bounds__(256) void reg_sets_finish_kernel(double* __restrict__ scratch, SetTable tab, int64_t set_doubles, int64_t vals_off,
                                                              double scale) {
    __shared__ double sh[4];
    const int t = blockIdx.x / tab.n_maps, m = blockIdx.x % tab.n_maps;
    const int side = tab.side[m], levels = map_levels(side);
    double* set_sc = scratch + (int64_t)t * set_doubles;
    const JobScratch js = job_scratch(set_sc + tab.sc[m], side);
    double reg = 0.0;
    for (int l = 0; l < levels; ++l) reg += reg_finish_level(js.stats, js.partials, l, level_parts(side >> l), side >> l, sh);
    if (threadIdx.x == 0) set_sc[vals_off + m] = (double)(float)(scale * reg);
}

// grid (blocks of side s, sets x jobs.n): the gradient of level `s` of every job that has one.  With fold_value (the first of the backward
// launches) one thread per set also adds the set's value row to value[t * value_stride], in float32 in table order.
__global__ __launch_bounds__(256) void reg_sets_bwd_kernel(float* __restrict__ dx, float* value, int64_t value_stride, double* __restrict__ scratch,
                                                           const float* __restrict__ x, SetTable tab, LevelJobs jobs, int64_t set_stride,
                                                           int64_t set_doubles, int64_t vals_off, int s, double scale, int accumulate_dx,
                                                           int accumulate_value, int fold_value) {
    const int t = blockIdx.y / jobs.n, k = blockIdx.y % jobs.n, m = jobs.map[k];
    const int side = tab.side[m], levels = map_levels(side);
    double* set_sc = scratch + (int64_t)t * set_doubles;
    if (fold_value && value && k == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
        float* dst = value + (int64_t)t * value_stride;
        float acc = accumulate_value ? *dst : 0.f;
        for (int i = 0; i < tab.n_maps; ++i) {
            const float v = (float)set_sc[vals_off + i];
            acc = (accumulate_value || i > 0) ? acc + v : v;
        }
        *dst = acc;
    }
    int l = 0;
    for (int q = side; q > s; q >>= 1) ++l;
    const JobScratch js = job_scratch(set_sc + tab.sc[m], side);
    const double* gparent = l + 1 < levels ? js.gpyr + pyramid_offset(side, l + 1) : nullptr;
    const int64_t o = (int64_t)t * set_stride + tab.off[m];
    if (l == 0)
        reg_level_bwd_body<float>((double*)nullptr, dx + o, x + o, gparent, js.stats, s, scale, accumulate_dx);
    else
        reg_level_bwd_body<double>(js.gpyr + pyramid_offset(side, l), (float*)nullptr, (const double*)(js.xpyr + pyramid_offset(side, l)), gparent,
                                   js.stats + 2 * l, s, 1.0, 0);
}

__host__ __device__ __forceinline__ int norm_parts(int side) {
    const int64_t g = ((int64_t)side * side + 1023) / 1024;
    return (int)(g > NO_PARTS ? NO_PARTS : g);
}

// Block b of a set's row of blocks -> (map, block inside the map's norm_parts blocks).
__device__ __forceinline__ int norm_job(const SetTable& tab, int b, int* bx) {
    int m = 0;
    for (; m + 1 < tab.n_maps; ++m) {
        const int np = norm_parts(tab.side[m]);
        if (b < np) break;
        b -= np;
    }
    *bx = b;
    return m;
}

// grid (sum of the maps' partial counts, sets); partials of job (t, m) at scratch[(t * n_maps + m) * NO_PARTS * 2].
__global__ __launch_bounds__(256) void norm_sets_partial_kernel(double* __restrict__ scratch, const float* __restrict__ x, SetTable tab, int64_t set_stride) {
    __shared__ double sh[4];
    int bx;
    const int t = blockIdx.y, m = norm_job(tab, blockIdx.x, &bx);
    const int side = tab.side[m];
    norm_partial_body(scratch + ((int64_t)t * tab.n_maps + m) * NO_PARTS * 2, x + (int64_t)t * set_stride + tab.off[m], (int64_t)side * side, bx,
                      norm_parts(side), sh);
}

__global__ __launch_bounds__(256) void norm_sets_apply_kernel(float* __restrict__ x, const double* __restrict__ scratch, SetTable tab, int64_t set_stride,
                                                              const int32_t* step, int64_t step_stride, const int32_t* valid, int64_t valid_stride,
                                                              int steps_total) {
    __shared__ double sh[4];
    const int t = blockIdx.y;
    if (!step_is_live(step ? step + t * step_stride : nullptr, valid ? valid + t * valid_stride : nullptr, steps_total)) return;   // (uniform over the block)
    int bx;
    const int m = norm_job(tab, blockIdx.x, &bx);
    const int side = tab.side[m];
    norm_apply_body(x + (int64_t)t * set_stride + tab.off[m], scratch + ((int64_t)t * tab.n_maps + m) * NO_PARTS * 2, norm_parts(side),
                    (int64_t)side * side, bx, norm_parts(side), sh);
}

// dst, map-major and dense ([map][set][side^2]: what the generator's layers read, n_sets maps each), from the sets; tab.sc[m] = the floats
// of the maps in front of m.  grid as norm_sets_partial_kernel.
__global__ __launch_bounds__(256) void sets_pack_kernel(float* __restrict__ dst, const float* __restrict__ x, SetTable tab, int64_t set_stride) {
    int bx;
    const int t = blockIdx.y, m = norm_job(tab, blockIdx.x, &bx);
    const int side = tab.side[m], gx = norm_parts(side);
    const int64_t numel = (int64_t)side * side;
    const float* src = x + (int64_t)t * set_stride + tab.off[m];
    float* out = dst + (int64_t)gridDim.y * tab.sc[m] + (int64_t)t * numel;
    for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < numel; i += (int64_t)gx * 256) out[i] = src[i];
}

// Check a map table and fill the kernels' copy.  0 with the error set, else 1.
int sets_table(const char* who, const int64_t* offsets, const int32_t* sides, int32_t n_maps, int32_t n_sets, int64_t set_stride, SetTable* tab,
               int64_t* jobs_doubles, int64_t* span = nullptr) {
#define SETS_REQUIRE(cond, ...) do { if (!(cond)) { mgf_set_error(__VA_ARGS__); return 0; } } while (0)
    SETS_REQUIRE(offsets && sides, "%s: null map table", who);
    SETS_REQUIRE(n_maps >= 1 && n_maps <= SETS_MAX_MAPS, "%s: n_maps must lie in 1..%d (got %d)", who, SETS_MAX_MAPS, n_maps);
    SETS_REQUIRE(n_sets >= 1 && (int64_t)n_sets * n_maps <= 65535, "%s: n_sets must be >= 1 and n_sets * n_maps <= 65535 (got %d sets)", who, n_sets);
    int64_t extent = 0, sc = 0;
    tab->n_maps = n_maps;
    for (int m = 0; m < n_maps; ++m) {
        RegLevels lv;
        SETS_REQUIRE(reg_levels(sides[m], &lv), "%s: map %d: the side must be a power of two in 2..32768 (got %d)", who, m, sides[m]);
        SETS_REQUIRE(offsets[m] >= 0, "%s: map %d: negative offset", who, m);
        const int64_t end = offsets[m] + (int64_t)sides[m] * sides[m];
        for (int k = 0; k < m; ++k)
            SETS_REQUIRE(end <= offsets[k] || offsets[k] + (int64_t)sides[k] * sides[k] <= offsets[m], "%s: maps %d and %d overlap", who, k, m);
        if (end > extent) extent = end;
        tab->side[m] = sides[m];
        tab->off[m] = offsets[m];
        tab->sc[m] = sc;
        sc += mgf_noise_regularize_scratch_bytes(sides[m]) / 8;
    }
    for (int m = n_maps; m < SETS_MAX_MAPS; ++m) { tab->side[m] = 0; tab->off[m] = 0; tab->sc[m] = 0; }
    SETS_REQUIRE(set_stride >= extent, "%s: set_stride %lld is smaller than the table's extent %lld", who, (long long)set_stride, (long long)extent);
#undef SETS_REQUIRE
    *jobs_doubles = sc;
    if (span) *span = (int64_t)(n_sets - 1) * set_stride + extent;          // floats from set 0's start to the end of the last set's maps
    return 1;
}

}  // namespace

extern "C" int mgf_noise_grad_f32(float* dnoise, const float* dpre, const float* strength, int32_t c, int64_t hw, int32_t accumulate,
                                  mgf_stream_t stream) {
    MGF_REQUIRE(dnoise && dpre && strength, MGF_EINVAL, "noise_grad: null pointer");
    MGF_REQUIRE(c >= 1 && hw >= 1, MGF_EINVAL, "noise_grad: bad sizes");
    MGF_REQUIRE(hw <= ((int64_t)1 << 30), MGF_ETOOBIG, "noise_grad: map too large (%lld pixels)", (long long)hw);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = hw % 4 == 0 && ((uintptr_t)dpre % 16) == 0 && ((uintptr_t)dnoise % 16) == 0;
    choose_noise_grad(vec, dnoise, dpre, strength, c, hw, accumulate, st, 1, hw);
    MGF_CHECK_LAUNCH("noise_grad");
    return MGF_OK;
}

extern "C" int64_t mgf_noise_regularize_scratch_bytes(int32_t side) {
    RegLevels lv;
    if (!reg_levels(side, &lv)) return 0;
    return 8 * ((int64_t)lv.levels * NO_PARTS * 2 + (int64_t)lv.levels * 2 + 2 * reg_pyramid_doubles(lv));
}

extern "C" int mgf_noise_regularize_f32(float* value, const float* x, int32_t side, float scale, int32_t accumulate, void* scratch,
                                        mgf_stream_t stream) {
    RegLevels lv;
    MGF_REQUIRE(value && x && scratch, MGF_EINVAL, "noise_regularize: null pointer");
    MGF_REQUIRE(reg_levels(side, &lv), MGF_EUNSUPPORTED, "noise_regularize: the side must be a power of two in 2..32768 (got %d)", side);
    MGF_REQUIRE(((uintptr_t)scratch % 8) == 0, MGF_EINVAL, "noise_regularize: scratch must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* sc = (double*)scratch;
    reg_forward(x, lv, sc, st);
    hipLaunchKernelGGL(reg_finish_kernel, dim3(1), dim3(256), 0, st, sc + (int64_t)lv.levels * NO_PARTS * 2, value, sc, lv, (double)scale, accumulate);
    MGF_CHECK_LAUNCH("noise_regularize");
    return MGF_OK;
}

extern "C" int mgf_noise_regularize_grad_f32(float* dx, float* value, const float* x, int32_t side, float scale, int32_t accumulate_dx,
                                             int32_t accumulate_value, void* scratch, mgf_stream_t stream) {
    RegLevels lv;
    MGF_REQUIRE(dx && x && scratch, MGF_EINVAL, "noise_regularize_grad: null pointer");
    MGF_REQUIRE(dx != x, MGF_EINVAL, "noise_regularize_grad: dx must not alias x");
    MGF_REQUIRE(reg_levels(side, &lv), MGF_EUNSUPPORTED, "noise_regularize_grad: the side must be a power of two in 2..32768 (got %d)", side);
    MGF_REQUIRE(((uintptr_t)scratch % 8) == 0, MGF_EINVAL, "noise_regularize_grad: scratch must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* sc = (double*)scratch;
    double* stats = sc + (int64_t)lv.levels * NO_PARTS * 2;
    double* xpyr = stats + (int64_t)lv.levels * 2;
    double* gpyr = xpyr + reg_pyramid_doubles(lv);
    reg_forward(x, lv, sc, st);
    hipLaunchKernelGGL(reg_finish_kernel, dim3(1), dim3(256), 0, st, stats, value, sc, lv, (double)scale, accumulate_value);
    // offsets of levels 1.. inside the two pyramids
    int64_t off[16] = {0};
    for (int l = 2; l < lv.levels; ++l) off[l] = off[l - 1] + (int64_t)lv.side[l - 1] * lv.side[l - 1];
    for (int l = lv.levels - 1; l >= 0; --l) {
        const int s = lv.side[l];
        const int grid = mgf_stream_grid((int64_t)s * s, 256, 4);
        const double* gparent = l + 1 < lv.levels ? gpyr + off[l + 1] : nullptr;
        if (l == 0)
            hipLaunchKernelGGL(reg_level_bwd_kernel<float>, dim3(grid), dim3(256), 0, st, (double*)nullptr, dx, x, gparent, stats, s, (double)scale,
                               accumulate_dx);
        else
            hipLaunchKernelGGL(reg_level_bwd_kernel<double>, dim3(grid), dim3(256), 0, st, gpyr + off[l], (float*)nullptr,
                               (const double*)(xpyr + off[l]), gparent, stats + 2 * l, s, 1.0, 0);
    }
    MGF_CHECK_LAUNCH("noise_regularize_grad");
    return MGF_OK;
}

extern "C" int64_t mgf_noise_normalize_scratch_bytes(void) { return 8 * NO_PARTS * 2; }

extern "C" int mgf_noise_normalize_f32(float* x, int64_t numel, const int32_t* step, const int32_t* valid, int32_t steps_total, void* scratch,
                                       mgf_stream_t stream) {
    MGF_REQUIRE(x && scratch, MGF_EINVAL, "noise_normalize: null pointer");
    MGF_REQUIRE(numel >= 2, MGF_EINVAL, "noise_normalize: the unbiased std needs at least two elements (got %lld)", (long long)numel);
    MGF_REQUIRE(step || !valid, MGF_EINVAL, "noise_normalize: a valid table needs the step counter");
    MGF_REQUIRE(!step || steps_total >= 1, MGF_EINVAL, "noise_normalize: bad steps_total");
    MGF_REQUIRE(((uintptr_t)scratch % 8) == 0, MGF_EINVAL, "noise_normalize: scratch must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int64_t g = mgf_cdiv(numel, 256 * 4);
    const int nparts = (int)(g > NO_PARTS ? NO_PARTS : g);
    hipLaunchKernelGGL(norm_partial_kernel, dim3(nparts), dim3(256), 0, st, (double*)scratch, x, numel);
    hipLaunchKernelGGL(norm_apply_kernel, dim3(mgf_stream_grid(numel, 256, 4)), dim3(256), 0, st, x, (const double*)scratch, nparts, numel, step,
                       valid, steps_total);
    MGF_CHECK_LAUNCH("noise_normalize");
    return MGF_OK;
}

// ---------------------------------------------------------------------------------------------- sets: entries
extern "C" int64_t mgf_noise_sets_scratch_bytes(const int32_t* sides, int32_t n_maps, int32_t n_sets) {
    if (!sides || n_maps < 1 || n_maps > SETS_MAX_MAPS || n_sets < 1) return 0;
    int64_t d = n_maps;                                     // the set's value row
    for (int m = 0; m < n_maps; ++m) {
        const int64_t b = mgf_noise_regularize_scratch_bytes(sides[m]);
        if (!b) return 0;
        d += b / 8;
    }
    return 8 * d * n_sets;                                  // (the normalisation's [sets][maps][NO_PARTS][2] partials fit: every job holds more)
}

extern "C" int mgf_noise_sets_regularize_grad_f32(float* dx, float* value, int64_t value_stride, const float* x, const int64_t* offsets,
                                                  const int32_t* sides, int32_t n_maps, int32_t n_sets, int64_t set_stride, float scale,
                                                  int32_t accumulate_dx, int32_t accumulate_value, void* scratch, mgf_stream_t stream) {
    SetTable tab;
    int64_t jobs_doubles = 0, span = 0;
    MGF_REQUIRE(dx && x && scratch, MGF_EINVAL, "noise_sets_regularize_grad: null pointer");
    MGF_REQUIRE(((uintptr_t)scratch % 8) == 0, MGF_EINVAL, "noise_sets_regularize_grad: scratch must be 8-byte aligned");
    if (!sets_table("noise_sets_regularize_grad", offsets, sides, n_maps, n_sets, set_stride, &tab, &jobs_doubles, &span)) return MGF_EINVAL;
    MGF_REQUIRE(dx + span <= x || x + span <= dx, MGF_EINVAL, "noise_sets_regularize_grad: dx must not alias x");
    MGF_REQUIRE(!value || n_sets == 1 || value_stride >= 1, MGF_EINVAL, "noise_sets_regularize_grad: bad value_stride");
    hipStream_t st = (hipStream_t)stream;
    double* sc = (double*)scratch;
    const int64_t set_doubles = jobs_doubles + n_maps, vals_off = jobs_doubles;
    // the distinct pyramid sides, largest first, and the maps that have each
    int32_t level_side[16];
    LevelJobs jobs[16];
    int nlev = 0;
    for (int32_t s = 32768; s >= 2; s >>= 1) {
        LevelJobs j;
        j.n = 0;
        for (int m = 0; m < n_maps; ++m)
            if (s == sides[m] || (s >= 8 && s < sides[m])) j.map[j.n++] = (uint8_t)m;
        for (int k = j.n; k < SETS_MAX_MAPS; ++k) j.map[k] = 0;
        if (j.n) { level_side[nlev] = s; jobs[nlev++] = j; }
    }
    for (int i = 0; i < nlev; ++i)
        hipLaunchKernelGGL(reg_sets_fwd_kernel, dim3(level_parts(level_side[i]), n_sets * jobs[i].n), dim3(256), 0, st, sc, x, tab, jobs[i], set_stride,
                           set_doubles, level_side[i]);
    hipLaunchKernelGGL(reg_sets_finish_kernel, dim3(n_sets * n_maps), dim3(256), 0, st, sc, tab, set_doubles, vals_off, (double)scale);
    for (int i = nlev - 1; i >= 0; --i) {
        const int s = level_side[i];
        hipLaunchKernelGGL(reg_sets_bwd_kernel, dim3(mgf_stream_grid((int64_t)s * s, 256, 4), n_sets * jobs[i].n), dim3(256), 0, st, dx, value,
                           value_stride, sc, x, tab, jobs[i], set_stride, set_doubles, vals_off, s, (double)scale, accumulate_dx, accumulate_value,
                           (int)(i == nlev - 1));
    }
    MGF_CHECK_LAUNCH("noise_sets_regularize_grad");
    return MGF_OK;
}

extern "C" int mgf_noise_sets_normalize_f32(float* x, const int64_t* offsets, const int32_t* sides, int32_t n_maps, int32_t n_sets, int64_t set_stride,
                                            const int32_t* step, int64_t step_stride, const int32_t* valid, int64_t valid_stride,
                                            int32_t steps_total, void* scratch, mgf_stream_t stream) {
    SetTable tab;
    int64_t jobs_doubles = 0;
    MGF_REQUIRE(x && scratch, MGF_EINVAL, "noise_sets_normalize: null pointer");
    MGF_REQUIRE(step || !valid, MGF_EINVAL, "noise_sets_normalize: a valid table needs the step counters");
    MGF_REQUIRE(!step || steps_total >= 1, MGF_EINVAL, "noise_sets_normalize: bad steps_total");
    MGF_REQUIRE(!step || (step_stride >= 0 && valid_stride >= 0), MGF_EINVAL, "noise_sets_normalize: negative stride");
    MGF_REQUIRE(((uintptr_t)scratch % 8) == 0, MGF_EINVAL, "noise_sets_normalize: scratch must be 8-byte aligned");
    if (!sets_table("noise_sets_normalize", offsets, sides, n_maps, n_sets, set_stride, &tab, &jobs_doubles)) return MGF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int blocks = 0;
    for (int m = 0; m < n_maps; ++m) blocks += norm_parts(sides[m]);
    hipLaunchKernelGGL(norm_sets_partial_kernel, dim3(blocks, n_sets), dim3(256), 0, st, (double*)scratch, (const float*)x, tab, set_stride);
    hipLaunchKernelGGL(norm_sets_apply_kernel, dim3(blocks, n_sets), dim3(256), 0, st, x, (const double*)scratch, tab, set_stride, step, step_stride,
                       valid, valid_stride, steps_total);
    MGF_CHECK_LAUNCH("noise_sets_normalize");
    return MGF_OK;
}

extern "C" int mgf_noise_sets_grad_f32(float* dnoise, int64_t dnoise_stride, const float* dpre, const float* strength, int32_t n, int32_t c, int64_t hw,
                                       int32_t accumulate, mgf_stream_t stream) {
    MGF_REQUIRE(dnoise && dpre && strength, MGF_EINVAL, "noise_sets_grad: null pointer");
    MGF_REQUIRE(n >= 1 && n <= 65535 && c >= 1 && hw >= 1, MGF_EINVAL, "noise_sets_grad: bad sizes");
    MGF_REQUIRE(hw <= ((int64_t)1 << 30), MGF_EINVAL, "noise_sets_grad: map too large (%lld pixels)", (long long)hw);
    MGF_REQUIRE(dnoise_stride >= hw, MGF_EINVAL, "noise_sets_grad: dnoise_stride %lld is smaller than a map (%lld)", (long long)dnoise_stride,
                (long long)hw);
    const bool vec = hw % 4 == 0 && dnoise_stride % 4 == 0 && ((uintptr_t)dpre % 16) == 0 && ((uintptr_t)dnoise % 16) == 0;
    choose_noise_grad(vec, dnoise, dpre, strength, c, hw, accumulate, (hipStream_t)stream, n, dnoise_stride);
    MGF_CHECK_LAUNCH("noise_sets_grad");
    return MGF_OK;
}

extern "C" int mgf_noise_sets_pack_f32(float* dst, const float* x, const int64_t* offsets, const int32_t* sides, int32_t n_maps, int32_t n_sets,
                                       int64_t set_stride, mgf_stream_t stream) {
    SetTable tab;
    int64_t jobs_doubles = 0, span = 0, total = 0;
    MGF_REQUIRE(dst && x, MGF_EINVAL, "noise_sets_pack: null pointer");
    if (!sets_table("noise_sets_pack", offsets, sides, n_maps, n_sets, set_stride, &tab, &jobs_doubles, &span)) return MGF_EINVAL;
    int blocks = 0;
    for (int m = 0; m < n_maps; ++m) {
        tab.sc[m] = total;                                  // (the pack kernel's reading of `sc`: floats of the maps in front of m)
        total += (int64_t)sides[m] * sides[m];
        blocks += norm_parts(sides[m]);
    }
    MGF_REQUIRE(dst + total * n_sets <= x || x + span <= dst, MGF_EINVAL, "noise_sets_pack: dst must not overlap x");
    hipLaunchKernelGGL(sets_pack_kernel, dim3(blocks, n_sets), dim3(256), 0, (hipStream_t)stream, dst, x, tab, set_stride);
    MGF_CHECK_LAUNCH("noise_sets_pack");
    return MGF_OK;
}
