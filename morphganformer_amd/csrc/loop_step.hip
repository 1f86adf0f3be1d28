// The literal loop's step kernels, all device-side so an iteration never synchronises with the host: the perturbed candidates of a batch
// (mgf_latent_perturb, mgf_latent_perturb_mean), the sequential best-of bookkeeping over them (mgf_select_best, mgf_keep_improvements) and the
// images the drivers save or hand to dlib (mgf_to_uint8_hwc, mgf_reference_gray_u8).  Contract: include/mgf.h.
#include "mgf_common.h"

namespace {

// latent_n[j] = latent_in + eps[s_j] * sigma[s_j], s_j = min(*step + j, steps_total - 1), j < batch
__global__ __launch_bounds__(256) void perturb_kernel(float* latent_n, const float* latent_in, const float* eps, const float* sigma,
                                                      const int32_t* step, int batch, int steps_total, int64_t numel) {
    const int64_t total = (int64_t)batch * numel;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int j = (int)(idx / numel);
        const int64_t i = idx - (int64_t)j * numel;
        int s = *step + j;
        if (s > steps_total - 1) s = steps_total - 1;
        float prod = eps[(int64_t)s * numel + i] * sigma[s];
        asm volatile("" : "+v"(prod));                 // opaque to the fma combiner: two roundings like torch -> bit-exact latents
        latent_n[idx] = latent_in[i] + prod;
    }
}

// projection_example_v2_percept.py:131-166: the optimised latent is [1, copies = 18, k D], every copy gets its own noise, and the generator
// sees `torch.mean(latent_n, 1)`.  The mean must come out bit for bit (the kept latent IS that mean): torch's CPU sum over an outer dimension
// (SumKernel.cpp, cascade_sum / multi_row_sum) adds the rows in blocks of 16 -- each block sequentially from zero, the block sums sequentially
// into a second accumulator -- adds the remaining rows sequentially from zero, then tail + blocks; the mean divides by the count.  Same
// order here, every step of it a separate float32 rounding (no fma: the products are two roundings like torch's `randn_like(..) * strength`).
__global__ __launch_bounds__(256) void perturb_mean_kernel(float* latent_n, const float* latent_in, const float* eps, const float* sigma,
                                                           const int32_t* step, int batch, int steps_total, int64_t numel, int copies) {
    const int64_t total = (int64_t)batch * numel;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int j = (int)(idx / numel);
        const int64_t i = idx - (int64_t)j * numel;
        int s = *step + j;
        if (s > steps_total - 1) s = steps_total - 1;
        const float sg = sigma[s], base = latent_in[i];
        const float* e = eps + ((int64_t)s * copies) * numel + i;
        float blocks = 0.f, run = 0.f;
        for (int c = 0; c < copies; ++c) {
            float prod = e[(int64_t)c * numel] * sg;
            asm volatile("" : "+v"(prod));                 // opaque to the fma combiner
            float v = base + prod;
            asm volatile("" : "+v"(v));
            run = run + v;
            asm volatile("" : "+v"(run));
            if ((c & 15) == 15) { blocks = blocks + run; asm volatile("" : "+v"(blocks)); run = 0.f; }
        }
        latent_n[idx] = (run + blocks) / (float)copies;
    }
}

// candidates j = 0 .. batch-1 are examined in step order, exactly as the sequential loop would
__global__ __launch_bounds__(256) void select_kernel(double* min_loss, float* best_latent, int32_t* best_step, double* losses_out,
                                                     const float* latent_n, int64_t numel, const float* p_loss, const double* w_loss,
                                                     const float* mse_loss, double lamda, float beta, int32_t* step, const int32_t* valid_tab,
                                                     int batch, int steps_total, int32_t* take_slot, int32_t* trail_count, int trail_capacity,
                                                     int32_t* trail_steps, double* trail_losses) {
    __shared__ int take;
    const int s0 = *step;
    int last_full_j = -1;            // (thread 0) candidate of this batch that already sits in the last trail slot
    for (int j = 0; j < batch; ++j) {
        const int s = s0 + j;
        if (s >= steps_total) {
            if (take_slot && threadIdx.x == 0) take_slot[j] = -1;
            continue;
        }
        if (threadIdx.x == 0) {
            const int valid = valid_tab ? valid_tab[s] : 1;
            // same evaluation order and promotions as `p_loss + lamda * w_loss + beta * mse_loss` with a float64 wing term; every product and
            // sum is a rounding of its own like torch's (`total += lamda * w` would contract into one fma under -ffp-contract=on) -- the
            // spelling of demorph.hip's row totals, which promise these bits
            double total = 0.0;
            if (p_loss) total = __dadd_rn(total, (double)p_loss[j]);
            if (w_loss) total = __dadd_rn(total, __dmul_rn(lamda, w_loss[j]));
            if (mse_loss) total = __dadd_rn(total, (double)__fmul_rn(beta, mse_loss[j]));
            if (losses_out) losses_out[s] = valid ? total : __longlong_as_double(0x7ff8000000000000LL);
            take = valid && total < min_loss[0];
            if (take) { min_loss[0] = total; best_step[0] = s; }
            if (take_slot) {
                int slot = -1;
                if (take) {
                    const int cnt = *trail_count;
                    slot = cnt < trail_capacity ? cnt : trail_capacity - 1;
                    if (slot == trail_capacity - 1) {            // two candidates of one batch must not both be copied into the last slot
                        if (last_full_j >= 0) take_slot[last_full_j] = -1;
                        last_full_j = j;
                    }
                    trail_steps[slot] = s;
                    trail_losses[slot] = total;
                    *trail_count = cnt + 1;
                }
                take_slot[j] = slot;
            }
        }
        __syncthreads();
        if (take)
            for (int64_t i = threadIdx.x; i < numel; i += 256) best_latent[i] = latent_n[(int64_t)j * numel + i];
        __syncthreads();
    }
    if (threadIdx.x == 0) *step = s0 + batch < steps_total ? s0 + batch : steps_total;
}

// trail_imgs[take_slot[j]] = imgs[j] for the improving candidates of a batch; grid (blocks, batch), float4 body + scalar tail
__global__ __launch_bounds__(256) void keep_improvements_kernel(float* __restrict__ trail, const float* __restrict__ imgs, int64_t numel,
                                                                const int32_t* __restrict__ take_slot) {
    const int j = blockIdx.y;
    const int slot = take_slot[j];
    if (slot < 0) return;
    const float* src = imgs + (int64_t)j * numel;
    float* dst = trail + (int64_t)slot * numel;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if ((numel & 3) == 0) {
        const int64_t n4 = numel >> 2;
        for (int64_t i = tid; i < n4; i += stride) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
    } else {
        for (int64_t i = tid; i < numel; i += stride) dst[i] = src[i];
    }
}

__global__ __launch_bounds__(256) void to_uint8_kernel(uint8_t* out, const float* img, int c, int h, int w) {
    const int64_t hw = (int64_t)h * w, total = hw * c;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ch = (int)(i % c);
        const int64_t px = i / c;
        float v = __fadd_rn(__fmul_rn(img[(int64_t)ch * hw + px], 127.5f), 127.5f);      // two roundings like numpy's `data * scale + bias` (misc.py:103-104)
        v = rintf(v);
        v = fminf(fmaxf(v, 0.f), 255.f);
        out[i] = (uint8_t)v;
    }
}

// ---- the gray uint8 image the drivers hand to dlib (...sqz_MSE.py:159-163): cv2.normalize(img, None, 0, 255, NORM_MINMAX, CV_8U) over the
// WHOLE float image, then cv2.cvtColor(COLOR_BGR2GRAY) on RGB-ordered data.  Two passes per candidate: partial minima / maxima, then the
// conversion (every block of the second pass first folds the candidate's partials: min / max do not depend on the order).
constexpr int GRAY_PARTS = 256;

__global__ __launch_bounds__(256) void minmax_partial_kernel(float* part, const float* img, int64_t per) {
    __shared__ float slo[4], shi[4];
    const float* x = img + (int64_t)blockIdx.y * per;
    float lo = INFINITY, hi = -INFINITY;
    const int64_t n4 = per / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        lo = fminf(fminf(lo, fminf(v.x, v.y)), fminf(v.z, v.w));
        hi = fmaxf(fmaxf(hi, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
    for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) { lo = fminf(lo, x[i]); hi = fmaxf(hi, x[i]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = lo; shi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* p = part + ((int64_t)blockIdx.y * GRAY_PARTS + blockIdx.x) * 2;
        p[0] = fminf(fminf(slo[0], slo[1]), fminf(slo[2], slo[3]));
        p[1] = fmaxf(fmaxf(shi[0], shi[1]), fmaxf(shi[2], shi[3]));
    }
}

// u8 = clip(rint((double(x) - lo) * (255.0 / (hi - lo)))), the scale 0 for a flat image, exactly the arithmetic of drivers.reference_gray_u8;
// gray = (c0 * 1868 + c1 * 9617 + c2 * 4899 + (1 << 13)) >> 14: OpenCV's 8-bit BGR2GRAY coefficients (B 1868, G 9617, R 4899) with channel 0 -- RED
// in the generator's RGB order -- in the blue slot, as the drivers call it.  img [n,3,h,w] planar -> gray [n,h,w]
__global__ __launch_bounds__(256) void gray_u8_kernel(uint8_t* gray, const float* img, const float* part, int nparts, int64_t hw) {
    __shared__ float slo[4], shi[4];
    const int n = blockIdx.y;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < nparts; i += 256) { lo = fminf(lo, part[((int64_t)n * GRAY_PARTS + i) * 2]); hi = fmaxf(hi, part[((int64_t)n * GRAY_PARTS + i) * 2 + 1]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = lo; shi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    const double dlo = (double)fminf(fminf(slo[0], slo[1]), fminf(slo[2], slo[3])), dhi = (double)fmaxf(fmaxf(shi[0], shi[1]), fmaxf(shi[2], shi[3]));
    const double scale = dhi > dlo ? 255.0 / (dhi - dlo) : 0.0;
    const float* x = img + (int64_t)n * 3 * hw;
    uint8_t* g = gray + (int64_t)n * hw;
    auto q = [&](float v) -> unsigned {
        double t = rint(__dmul_rn(__dsub_rn((double)v, dlo), scale));
        t = t < 0.0 ? 0.0 : (t > 255.0 ? 255.0 : t);
        return (unsigned)t;
    };
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < hw; i += (int64_t)gridDim.x * 1024) {
        if (i + 4 <= hw && (hw & 3) == 0) {
            const float4 a = *reinterpret_cast<const float4*>(x + i), b = *reinterpret_cast<const float4*>(x + hw + i),
                         c = *reinterpret_cast<const float4*>(x + 2 * hw + i);
            const unsigned g0 = (q(a.x) * 1868u + q(b.x) * 9617u + q(c.x) * 4899u + (1u << 13)) >> 14;
            const unsigned g1 = (q(a.y) * 1868u + q(b.y) * 9617u + q(c.y) * 4899u + (1u << 13)) >> 14;
            const unsigned g2 = (q(a.z) * 1868u + q(b.z) * 9617u + q(c.z) * 4899u + (1u << 13)) >> 14;
            const unsigned g3 = (q(a.w) * 1868u + q(b.w) * 9617u + q(c.w) * 4899u + (1u << 13)) >> 14;
            *reinterpret_cast<uint32_t*>(g + i) = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
        } else {
            for (int64_t j = i; j < hw && j < i + 4; ++j)
                g[j] = (uint8_t)((q(x[j]) * 1868u + q(x[hw + j]) * 9617u + q(x[2 * hw + j]) * 4899u + (1u << 13)) >> 14);
        }
    }
}

}  // namespace

extern "C" int mgf_latent_perturb(float* latent_n, const float* latent_in, const float* eps, const float* sigma, const int32_t* step,
                                  int32_t batch, int32_t steps_total, int64_t numel, mgf_stream_t stream) {
    MGF_REQUIRE(latent_n && latent_in && eps && sigma && step && numel >= 1 && batch >= 1 && steps_total >= 1, MGF_EINVAL,
                "latent_perturb: bad arguments");
    hipLaunchKernelGGL(perturb_kernel, dim3((unsigned)mgf_cdiv(numel * batch, 256)), dim3(256), 0, (hipStream_t)stream, latent_n, latent_in,
                       eps, sigma, step, batch, steps_total, numel);
    MGF_CHECK_LAUNCH("latent_perturb");
    return MGF_OK;
}

extern "C" int mgf_latent_perturb_mean(float* latent_n, const float* latent_in, const float* eps, const float* sigma, const int32_t* step,
                                       int32_t batch, int32_t steps_total, int64_t numel, int32_t copies, mgf_stream_t stream) {
    MGF_REQUIRE(latent_n && latent_in && eps && sigma && step && numel >= 1 && batch >= 1 && steps_total >= 1, MGF_EINVAL,
                "latent_perturb_mean: bad arguments");
    MGF_REQUIRE(copies >= 1 && copies <= 255, MGF_EUNSUPPORTED, "latent_perturb_mean: 1 .. 255 copies (torch's two-level summation order; got %d)", copies);
    hipLaunchKernelGGL(perturb_mean_kernel, dim3((unsigned)mgf_cdiv(numel * batch, 256)), dim3(256), 0, (hipStream_t)stream, latent_n, latent_in,
                       eps, sigma, step, batch, steps_total, numel, copies);
    MGF_CHECK_LAUNCH("latent_perturb_mean");
    return MGF_OK;
}

extern "C" int mgf_select_best(double* min_loss, float* best_latent, int32_t* best_step, double* losses_out, const float* latent_n,
                               int64_t numel, const float* p_loss, const double* w_loss, const float* mse_loss, double lamda, float beta,
                               int32_t* step, const int32_t* valid, int32_t batch, int32_t steps_total, int32_t* take_slot,
                               int32_t* trail_count, int32_t trail_capacity, int32_t* trail_steps, double* trail_losses, mgf_stream_t stream) {
    MGF_REQUIRE(min_loss && best_latent && best_step && latent_n && step && numel >= 1 && batch >= 1 && steps_total >= 1, MGF_EINVAL,
                "select_best: bad arguments");
    MGF_REQUIRE(!take_slot || (trail_count && trail_steps && trail_losses && trail_capacity >= 1), MGF_EINVAL,
                "select_best: take_slot needs trail_count, trail_steps, trail_losses and a capacity >= 1");
    hipLaunchKernelGGL(select_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, min_loss, best_latent, best_step, losses_out, latent_n,
                       numel, p_loss, w_loss, mse_loss, lamda, beta, step, valid, batch, steps_total, take_slot, trail_count, trail_capacity,
                       trail_steps, trail_losses);
    MGF_CHECK_LAUNCH("select_best");
    return MGF_OK;
}

extern "C" int mgf_keep_improvements(float* trail_imgs, const float* imgs, int64_t numel, const int32_t* take_slot, int32_t batch,
                                     mgf_stream_t stream) {
    MGF_REQUIRE(trail_imgs && imgs && take_slot && numel >= 1 && batch >= 1 && batch <= 65535, MGF_EINVAL, "keep_improvements: bad arguments");
    MGF_REQUIRE((numel & 3) != 0 || ((((uintptr_t)trail_imgs | (uintptr_t)imgs) & 15) == 0), MGF_EINVAL, "keep_improvements: buffers must be 16-byte aligned");
    const int64_t want = (numel / 4 + 255) / 256 + 1;
    const int blocks = (int)(want < 512 ? want : 512);
    hipLaunchKernelGGL(keep_improvements_kernel, dim3(blocks, batch), dim3(256), 0, (hipStream_t)stream, trail_imgs, imgs, numel, take_slot);
    MGF_CHECK_LAUNCH("keep_improvements");
    return MGF_OK;
}

extern "C" int mgf_to_uint8_hwc(uint8_t* out, const float* img, int32_t c, int32_t h, int32_t w, mgf_stream_t stream) {
    MGF_REQUIRE(out && img && c >= 1 && h >= 1 && w >= 1, MGF_EINVAL, "to_uint8: bad arguments");
    const int64_t total = (int64_t)c * h * w;
    hipLaunchKernelGGL(to_uint8_kernel, dim3(mgf_stream_grid(total, 256, 4)), dim3(256), 0, (hipStream_t)stream, out, img, c, h, w);
    MGF_CHECK_LAUNCH("to_uint8");
    return MGF_OK;
}

extern "C" int64_t mgf_reference_gray_scratch_floats(void) { return 2 * GRAY_PARTS; }

extern "C" int mgf_reference_gray_u8(uint8_t* gray, const float* img, int32_t n, int32_t h, int32_t w, float* scratch, mgf_stream_t stream) {
    MGF_REQUIRE(gray && img && scratch && n >= 1 && n <= 65535 && h >= 1 && w >= 1, MGF_EINVAL, "reference_gray_u8: bad arguments");
    MGF_REQUIRE(((uintptr_t)img % 16) == 0 && ((uintptr_t)gray % 4) == 0, MGF_EINVAL, "reference_gray_u8: img must be 16-byte, gray 4-byte aligned");
    const int64_t hw = (int64_t)h * w, per = 3 * hw;
    MGF_REQUIRE(per % 4 == 0 || n == 1, MGF_EINVAL, "reference_gray_u8: a batch needs 16-byte aligned samples (3 h w a multiple of 4)");
    const int parts = (int)(mgf_cdiv(per, 256 * 16) < GRAY_PARTS ? mgf_cdiv(per, 256 * 16) : GRAY_PARTS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(minmax_partial_kernel, dim3(parts, n), dim3(256), 0, st, scratch, img, per);
    const int blocks = (int)(mgf_cdiv(hw, 1024 * 4) < 1024 ? mgf_cdiv(hw, 1024 * 4) : 1024);
    hipLaunchKernelGGL(gray_u8_kernel, dim3(blocks < 1 ? 1 : blocks, n), dim3(256), 0, st, gray, img, scratch, parts, hw);
    MGF_CHECK_LAUNCH("reference_gray_u8");
    return MGF_OK;
}
