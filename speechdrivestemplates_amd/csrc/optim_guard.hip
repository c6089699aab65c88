// Optimiser-side safeguards of the flat-buffer Adam: the gradient norm of a step group in float64, the
// device-resident guard record (norm, clip scale, skip flag, skip counter) and the guarded Adam step with the weight EMA fused in.
// No atomics and no host read-back anywhere: every sum has one fixed order, every decision is taken on the device.
#include "common.h"

// ---------------------------------------------------------------------------------------------
// Ordered float64 sum of squares of an fp32 buffer.  The order (the CONTRACT that optim.sumsq_model states in numpy):
//   grid     B = min(max(ceil(nv / 256), 1), SUMSQ_MAX_BLOCKS) blocks of 256 threads, nv = n / 4 whole float4s;
//   thread   t = block * 256 + lane walks the vectors t, t + 256 B, t + 512 B, ... and adds the four squares of each, element 0 first, to
//            one accumulator that starts at +0; thread t < n % 4 then adds the square of tail element 4 nv + t;
//   wave     six butterfly steps v += v[lane ^ o], o = 32, 16, 8, 4, 2, 1 (every lane ends with the same bits);
//   block    (w0 + w1) + (w2 + w3) over its four waves -> partial[1 + block];
//   final    one block: thread t adds partial[1 + t], partial[1 + t + 256], ... in index order, then the same wave and block steps
//            -> partial[0].
// An fp32 square is exact in float64 (48-bit product) and at most 2^256: no sum of fewer than 2^700 of them overflows, so the result is
// non-finite exactly when an element is.
#define SUMSQ_MAX_BLOCKS 2048
#define GUARD_ADAM_MAX_BLOCKS 4096  // as misc.hip's ew_grid: adam_kernel's launch shape

static unsigned sumsq_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv64(n >> 2, 256), SUMSQ_MAX_BLOCKS)); }

__device__ __forceinline__ double block_sum_d(double acc, double* red) {
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ partial) {
    __shared__ double red[4];
    const int64_t nv = n >> 2, stride = (int64_t)gridDim.x * 256;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double acc = 0.0;
#pragma unroll 4
    for (int64_t i = t; i < nv; i += stride) {
        const f32x4 gv = *(const f32x4*)(g + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double x = (double)gv[e];
            acc += x * x;  // (the product is exact: fused or not, the sum rounds once)
        }
    }
    if (t < (n & 3)) {
        const double x = (double)g[(nv << 2) + t];
        acc += x * x;
    }
    const double s = block_sum_d(acc, red);
    if (threadIdx.x == 0) partial[1 + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void grad_sumsq_final_kernel(double* __restrict__ partial, int nblocks) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) acc += partial[1 + i];
    const double s = block_sum_d(acc, red);
    if (threadIdx.x == 0) partial[0] = s;
}

// ---------------------------------------------------------------------------------------------
// The guard record of a step group (32 device bytes, zero-initialised by the caller).
struct GuardRecord {
    double norm;      // grad_scale * sqrt(sum of squares): the L2 norm of the gradient Adam consumes, before clipping
    float scale;      // grad_scale * coef: what the guarded Adam kernel multiplies the gradient by
    int32_t skip;     // 1: this step is not applied
    int64_t skipped;  // running count of skipped steps
    int64_t reserved;
};
struct GuardPartials {
    const double* p[4];
};

__global__ void guard_prep_kernel(GuardPartials parts, int nb, float grad_scale, double max_norm, int skip_nonfinite,
                                  GuardRecord* __restrict__ rec) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += parts.p[b][0];  // argument order
    const double norm = (double)grad_scale * sqrt(s);
    // torch.nn.utils.clip_grad_norm_(norm_type=2, error_if_nonfinite=False): max_norm / (norm + 1e-6), clamped to at most 1; a NaN stays a NaN
    double coef = 1.0;
    if (max_norm > 0.0) {
        coef = max_norm / (norm + 1e-6);
        coef = coef > 1.0 ? 1.0 : coef;
    }
    const bool skip = skip_nonfinite && !isfinite(norm);
    rec->norm = norm;
    rec->scale = (float)((double)grad_scale * coef);
    rec->skip = skip ? 1 : 0;
    if (skip) rec->skipped = rec->skipped + 1;
}

// ---------------------------------------------------------------------------------------------
// misc.hip's Adam with the gradient scale and the skip decision read from the guard record, and the EMA of the new parameters
// written in the same pass.  The arithmetic of the update is adam_kernel's, expression by expression.
struct AdamState {
    int64_t step;
    float bc1, bc2_sqrt;
};
__global__ void adam_guarded_prep_kernel(AdamState* st, float beta1, float beta2, const GuardRecord* __restrict__ rec) {
    if (rec->skip) return;  // a skipped step leaves the counter and the bias corrections where they were
    const int64_t s = st->step + 1;
    st->step = s;
    st->bc1 = (float)(1.0 - pow((double)beta1, (double)s));
    st->bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)s));
}
template <bool EMA>
__global__ __launch_bounds__(256) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, int64_t n, const float* __restrict__ lr_dev,
                                                           float beta1, float beta2, float eps, float wd,
                                                           const GuardRecord* __restrict__ rec, float* __restrict__ ema, float decay,
                                                           const AdamState* __restrict__ st) {
    if (rec->skip) return;  // (uniform over the grid)
    const float gscale = rec->scale;
    const float lr = lr_dev[0];
    const float step_size = lr / st->bc1, bc2s = st->bc2_sqrt;
    const int64_t nv = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
        f32x4 pv = *(f32x4*)(p + 4 * i), gv = *(const f32x4*)(g + 4 * i), mv = *(f32x4*)(m + 4 * i), vv = *(f32x4*)(v + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float gg = gv[e] * gscale;
            if (wd != 0.f) gg += wd * pv[e];
            mv[e] = mv[e] * beta1 + (1.f - beta1) * gg;
            vv[e] = vv[e] * beta2 + (1.f - beta2) * gg * gg;
            const float denom = sqrtf(vv[e]) / bc2s + eps;
            pv[e] = pv[e] - step_size * (mv[e] / denom);
        }
        *(f32x4*)(p + 4 * i) = pv;
        *(f32x4*)(m + 4 * i) = mv;
        *(f32x4*)(v + 4 * i) = vv;
        if (EMA) {
            f32x4 ev = *(f32x4*)(ema + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) ev[e] = ev[e] * decay + (1.f - decay) * pv[e];
            *(f32x4*)(ema + 4 * i) = ev;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = (nv << 2) + threadIdx.x;
        float gg = g[i] * gscale;
        if (wd != 0.f) gg += wd * p[i];
        const float mm = m[i] * beta1 + (1.f - beta1) * gg;
        const float vv = v[i] * beta2 + (1.f - beta2) * gg * gg;
        m[i] = mm;
        v[i] = vv;
        const float pn = p[i] - step_size * (mm / (sqrtf(vv) / bc2s + eps));
        p[i] = pn;
        if (EMA) ema[i] = ema[i] * decay + (1.f - decay) * pn;
    }
}

// ---------------------------------------------------------------------------------------------
extern "C" int64_t sdt_grad_sumsq_partials(void) { return 1 + SUMSQ_MAX_BLOCKS; }
extern "C" int64_t sdt_optim_guard_pass_elems(int which) {
    return which == 0 ? (int64_t)SUMSQ_MAX_BLOCKS * 256 * 4 : which == 1 ? (int64_t)GUARD_ADAM_MAX_BLOCKS * 256 * 4 : -1;
}
extern "C" int sdt_grad_sumsq_f64(const float* g, int64_t n, double* partial, void* stream) {
    SDT_CHECK_ARG(g && partial && n > 0, "bad argument");
    SDT_CHECK_ARG(((uintptr_t)g % 16) == 0 && ((uintptr_t)partial % 8) == 0, "g must be 16-byte aligned, partial 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const unsigned nb = sumsq_blocks(n);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(nb), dim3(256), 0, s, g, n, partial);
    hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(256), 0, s, partial, (int)nb);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
extern "C" int sdt_optim_guard_prep(const double* const* partials, int n_buffers, float grad_scale, double max_norm,
                                    int skip_nonfinite, void* guard, void* stream) {
    SDT_CHECK_ARG(partials && guard && n_buffers >= 1 && n_buffers <= 4, "bad argument (1..4 buffers)");
    SDT_CHECK_ARG(((uintptr_t)guard % 8) == 0, "guard record must be 8-byte aligned");
    SDT_CHECK_ARG(grad_scale == grad_scale && max_norm == max_norm, "grad_scale / max_norm is NaN");
    GuardPartials parts;
    for (int b = 0; b < 4; ++b) {
        parts.p[b] = b < n_buffers ? partials[b] : nullptr;
        SDT_CHECK_ARG(b >= n_buffers || parts.p[b] != nullptr, "null partial buffer");
    }
    hipLaunchKernelGGL(guard_prep_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, parts, n_buffers, grad_scale, max_norm,
                       skip_nonfinite, (GuardRecord*)guard);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
extern "C" int sdt_adam_step_guarded_f32(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1,
                                         float beta2, float eps, float weight_decay, const void* guard, float* ema, float ema_decay,
                                         void* state_dev, void* stream) {
    SDT_CHECK_ARG(p && g && m && v && lr_dev && state_dev && guard && n > 0, "bad argument");
    SDT_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) % 16) == 0, "buffers must be 16-byte aligned");
    SDT_CHECK_ARG(ema == nullptr || (ema_decay > 0.f && ema_decay < 1.f), "ema_decay must lie in (0, 1)");
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv64(n / 4 + 1, 256), GUARD_ADAM_MAX_BLOCKS));
    hipLaunchKernelGGL(adam_guarded_prep_kernel, dim3(1), dim3(1), 0, s, (AdamState*)state_dev, beta1, beta2, (const GuardRecord*)guard);
    if (ema != nullptr)
        hipLaunchKernelGGL(adam_guarded_kernel<true>, dim3(grid), dim3(256), 0, s, p, g, m, v, n, lr_dev, beta1, beta2, eps, weight_decay,
                           (const GuardRecord*)guard, ema, ema_decay, (const AdamState*)state_dev);
    else
        hipLaunchKernelGGL(adam_guarded_kernel<false>, dim3(grid), dim3(256), 0, s, p, g, m, v, n, lr_dev, beta1, beta2, eps, weight_decay,
                           (const GuardRecord*)guard, (float*)nullptr, 0.f, (const AdamState*)state_dev);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
