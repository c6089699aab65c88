// Fitting template codes to clips with the generator held fixed (TEST.FIT_CODE, python -m speechdrivestemplates_amd.code_fit; include/sdt_hip.h
// states the layouts, DESIGN.md section 32 the contract; code_fit.loss_model / step_model / set_model / pick_model in Python are the same
// operations in the same order).  Everything around the Conv1d chain inside an iteration of the fit: the per-clip L1 loss and its gradient,
// the per-clip Adam step on the (B, D) codes with the best iterate kept, and the write of the next code into the chain's own input buffer.
// No floating-point atomics, no allocation, no host synchronisation: every decision is taken on the device, every sum has one fixed order,
// and a clip reads and writes its own rows only -- nothing of one clip can reach another.
//
// Contraction is off for the whole file: every floating-point operation is rounded on its own.  The three multiply-adds of the Adam update
// are WRITTEN as fused operations (fmaf), because that is what the compiler makes of adam_kernel's vector path (csrc/misc.hip) and the step
// has to agree with sdt_adam_step_f32 bit for bit on the same numbers; a fused multiply-add is one operation with one rounding.
#include "common.h"

#pragma clang fp contract(off)

#define CODE_FIT_MAX_D 256  // the step runs one wave per clip, lane l holds the code dimensions l, l + 64, l + 128, l + 192
#define CODE_FIT_PER_LANE (CODE_FIT_MAX_D / 64)

namespace {

__device__ __forceinline__ bool fit_finite_d(double x) { return fabs(x) <= 1.79769313486231570815e308; }  // false for NaN and +-inf
__device__ __forceinline__ bool fit_finite_f(float x) { return fabsf(x) <= 3.40282346638528859812e38f; }

// loss[b] = (sum over the clip of |double(pred) - double(gt)|) / n, dpred = sign(pred - gt) / n.  One workgroup of 256 threads per clip:
//   thread   t adds the elements t, t + 256, t + 512, ... of the clip, in that order, to one float64 accumulator that starts at +0;
//   wave     six butterfly steps v += v[lane ^ o], o = 32, 16, 8, 4, 2, 1;
//   block    (w0 + w1) + (w2 + w3) over its four waves;  loss = sum / double(n), NaN when the sum is not finite.
// The difference of two floats is exact in float64 unless an operand is not finite: its sign is the sign of the real difference.
__global__ __launch_bounds__(256) void code_fit_loss_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int64_t n,
                                                            double* __restrict__ loss, float* __restrict__ dpred) {
    __shared__ double red[4];
    const int64_t base = (int64_t)blockIdx.x * n;
    const float inv = (float)(1.0 / (double)n);
    const float qnan = __int_as_float(0x7fc00000);
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double e = (double)pred[base + i] - (double)gt[base + i];
        acc += fabs(e);
        dpred[base + i] = e > 0.0 ? inv : (e < 0.0 ? -inv : (e == 0.0 ? 0.f : qnan));
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s = (red[0] + red[1]) + (red[2] + red[3]);
        loss[blockIdx.x] = fit_finite_d(s) ? s / (double)n : (double)qnan;
    }
}

// One wave per clip.  mode 0: the whole iteration:
//   1. loss[b] < best_loss[b] (false for a NaN): best_code[b] = code[b], best_loss[b] = loss[b];
//   2. g[d] = float(sum over t = 0 .. T-1, in that order, from +0.0, of double(dh[b, t, C + d]));
//   3. lambda > 0: g[d] = float(double(g[d]) + ((lambda * (double(code[d]) - mu[d])) * ivar[d]) / double(D));
//   4. if loss[b] and every g[d] of the clip are finite: Adam with s = counter + 1, bc1 = float(1 - pow(double(beta1), s)),
//      bc2s = float(sqrt(1 - pow(double(beta2), s))), step_size = lr / bc1 and, per element,
//        m = fmaf(m, beta1, (1 - beta1) * g);  v = fmaf(v, beta2, ((1 - beta2) * g) * g);  code = fmaf(-step_size, m / (sqrtf(v) / bc2s + eps), code)
//      otherwise code, m and v keep their bits and nonfinite[b] = 1;
//   5. h[b, t, C + d] = code[d] for every t (also for a clip that kept its code: the same bits again);
//   6. history[counter, b] = loss[b] where counter < history_rows.
// mode 1: 1 and 6 only (the loss of the last code, after the last step).  The counter is advanced by code_fit_tick_kernel, behind this
// launch on the same stream.
__global__ __launch_bounds__(64) void code_fit_step_kernel(const float* __restrict__ dh, const double* __restrict__ loss, float* __restrict__ code,
                                                           float* __restrict__ m, float* __restrict__ v, float* __restrict__ best_code,
                                                           double* __restrict__ best_loss, const int64_t* __restrict__ counter,
                                                           const float* __restrict__ lr_dev, const double* __restrict__ mu,
                                                           const double* __restrict__ ivar, double lambda, float beta1, float beta2, float eps,
                                                           float* __restrict__ h, int B, int T, int C, int D, double* __restrict__ history,
                                                           int64_t history_rows, int32_t* __restrict__ nonfinite, int mode) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t it = counter[0];
    const double l = loss[b];
    const bool better = l < best_loss[b];  // (every lane reads the old value before lane 0 writes the new one: one wave, program order)
    float c[CODE_FIT_PER_LANE];
#pragma unroll
    for (int j = 0; j < CODE_FIT_PER_LANE; ++j) {
        const int d = lane + 64 * j;
        c[j] = d < D ? code[(int64_t)b * D + d] : 0.f;
        if (better && d < D) best_code[(int64_t)b * D + d] = c[j];
    }
    if (better && lane == 0) best_loss[b] = l;
    if (lane == 0 && it >= 0 && it < history_rows) history[it * B + b] = l;
    if (mode != 0) return;

    const int W = C + D;
    const int64_t row0 = (int64_t)b * T * W + C;
    float g[CODE_FIT_PER_LANE];
    bool ok = fit_finite_d(l);
#pragma unroll
    for (int j = 0; j < CODE_FIT_PER_LANE; ++j) {
        const int d = lane + 64 * j;
        g[j] = 0.f;
        if (d < D) {
            double s = 0.0;
            for (int t = 0; t < T; ++t) s += (double)dh[row0 + (int64_t)t * W + d];
            g[j] = (float)s;
            if (lambda > 0.0) g[j] = (float)((double)g[j] + ((lambda * ((double)c[j] - mu[d])) * ivar[d]) / (double)D);
            ok = ok && fit_finite_f(g[j]);
        }
    }
    ok = __all(ok);  // one decision per clip
    if (ok) {
        const double s = (double)(it + 1);
        const float bc1 = (float)(1.0 - pow((double)beta1, s));
        const float bc2s = (float)sqrt(1.0 - pow((double)beta2, s));
        const float step_size = lr_dev[0] / bc1;
        const float om1 = 1.f - beta1, om2 = 1.f - beta2;
#pragma unroll
        for (int j = 0; j < CODE_FIT_PER_LANE; ++j) {
            const int d = lane + 64 * j;
            if (d < D) {
                const int64_t i = (int64_t)b * D + d;
                const float mm = __builtin_fmaf(m[i], beta1, om1 * g[j]);
                const float vv = __builtin_fmaf(v[i], beta2, (om2 * g[j]) * g[j]);
                const float denom = sqrtf(vv) / bc2s + eps;
                c[j] = __builtin_fmaf(-step_size, mm / denom, c[j]);
                m[i] = mm;
                v[i] = vv;
                code[i] = c[j];
            }
        }
    } else if (lane == 0) {
        nonfinite[b] = 1;
    }
#pragma unroll
    for (int j = 0; j < CODE_FIT_PER_LANE; ++j) {
        const int d = lane + 64 * j;
        if (d < D)
            for (int t = 0; t < T; ++t) h[row0 + (int64_t)t * W + d] = c[j];
    }
}

__global__ void code_fit_tick_kernel(int64_t* counter) { counter[0] = counter[0] + 1; }

// h[b, t, C + d] = codes[b, d]; the first C channels of a row are not touched
__global__ __launch_bounds__(256) void code_fit_set_kernel(const float* __restrict__ codes, float* __restrict__ h, int T, int C, int D, int64_t n) {
    const int W = C + D;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t bt = i / D;
        const int d = (int)(i - bt * D);
        h[bt * W + C + d] = codes[(bt / T) * D + d];
    }
}

// index[b] = the lowest j with the smallest finite cand_loss[j, b] (-1: no candidate of the clip is finite), best[b] = that loss (NaN);
// code_out[b] = cands[max(index[b], 0)].  One wave per clip, lane 0 walks the M candidates in index order.
__global__ __launch_bounds__(64) void code_fit_pick_kernel(const double* __restrict__ cand_loss, int M, int B, const float* __restrict__ cands,
                                                           int D, int32_t* __restrict__ index, double* __restrict__ best,
                                                           float* __restrict__ code_out) {
    __shared__ int pick;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        int arg = -1;
        double lo = 0.0;
        for (int j = 0; j < M; ++j) {
            const double l = cand_loss[(int64_t)j * B + b];
            if (fit_finite_d(l) && (arg < 0 || l < lo)) {
                arg = j;
                lo = l;
            }
        }
        index[b] = arg;
        best[b] = arg >= 0 ? lo : (double)__int_as_float(0x7fc00000);
        pick = arg >= 0 ? arg : 0;
    }
    __syncthreads();
    if (cands != nullptr && code_out != nullptr)
        for (int d = threadIdx.x; d < D; d += 64) code_out[(int64_t)b * D + d] = cands[(int64_t)pick * D + d];
}

bool code_fit_dims_ok(int B, int T, int C, int D) {
    return B > 0 && T > 0 && C >= 0 && D > 0 && D <= CODE_FIT_MAX_D && (int64_t)B * T * ((int64_t)C + D) < ((int64_t)1 << 40);
}

}  // namespace

extern "C" int sdt_code_fit_loss_f32(const float* pred, const float* gt, int B, int64_t n, double* loss, float* dpred, void* stream) {
    SDT_CHECK_ARG(pred && gt && loss && dpred, "null pointer");
    SDT_CHECK_ARG(B > 0 && n > 0 && n < ((int64_t)1 << 40) / B, "B and n must be positive (and B * n below 2^40)");
    SDT_CHECK_ARG(((uintptr_t)loss % 8) == 0, "loss must be 8-byte aligned");
    hipLaunchKernelGGL(code_fit_loss_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pred, gt, n, loss, dpred);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_code_fit_step_f32(const float* dh, const double* loss, float* code, float* m, float* v, float* best_code, double* best_loss,
                                     int64_t* counter, const float* lr_dev, const double* mu, const double* ivar, double lambda, float beta1,
                                     float beta2, float eps, float* h, int B, int T, int C, int D, double* history, int64_t history_rows,
                                     int32_t* nonfinite, int mode, void* stream) {
    SDT_CHECK_ARG(loss && code && best_code && best_loss && counter && history && nonfinite, "null pointer");
    SDT_CHECK_ARG(mode == 0 || mode == 1, "mode must be 0 (iteration) or 1 (bookkeeping only)");
    SDT_CHECK_ARG(code_fit_dims_ok(B, T, C, D), "B, T and D must be positive, C >= 0 and D at most 256");
    SDT_CHECK_ARG(history_rows >= 0, "history_rows must be >= 0");
    SDT_CHECK_ARG(mode == 1 || (dh && m && v && lr_dev && h), "null pointer");
    SDT_CHECK_ARG(lambda == lambda && lambda >= 0.0 && (lambda == 0.0 || (mu && ivar)), "the prior weight must be >= 0 and needs mu and ivar");
    SDT_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f, "bad Adam constants");
    SDT_CHECK_ARG((((uintptr_t)loss | (uintptr_t)best_loss | (uintptr_t)counter | (uintptr_t)history | (uintptr_t)mu |
                    (uintptr_t)ivar) % 8) == 0, "the float64 / int64 buffers must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(code_fit_step_kernel, dim3(B), dim3(64), 0, s, dh, loss, code, m, v, best_code, best_loss, (const int64_t*)counter, lr_dev,
                       mu, ivar, lambda, beta1, beta2, eps, h, B, T, C, D, history, history_rows, nonfinite, mode);
    if (mode == 0) hipLaunchKernelGGL(code_fit_tick_kernel, dim3(1), dim3(1), 0, s, counter);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_code_fit_set_f32(const float* codes, float* h, int B, int T, int C, int D, void* stream) {
    SDT_CHECK_ARG(codes && h, "null pointer");
    SDT_CHECK_ARG(code_fit_dims_ok(B, T, C, D), "B, T and D must be positive, C >= 0 and D at most 256");
    const int64_t n = (int64_t)B * T * D;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(n, 256), 4096);
    hipLaunchKernelGGL(code_fit_set_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, codes, h, T, C, D, n);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_code_fit_pick_f32(const double* cand_loss, int M, int B, const float* cands, int D, int32_t* index, double* best,
                                     float* code_out, void* stream) {
    SDT_CHECK_ARG(cand_loss && index && best, "null pointer");
    SDT_CHECK_ARG(M > 0 && M <= 65536 && B > 0, "M must lie in 1 .. 65536 and B be positive");
    SDT_CHECK_ARG((cands == nullptr) == (code_out == nullptr), "cands and code_out come together");
    SDT_CHECK_ARG(cands == nullptr || (D > 0 && D <= 65536), "D must lie in 1 .. 65536");
    SDT_CHECK_ARG((((uintptr_t)cand_loss | (uintptr_t)best) % 8) == 0, "the float64 buffers must be 8-byte aligned");
    hipLaunchKernelGGL(code_fit_pick_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, cand_loss, M, B, cands, D, index, best, code_out);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
