// Regression loss with a confidence mask, per-channel weights and a velocity (first-difference) term: the opt-in form of the L1
// loss of misc.hip (VOICE2POSE.GENERATOR.LAMBDA_VEL / REG_MIN_CONFIDENCE / REG_PART_WEIGHTS).
//
//   e = double(pred) - double(gt)  (B, T, C);   d[b,t,c] = e[b,t+1,c] - e[b,t,c]  (t < T-1)
//   m = score > min_conf ? 1 : 0  (1 everywhere without a score);   m2[b,t,c] = m[b,t,c] * m[b,t+1,c];   w[c] = chan_w[c] (1 without)
//   reg = lambda_reg * sum(m  * w * |e|) / max(sum m , 1)
//   vel = lambda_vel * sum(m2 * w * |d|) / max(sum m2, 1)
//
// Forward: one pass (every thread takes element (b,t,c) and its t+1 neighbour) into per-block float64 sums and integer counts, then one
// block that combines them in a fixed order, divides ON THE DEVICE and keeps the two denominators for backward -- the reduction shape of
// l1_partial_kernel / l1_final_kernel, no atomics, bit-identical from call to call.  Backward: one pass over the t-1 / t / t+1 neighbours.
// A masked element is SELECTED away, never multiplied by 0: a NaN or a huge value under the mask reaches neither a sum nor a gradient.
#include "common.h"

#define REG_LOSS_MAX_BLOCKS 256

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ bool reg_live(const float* __restrict__ score, int64_t i, float min_conf) { return score == nullptr || score[i] > min_conf; }
__device__ __forceinline__ double sign_d(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }  // torch.sign: sign(0) = 0

// partial: [0, nblk) sums of m*w*|e|, [MAX, MAX + nblk) sums of m2*w*|d|;  counts: [0, nblk) sum m, [MAX, MAX + nblk) sum m2
__global__ __launch_bounds__(256) void reg_loss_partial_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                               const float* __restrict__ score, const float* __restrict__ chan_w, int T,
                                                               int C, int64_t n, float min_conf, double* __restrict__ partial,
                                                               unsigned long long* __restrict__ counts) {
    __shared__ double red[2][4];
    __shared__ unsigned long long redc[2][4];
    double s_reg = 0.0, s_vel = 0.0;
    unsigned long long c_reg = 0, c_vel = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t bt = i / C;
        const int c = (int)(i - bt * C);
        const int t = (int)(bt % T);
        const double w = chan_w ? (double)chan_w[c] : 1.0;
        const bool m0 = reg_live(score, i, min_conf);
        const double e0 = (double)p[i] - (double)g[i];
        s_reg += m0 ? w * fabs(e0) : 0.0;
        c_reg += m0 ? 1u : 0u;
        if (t < T - 1) {  // (i + C < n: frame t + 1 of the same clip)
            const bool m2 = m0 && reg_live(score, i + C, min_conf);
            const double e1 = (double)p[i + C] - (double)g[i + C];
            s_vel += m2 ? w * fabs(e1 - e0) : 0.0;
            c_vel += m2 ? 1u : 0u;
        }
    }
    s_reg = wave_sum_d(s_reg);
    s_vel = wave_sum_d(s_vel);
    c_reg = wave_sum_u64(c_reg);
    c_vel = wave_sum_u64(c_vel);
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        red[0][wv] = s_reg;
        red[1][wv] = s_vel;
        redc[0][wv] = c_reg;
        redc[1][wv] = c_vel;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int q = threadIdx.x;
        partial[q * REG_LOSS_MAX_BLOCKS + blockIdx.x] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
        counts[q * REG_LOSS_MAX_BLOCKS + blockIdx.x] = (redc[q][0] + redc[q][1]) + (redc[q][2] + redc[q][3]);
    }
}

// losses[q] = (float)(lambda_q * sum_q / denom_q), denom_q = max(count_q, 1): the quotient in float64, one rounding to fp32
__global__ __launch_bounds__(256) void reg_loss_final_kernel(const double* __restrict__ partial, const unsigned long long* __restrict__ counts,
                                                             int nblk, double lambda_reg, double lambda_vel, float* __restrict__ losses,
                                                             double* __restrict__ denom) {
    __shared__ double red[2][4];
    __shared__ unsigned long long redc[2][4];
    double s[2] = {0.0, 0.0};
    unsigned long long k[2] = {0, 0};
    for (int i = threadIdx.x; i < nblk; i += 256) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            s[q] += partial[q * REG_LOSS_MAX_BLOCKS + i];
            k[q] += counts[q * REG_LOSS_MAX_BLOCKS + i];
        }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        s[q] = wave_sum_d(s[q]);
        k[q] = wave_sum_u64(k[q]);
        if ((threadIdx.x & 63) == 0) {
            red[q][threadIdx.x >> 6] = s[q];
            redc[q][threadIdx.x >> 6] = k[q];
        }
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int q = threadIdx.x;
        const double sum = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
        const unsigned long long cnt = (redc[q][0] + redc[q][1]) + (redc[q][2] + redc[q][3]);
        const double den = cnt > 0 ? (double)cnt : 1.0;
        denom[q] = den;
        losses[q] = (float)((q == 0 ? lambda_reg : lambda_vel) * sum / den);
    }
}

// dpred = (float)((creg * w) * m * sign(e) + (cvel * w) * m2[t-1] * sign(d[t-1]) - (cvel * w) * m2[t] * sign(d[t])) in float64, with
// creg = (gout_reg / denom[0]) * lambda_reg and cvel = (gout_vel / denom[1]) * lambda_vel.  The order is autograd's on the float64 torch
// expression lambda * sum(m w |e|) / count: where the terms of an element cancel there (creg == cvel happens: 0.75 * 0.7 / 112 and
// 1.5 * 0.3 / 96) they cancel here to the same exact 0, instead of leaving the 1e-19 that one differently rounded coefficient would.
__global__ __launch_bounds__(256) void reg_loss_bwd_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                           const float* __restrict__ score, const float* __restrict__ chan_w,
                                                           const float* __restrict__ gout_reg, const float* __restrict__ gout_vel,
                                                           const double* __restrict__ denom, int T, int C, int64_t n, double lambda_reg,
                                                           double lambda_vel, float min_conf, float* __restrict__ dp) {
    const double creg = gout_reg ? (double)gout_reg[0] / denom[0] * lambda_reg : 0.0;
    const double cvel = gout_vel ? (double)gout_vel[0] / denom[1] * lambda_vel : 0.0;
    const bool vel = gout_vel != nullptr && lambda_vel != 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t bt = i / C;
        const int c = (int)(i - bt * C);
        const int t = (int)(bt % T);
        float out = 0.f;
        if (reg_live(score, i, min_conf)) {  // a masked element takes part in no term: m = 0 and both of its pairs have m2 = 0
            const double w = chan_w ? (double)chan_w[c] : 1.0;
            const double e0 = (double)p[i] - (double)g[i];
            double k = (creg * w) * sign_d(e0);  // (a product with a sign is exact)
            if (vel) {
                const double vw = cvel * w;
                if (t >= 1 && reg_live(score, i - C, min_conf)) k += vw * sign_d(e0 - ((double)p[i - C] - (double)g[i - C]));
                if (t < T - 1 && reg_live(score, i + C, min_conf)) k -= vw * sign_d(((double)p[i + C] - (double)g[i + C]) - e0);
            }
            out = (float)k;
        }
        dp[i] = out;
    }
}

static bool reg_loss_dims_ok(int B, int T, int C) { return B > 0 && T > 0 && C > 0; }

extern "C" int sdt_reg_loss_fwd_f32(const float* pred, const float* gt, const float* score, const float* chan_w, int B, int T, int C,
                                    double lambda_reg, double lambda_vel, float min_conf, double* partial, int64_t* counts, float* losses,
                                    double* denom, void* stream) {
    SDT_CHECK_ARG(pred && gt && partial && counts && losses && denom, "null pointer");
    SDT_CHECK_ARG(reg_loss_dims_ok(B, T, C), "B, T and C must be positive");
    SDT_CHECK_ARG(lambda_reg >= 0.0 && lambda_vel >= 0.0, "the weights must be >= 0");  // (false for NaN too)
    SDT_CHECK_ARG(score == nullptr || min_conf == min_conf, "min_conf is NaN");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)B * T * C;
    const int nblk = (int)std::min<int64_t>(REG_LOSS_MAX_BLOCKS, cdiv64(n, 256));
    hipLaunchKernelGGL(reg_loss_partial_kernel, dim3(nblk), dim3(256), 0, s, pred, gt, score, chan_w, T, C, n, min_conf, partial,
                       (unsigned long long*)counts);
    hipLaunchKernelGGL(reg_loss_final_kernel, dim3(1), dim3(256), 0, s, partial, (const unsigned long long*)counts, nblk, lambda_reg,
                       lambda_vel, losses, denom);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_reg_loss_bwd_f32(const float* pred, const float* gt, const float* score, const float* chan_w, const float* gout_reg,
                                    const float* gout_vel, const double* denom, int B, int T, int C, double lambda_reg, double lambda_vel,
                                    float min_conf, float* dpred, void* stream) {
    SDT_CHECK_ARG(pred && gt && denom && dpred, "null pointer");
    SDT_CHECK_ARG(reg_loss_dims_ok(B, T, C), "B, T and C must be positive");
    SDT_CHECK_ARG(lambda_reg >= 0.0 && lambda_vel >= 0.0, "the weights must be >= 0");
    SDT_CHECK_ARG(score == nullptr || min_conf == min_conf, "min_conf is NaN");
    const int64_t n = (int64_t)B * T * C;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(n, 256), 4096);
    hipLaunchKernelGGL(reg_loss_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, pred, gt, score, chan_w, gout_reg, gout_vel,
                       denom, T, C, n, lambda_reg, lambda_vel, min_conf, dpred);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
