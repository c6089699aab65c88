// First audio-encoder block (Conv2d 1->64 k3 s1 p1 + InstanceNorm2d/BatchNorm2d + LeakyReLU, generator.py:16,
// building_blocks.py:15-26,46) fused for the single-input-channel case.  Its output is the largest tensor of the
// network (B x 80 x 427 x 64 = 280 MB at B=32) and every pass over it is HBM time, while the convolution itself is 9
// MACs per element.  Two facts make a one-pass forward possible:
//   * y[c] = sum_t w[c][t] * x_t  (x_t = the 9 zero-padded neighbours of the mel pixel), hence
//       sum_pos y[c]   = sum_t w[c][t] S_t                    S_t    = sum_pos x_t
//       sum_pos y[c]^2 = sum_{t,u} w[c][t] w[c][u] R_{t,u}    R_{t,u} = sum_pos x_t x_u
//     i.e. the per-(clip, channel) statistics of ALL 64 channels follow from 9 + 45 moments of the 4.4 MB mel image
//     (accumulated in fp64); the normalised, activated output is then written exactly once, and the raw conv output is
//     never stored;
//   * in backward the normalised pre-activation is recomputed from the mel image (36 FMAs per 4 channels) instead of
//     being re-read: statistics of the incoming gradient and the weight gradient each read dz once.
// Forward: l0_moments -> l0_finalize -> l0_fwd (1 write of 280 MB).  Backward: l0_bwd_sums (THE one read of the gradient)
// -> l0_bwd_finalize: the weight gradient is assembled from 11 sums per channel and the forward pass's mel moments.
#include "common.h"

#define L0_C 64
#define L0_T 9
#define L0_NMOM 54  // 9 first moments + 45 upper-triangular second moments

__device__ __forceinline__ void l0_gather(const float* __restrict__ mel, int H, int W, int y, int x, float (&nb)[L0_T]) {
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int yy = y + dy, xx = x + dx;
            nb[(dy + 1) * 3 + (dx + 1)] = ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) ? mel[(size_t)yy * W + xx] : 0.f;
        }
}

// Sliding 3x3 window along one image row: each step shifts the window one pixel to the right and loads the 3 new
// right-column values (zero outside the image) -- 3 loads per pixel instead of 9 and no integer division.
struct L0Window {
    float nb[L0_T];
    const float* r0;
    const float* r1;
    const float* r2;  // rows y-1, y, y+1 (nullptr when outside the image)
    int W;
    __device__ __forceinline__ float at(const float* r, int x) const { return (r != nullptr && (unsigned)x < (unsigned)W) ? r[x] : 0.f; }
    __device__ __forceinline__ void init(const float* img, int H, int W_, int y, int x) {
        W = W_;
        r0 = (y - 1 >= 0) ? img + (size_t)(y - 1) * W : nullptr;
        r1 = img + (size_t)y * W;
        r2 = (y + 1 < H) ? img + (size_t)(y + 1) * W : nullptr;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            nb[d] = at(r0, x - 1 + d);
            nb[3 + d] = at(r1, x - 1 + d);
            nb[6 + d] = at(r2, x - 1 + d);
        }
    }
    __device__ __forceinline__ void advance(int xnew) {  // window now centred on xnew (= previous centre + 1)
        nb[0] = nb[1]; nb[1] = nb[2]; nb[2] = at(r0, xnew + 1);
        nb[3] = nb[4]; nb[4] = nb[5]; nb[5] = at(r1, xnew + 1);
        nb[6] = nb[7]; nb[7] = nb[8]; nb[8] = at(r2, xnew + 1);
    }
};

// grid (chunks, B); mom[b][54] doubles (zeroed by the caller)
// FEW (an image of at most L0_FEW pixels): sums and products in fp64, where the product of two fp32 values is exact.  The variance of a channel
// is a quadratic form of these moments minus m^2, and with fp32 products it carries 2^-24 (1 + (mean/std)^2) of relative error; among the 64
// channels of a two-pixel image some have their two outputs close together (mean/std of 100 .. 200: the forward output lost two digits, 2.9e-4
// of max at (B, H, W) = (2, 1, 2)) -- the case colstats_kernel (norm.hip) meets with up to four rows, with the same remedy and the same
// threshold.  A separate instantiation: the 54 fp64 accumulators would otherwise count against every launch's registers; larger images keep
// the fp32 partials and their bits.
#define L0_FEW 4
template <bool FEW> struct L0MomAcc { typedef float type; };
template <> struct L0MomAcc<true> { typedef double type; };
template <bool FEW>
__global__ __launch_bounds__(256) void l0_moments_kernel(const float* __restrict__ mel, double* __restrict__ mom, int H, int W,
                                                         int pix_per_block) {
    typedef typename L0MomAcc<FEW>::type acc_t;
    __shared__ double sM[L0_NMOM];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid < L0_NMOM) sM[tid] = 0.0;
    __syncthreads();
    const float* img = mel + (size_t)b * H * W;
    const int p0 = blockIdx.x * pix_per_block, p1 = min(H * W, p0 + pix_per_block);
    acc_t acc[L0_NMOM];
#pragma unroll
    for (int i = 0; i < L0_NMOM; ++i) acc[i] = (acc_t)0;
    for (int p = p0 + tid; p < p1; p += 256) {
        float nb[L0_T];
        l0_gather(img, H, W, p / W, p % W, nb);
        int k = L0_T;
#pragma unroll
        for (int t = 0; t < L0_T; ++t) {
            acc[t] += (acc_t)nb[t];
#pragma unroll
            for (int u = t; u < L0_T; ++u) acc[k++] += (acc_t)nb[t] * (acc_t)nb[u];
        }
    }
#pragma unroll
    for (int i = 0; i < L0_NMOM; ++i) {
        const double s = wave_sum_d((double)acc[i]);
        if ((tid & 63) == 0) atomicAdd(&sM[i], s);
    }
    __syncthreads();
    if (tid < L0_NMOM) atomicAdd(&mom[(size_t)b * L0_NMOM + tid], sM[tid]);
}

// one thread per (group, channel): mean / rstd from the moments (groups == B: InstanceNorm; groups == 1: BatchNorm)
__global__ void l0_finalize_kernel(const double* __restrict__ mom, const float* __restrict__ w, float* __restrict__ mean,
                                   float* __restrict__ rstd, float* __restrict__ rmean, float* __restrict__ rvar,
                                   int64_t* __restrict__ nbt, int B, int groups, double n_per_group, float eps, float momentum) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= groups * L0_C) return;
    const int g = i / L0_C, c = i % L0_C;
    double M[L0_NMOM];
    for (int k = 0; k < L0_NMOM; ++k) {
        double s = 0.0;
        if (groups == 1)
            for (int b = 0; b < B; ++b) s += mom[(size_t)b * L0_NMOM + k];
        else
            s = mom[(size_t)g * L0_NMOM + k];
        M[k] = s;
    }
    double wv[L0_T];
    for (int t = 0; t < L0_T; ++t) wv[t] = (double)w[c * L0_T + t];
    double s = 0.0, q = 0.0;
    int k = L0_T;
    for (int t = 0; t < L0_T; ++t) {
        s += wv[t] * M[t];
        for (int u = t; u < L0_T; ++u) q += (u == t ? 1.0 : 2.0) * wv[t] * wv[u] * M[k++];
    }
    const double m = s / n_per_group;
    double var = q / n_per_group - m * m;
    var = var > 0.0 ? var : 0.0;
    mean[i] = (float)m;
    rstd[i] = (float)(1.0 / sqrt(var + (double)eps));
    if (rmean != nullptr && groups == 1) {
        const double unb = n_per_group > 1.0 ? n_per_group / (n_per_group - 1.0) : 1.0;
        rmean[c] = (1.f - momentum) * rmean[c] + momentum * (float)m;
        rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)(var * unb);
        if (nbt != nullptr && c == 0) nbt[0] += 1;
    }
}

// thread = (pixel, channel quad): 16 threads per pixel, 16 pixels per 256-thread pass
struct L0Thread {
    float w[4][L0_T];
    f32x4 mu, rs, ga, be;
};
__device__ __forceinline__ void l0_setup(L0Thread& t, const float* __restrict__ w, const float* __restrict__ mean,
                                         const float* __restrict__ rstd, const float* __restrict__ gamma,
                                         const float* __restrict__ beta, int g, int cq) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int k = 0; k < L0_T; ++k) t.w[e][k] = w[(4 * cq + e) * L0_T + k];
    t.mu = *(const f32x4*)(mean + (size_t)g * L0_C + 4 * cq);
    t.rs = *(const f32x4*)(rstd + (size_t)g * L0_C + 4 * cq);
    t.ga = gamma ? *(const f32x4*)(gamma + 4 * cq) : (f32x4){1.f, 1.f, 1.f, 1.f};
    t.be = beta ? *(const f32x4*)(beta + 4 * cq) : (f32x4){0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ f32x4 l0_yhat(const L0Thread& t, const float (&nb)[L0_T]) {
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < L0_T; ++k) s = fmaf(nb[k], t.w[e][k], s);
        y[e] = (s - t.mu[e]) * t.rs[e];
    }
    return y;
}

// four consecutive channels as fp32 <-> the tensor's element type (fp32, or bf16 in the bf16-storage path)
typedef unsigned l0_u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 l0_bf16x4 __attribute__((ext_vector_type(4)));
template <typename T>
__device__ __forceinline__ f32x4 l0_ld4(const T* __restrict__ p) {
    if constexpr (sizeof(T) == 4) {
        return *(const f32x4*)p;
    } else {
        const l0_u32x2 w = *(const l0_u32x2*)p;
        return (f32x4){__uint_as_float(w[0] << 16), __uint_as_float(w[0] & 0xffff0000u), __uint_as_float(w[1] << 16), __uint_as_float(w[1] & 0xffff0000u)};
    }
}
template <typename T>
__device__ __forceinline__ void l0_st4(T* __restrict__ p, const f32x4 v) {
    if constexpr (sizeof(T) == 4) {
        *(f32x4*)p = v;
    } else {
        l0_bf16x4 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = (__bf16)v[e];
        *(l0_bf16x4*)p = h;
    }
}

// grid (H, B): one image row per workgroup; thread = (segment of the row, channel quad): 16 segments x 16 quads
template <typename TZ>
__global__ __launch_bounds__(256) void l0_fwd_kernel(const float* __restrict__ mel, const float* __restrict__ w,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     TZ* __restrict__ z, int H, int W, int groups, float slope) {
    const int b = blockIdx.y, y = blockIdx.x, tid = threadIdx.x, cq = tid & 15, seg = tid >> 4;
    L0Thread t;
    l0_setup(t, w, mean, rstd, gamma, beta, groups == 1 ? 0 : b, cq);
    const int len = (W + 15) / 16, x0 = seg * len, x1 = min(W, x0 + len);
    if (x0 >= x1) return;
    TZ* out = z + ((size_t)(b * H + y) * W) * L0_C + 4 * cq;
    L0Window win;
    win.init(mel + (size_t)b * H * W, H, W, y, x0);
    for (int x = x0; x < x1; ++x) {
        if (x > x0) win.advance(x);
        const f32x4 yh = l0_yhat(t, win.nb);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = act_fwd(yh[e] * t.ga[e] + t.be[e], slope);
        l0_st4(out + (size_t)x * L0_C, o);
    }
}

#define L0_Q 4      // gradient vectors per register set of the backward kernel's prefetch
#define L0_NSUM 11  // per (group, channel): sum g, sum g*yhat, sum g*x_t (9 taps)   with g = dz * act'(gamma*yhat+beta)

// Backward, the ONLY pass over dz.  With dy = gamma*rstd*(g - mean(g) - yhat*mean(g*yhat)) the weight gradient
//   dW[c][t] = sum_pos dy*x_t = gamma*rstd*( sum g*x_t - mean(g)*sum x_t - mean(g*yhat)*sum yhat*x_t )
// needs, besides three sums over the gradient, only  sum x_t  and  sum yhat*x_t = rstd*(sum_u w[c][u] R[u][t] - mean*S_t),
// i.e. the first/second moments of the mel image that the forward pass already computed.
// sums[g][c][11] doubles (zero on entry).  grid (row chunks, B).
// The gradient vectors of a thread go through a FOUR-DEEP QUEUE of raw registers that is refilled slot by slot: the load of pixel p + 4 is
// issued the moment pixel p's vector is taken out, and the pixel loop is one basic block (tails are masked, addresses clamped), so the
// compiler waits with vmcnt(3) -- not 0 -- and a wave's ~100 VALU operations per pixel run under its own loads.  The mel neighbourhood
// comes from LDS (the workgroup's rows + halo, zero border): as global loads its fetches sat in the same in-order vmcnt queue BEHIND the
// gradient prefetches and every pixel waited for all of them (99 us per launch = 36 % of the HBM rate; 4 loads in flight, then idle).
template <typename T> struct L0Raw { typedef f32x4 type; };
template <> struct L0Raw<__bf16> { typedef l0_u32x2 type; };
template <typename T>
__device__ __forceinline__ f32x4 l0_cvt(const typename L0Raw<T>::type r) {
    if constexpr (sizeof(T) == 4) {
        return r;
    } else {
        return (f32x4){__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xffff0000u), __uint_as_float(r[1] << 16), __uint_as_float(r[1] & 0xffff0000u)};
    }
}
template <typename TZ>
__global__ __launch_bounds__(256) void l0_bwd_sums_kernel(const TZ* __restrict__ dz, const float* __restrict__ mel,
                                                          const float* __restrict__ w, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, double* __restrict__ sums, int H,
                                                          int W, int groups, float slope, int rows_per_block) {
    typedef typename L0Raw<TZ>::type raw_t;
    extern __shared__ float sMel[];  // [rows_per_block + 2][W + 2]: image rows y_beg - 1 .. , columns -1 .. W, zeros outside the image
    __shared__ double sS[L0_C * L0_NSUM];
    const int b = blockIdx.y, tid = threadIdx.x, cq = tid & 15, seg = tid >> 4;
    const int y_beg = blockIdx.x * rows_per_block, nrows = min(H, y_beg + rows_per_block) - y_beg;
    const int g = groups == 1 ? 0 : b, WP = W + 2;
    for (int i = tid; i < L0_C * L0_NSUM; i += 256) sS[i] = 0.0;
    {
        const float* img = mel + (size_t)b * H * W;
        for (int i = tid; i < (rows_per_block + 2) * WP; i += 256) {
            const int r = i / WP, xx = i - r * WP - 1, yy = y_beg - 1 + r;
            sMel[i] = ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) ? img[(size_t)yy * W + xx] : 0.f;
        }
    }
    __syncthreads();
    L0Thread t;
    l0_setup(t, w, mean, rstd, gamma, beta, g, cq);
    const int len = (W + 15) / 16, x0 = seg * len;
    const int total = nrows * len;  // pixels per thread, the same for every thread of the workgroup (columns past the row are masked)
    const TZ* gbase = dz + ((size_t)(b * H + y_beg) * W) * L0_C + 4 * cq;
    int lrow = 0, lxi = 0;  // load cursor: L0_Q pixels ahead of the compute cursor
    // The load is an asm statement TIED to the slot's register ("+v"): hipcc otherwise loads into fresh registers and copies them into
    // the slot at the loop's back-edge -- a copy that waits for the load (vmcnt(0) once per trip: measured, three formulations).  The
    // compiler does not count these loads; the matching wait is the asm below, also tied to the slot, so that every use of the slot's
    // value is ordered after it.  In-order completion: with L0_Q - 1 younger loads outstanding the slot's own load has landed.  Loads are
    // unconditional (clamped addresses), so the count is exact; other loads the compiler may add in between only make the wait stronger.
    auto issue = [&](raw_t& slot) {
        const unsigned off = (unsigned)(min(lrow, nrows - 1) * W + min(x0 + lxi, W - 1)) * (unsigned)L0_C;
        const TZ* ptr = gbase + off;
        if constexpr (sizeof(TZ) == 4) asm volatile("global_load_dwordx4 %0, %1, off" : "+v"(slot) : "v"(ptr));
        else asm volatile("global_load_dwordx2 %0, %1, off" : "+v"(slot) : "v"(ptr));
        const bool wrap = lxi + 1 == len;
        lxi = wrap ? 0 : lxi + 1;
        lrow += wrap ? 1 : 0;
    };
    // the thread's constants have LANDED before the first queue load is issued (an empty asm that "uses" them makes the compiler place its
    // wait here; otherwise it waits at their first use INSIDE the loop, with vmcnt(0), on every trip)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int k = 0; k < L0_T; ++k) asm volatile("" : "+v"(t.w[e][k]));
        asm volatile("" : "+v"(t.mu[e]), "+v"(t.rs[e]), "+v"(t.ga[e]), "+v"(t.be[e]));
    }
    raw_t q[L0_Q];
#pragma unroll
    for (int j = 0; j < L0_Q; ++j) {
        if constexpr (sizeof(TZ) == 4) q[j] = (raw_t){0.f, 0.f, 0.f, 0.f};
        else q[j] = (raw_t){0u, 0u};
        issue(q[j]);
    }
    float acc[4][L0_NSUM];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int k = 0; k < L0_NSUM; ++k) acc[e][k] = 0.f;
    int crow = 0, cxi = 0;
    for (int p = 0; p < total; p += L0_Q) {
#pragma unroll
        for (int j = 0; j < L0_Q; ++j) {
            const int x = x0 + cxi;
            const bool live = x < W && crow < nrows;
            // column x - 1 of image row y - 1.  Row AND column are clamped for the dead slots of the last trip (total % L0_Q != 0: crow == nrows):
            // un-clamped they read the LDS row behind the staged ones -- outside this workgroup's allocation, i.e. whatever a workgroup that held
            // that LDS before left there (another process's bf16 tiles on a shared GPU) -- and 0 * (garbage -> inf in yhat) is NaN, not 0:
            // the whole first block's weight gradient went NaN with every error word clean (GPUTEST_r05, tools/debug/dp_nan_hunt.py)
            const float* c = sMel + min(crow, nrows - 1) * WP + min(x, W - 1);
            float nb[L0_T];
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int e = 0; e < 3; ++e) nb[3 * d + e] = c[d * WP + e];
            const f32x4 yh = l0_yhat(t, nb);
            static_assert(L0_Q == 4, "the wait below is vmcnt(L0_Q - 1)");
            // (scheduling barriers: the asm statements may not drift above the products of the slot's old value -- hipcc then keeps the
            // old value in a second register and is back to copying)
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(3)" : "+v"(q[j]));
            f32x4 g4;
            {
                const f32x4 gz = l0_cvt<TZ>(q[j]);
#pragma unroll
                for (int e = 0; e < 4; ++e) g4[e] = live ? gz[e] * act_grad(yh[e] * t.ga[e] + t.be[e], slope) : 0.f;
            }
            asm volatile("" : "+v"(g4[0]), "+v"(g4[1]), "+v"(g4[2]), "+v"(g4[3]));  // the old value is finished HERE (no sinking below the load)
            __builtin_amdgcn_sched_barrier(0);
            issue(q[j]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gg = g4[e];
                acc[e][0] += gg;
                acc[e][1] = fmaf(gg, yh[e], acc[e][1]);
#pragma unroll
                for (int k = 0; k < L0_T; ++k) acc[e][2 + k] = fmaf(gg, nb[k], acc[e][2 + k]);
            }
            const bool wrap = cxi + 1 == len;
            cxi = wrap ? 0 : cxi + 1;
            crow += wrap ? 1 : 0;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the L0_Q loads past the end (clamped addresses) before the registers are re-used
    // the 4 segment-lanes of a wave that share a channel quad (bits 4,5 of the lane id), then LDS / global fp64 atomics
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int k = 0; k < L0_NSUM; ++k) {
            float v = acc[e][k];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if ((tid & 48) == 0) atomicAdd(&sS[(4 * cq + e) * L0_NSUM + k], (double)v);
        }
    __syncthreads();
    for (int i = tid; i < L0_C * L0_NSUM; i += 256) atomicAdd(&sums[(size_t)g * L0_C * L0_NSUM + i], sS[i]);
}

// workgroup = channel, thread = (slice j of 32, tap t): dW[c][t] += sum_groups gamma*rstd*(T - S1/n*S_t - S2/n*Q_t);
// dgamma += S2, dbeta += S1 (BN).  Groups (InstanceNorm) or batch items (BatchNorm moments) are spread over the 32 slices and
// combined in slice order.
__global__ __launch_bounds__(288) void l0_bwd_finalize_kernel(const double* __restrict__ sums, const double* __restrict__ mom,
                                                              const float* __restrict__ w, const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                              float* __restrict__ dW, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, int B, int groups, double n_per_group) {
    __shared__ double sA[32][L0_T], sB[32][L0_T];
    const int c = blockIdx.x, j = threadIdx.x / L0_T, t = threadIdx.x % L0_T;
    double wv[L0_T];
    for (int u = 0; u < L0_T; ++u) wv[u] = (double)w[c * L0_T + u];
    const double ga = gamma ? (double)gamma[c] : 1.0;
    // first / second moments of batch item b seen from tap t: S_t and sum_u w[c][u] R[u][t] (upper-triangular storage)
    auto item = [&](int b, double& S_t, double& wR) {
        const double* M = mom + (size_t)b * L0_NMOM;
        S_t += M[t];
        for (int u = 0; u < L0_T; ++u) {
            const int lo = u < t ? u : t, hi = u < t ? t : u;
            wR += wv[u] * M[L0_T + lo * L0_T - lo * (lo - 1) / 2 + (hi - lo)];
        }
    };
    auto term = [&](int g, double S_t, double wR) {
        const double mu = (double)mean[(size_t)g * L0_C + c], rs = (double)rstd[(size_t)g * L0_C + c];
        const double Q_t = rs * (wR - mu * S_t);
        const double* sg = sums + ((size_t)g * L0_C + c) * L0_NSUM;
        return ga * rs * (sg[2 + t] - sg[0] / n_per_group * S_t - sg[1] / n_per_group * Q_t);
    };
    double a = 0.0, b2 = 0.0;
    if (groups == 1) {  // BatchNorm: one group, its moments are the sum over the batch
        for (int b = j; b < B; b += 32) item(b, a, b2);
    } else {            // InstanceNorm: group g == batch item g
        for (int g = j; g < groups; g += 32) {
            double S_t = 0.0, wR = 0.0;
            item(g, S_t, wR);
            a += term(g, S_t, wR);
        }
    }
    sA[j][t] = a;
    sB[j][t] = b2;
    __syncthreads();
    if (j == 0) {
        double x = 0.0, y = 0.0;
        for (int i = 0; i < 32; ++i) x += sA[i][t], y += sB[i][t];
        const double dw = groups == 1 ? term(0, x, y) : x;
        dW[c * L0_T + t] += (float)dw;
        if (t == 0 && groups == 1) {
            const double* sg = sums + (size_t)c * L0_NSUM;
            if (dgamma) dgamma[c] += (float)sg[1];
            if (dbeta) dbeta[c] += (float)sg[0];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// moments kernel only: pixels per workgroup.  (Tried in round 4: one round of workgroups -- 8 pieces per clip instead of 9 -- 31 -> 29 us;
// 34 pieces 44 us, the 54 atomics per workgroup then dominate.  Not kept: the regrouped fp64 sums move mean / rstd by an ulp, which is
// enough to flip a LeakyReLU decision of the Conv1d stage at B = 32 against the float64 oracle -- tests/test_fullsize_gpu.py compares
// distributions without a flip allowance -- and 2 us do not pay for re-deriving those bars.)
static int l0_ppb(int HW) { return std::max(1024, std::min(4096, cdiv(HW, 8) / 256 * 256)); }

extern "C" int sdt_l0_block_fwd_t(const float* mel, const float* w, void* z, int z_dtype, double* mom, float* mean, float* rstd,
                                  const float* gamma, const float* beta, float* running_mean, float* running_var,
                                  int64_t* num_batches_tracked, int B, int H, int W, int groups, float eps, float momentum,
                                  float slope, void* stream) {
    SDT_CHECK_ARG(mel && w && z && mom && mean && rstd, "null pointer");
    SDT_CHECK_ARG(z_dtype == SDT_F32 || z_dtype == SDT_BF16, "unknown element type");
    SDT_CHECK_ARG(B > 0 && H > 0 && W > 0 && (groups == B || groups == 1), "bad dims (groups must be B or 1)");
    SDT_CHECK_ARG((int64_t)B * H * W * L0_C * 4 < (1ll << 40), "tensor too large");
    hipStream_t s = (hipStream_t)stream;
    const int HW = H * W, ppb = l0_ppb(HW);
    dim3 grid(cdiv(HW, ppb), B);
    if (HW <= L0_FEW)
        hipLaunchKernelGGL(l0_moments_kernel<true>, grid, dim3(256), 0, s, mel, mom, H, W, ppb);
    else
        hipLaunchKernelGGL(l0_moments_kernel<false>, grid, dim3(256), 0, s, mel, mom, H, W, ppb);
    const double n = groups == 1 ? (double)B * HW : (double)HW;
    hipLaunchKernelGGL(l0_finalize_kernel, dim3(cdiv(groups * L0_C, 64)), dim3(64), 0, s, mom, w, mean, rstd, running_mean,
                       running_var, num_batches_tracked, B, groups, n, eps, momentum);
    if (z_dtype == SDT_F32)
        hipLaunchKernelGGL(l0_fwd_kernel<float>, dim3(H, B), dim3(256), 0, s, mel, w, mean, rstd, gamma, beta, (float*)z, H, W, groups, slope);
    else
        hipLaunchKernelGGL(l0_fwd_kernel<__bf16>, dim3(H, B), dim3(256), 0, s, mel, w, mean, rstd, gamma, beta, (__bf16*)z, H, W, groups, slope);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
extern "C" int sdt_l0_block_fwd_f32(const float* mel, const float* w, float* z, double* mom, float* mean, float* rstd,
                                    const float* gamma, const float* beta, float* running_mean, float* running_var,
                                    int64_t* num_batches_tracked, int B, int H, int W, int groups, float eps, float momentum,
                                    float slope, void* stream) {
    return sdt_l0_block_fwd_t(mel, w, z, SDT_F32, mom, mean, rstd, gamma, beta, running_mean, running_var, num_batches_tracked, B, H, W, groups, eps,
                              momentum, slope, stream);
}

extern "C" int sdt_l0_block_bwd_t(const void* dz, int dz_dtype, const float* mel, const float* w, const float* mean, const float* rstd,
                                  const float* gamma, const float* beta, const double* mom, double* sums, float* dw,
                                  float* dgamma, float* dbeta, int B, int H, int W, int groups, float slope, void* stream) {
    SDT_CHECK_ARG(dz && mel && w && mean && rstd && mom && sums && dw, "null pointer");
    SDT_CHECK_ARG(dz_dtype == SDT_F32 || dz_dtype == SDT_BF16, "unknown element type");
    SDT_CHECK_ARG(B > 0 && H > 0 && W > 0 && (groups == B || groups == 1), "bad dims (groups must be B or 1)");
    hipStream_t s = (hipStream_t)stream;
    const int HW = H * W;
    // several image rows per workgroup: ~2 workgroups per CU keeps HBM busy while bounding the number of workgroups
    // that push their partial sums through the same global atomics
    int rpb = std::max(1, (H * B) / 1280);
    while (rpb > 1 && (size_t)(rpb + 2) * (W + 2) * 4 > 40960) --rpb;  // the workgroup's mel rows + halo live in LDS
    const size_t lds = (size_t)(rpb + 2) * (W + 2) * 4;
    SDT_CHECK_ARG(lds <= 40960, "mel image too wide for the first block's backward kernel");
    dim3 grid(cdiv(H, rpb), B);
    if (dz_dtype == SDT_F32)
        hipLaunchKernelGGL(l0_bwd_sums_kernel<float>, grid, dim3(256), lds, s, (const float*)dz, mel, w, mean, rstd, gamma, beta, sums, H, W, groups, slope, rpb);
    else
        hipLaunchKernelGGL(l0_bwd_sums_kernel<__bf16>, grid, dim3(256), lds, s, (const __bf16*)dz, mel, w, mean, rstd, gamma, beta, sums, H, W, groups, slope,
                           rpb);
    const double n = groups == 1 ? (double)B * HW : (double)HW;
    hipLaunchKernelGGL(l0_bwd_finalize_kernel, dim3(L0_C), dim3(288), 0, s, sums, mom, w, mean, rstd, gamma, dw, dgamma, dbeta, B,
                       groups, n);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
extern "C" int sdt_l0_block_bwd_f32(const float* dz, const float* mel, const float* w, const float* mean, const float* rstd,
                                    const float* gamma, const float* beta, const double* mom, double* sums, float* dw,
                                    float* dgamma, float* dbeta, int B, int H, int W, int groups, float slope, void* stream) {
    return sdt_l0_block_bwd_t(dz, SDT_F32, mel, w, mean, rstd, gamma, beta, mom, sums, dw, dgamma, dbeta, B, H, W, groups, slope, stream);
}
