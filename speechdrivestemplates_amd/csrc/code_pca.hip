// The per-epoch clip-code figure (Voice2Pose.draw_figure_epoch, core/pipelines/voice2pose.py:479-510, and Pose2Pose.draw_figure_epoch,
// pose2pose.py:314-345, of the reference): a 2-component PCA of the (N, D) code table and a scatter plot of the projection, without
// the table leaving the device.  Four stages, nine small kernels:
//   moments : column sums (partials per workgroup, ordered final reduce) -> mean; centred products of 16-row tiles staged in LDS
//             (partials per workgroup, ordered final reduce) -> covariance.  Fixed grid, no floating-point atomics: deterministic.
//   eigh    : cyclic Jacobi on the D x D covariance in LDS, one wave (jacobi.h: the sweeps that fgd.hip runs too); eigenvalues ranked,
//             the leading components with the sign rule.  The one kernel serves sdt_code_pca_eigh (two components) and
//             sdt_code_axes_eigh (all of them, code_axes.hip).
//   project : X = (x - mean) . comp^T, per-workgroup min / max, then one workgroup reduces them and derives the axis limits.
//   raster  : uint32 counters per plot pixel (integer atomics: exact in any order), then counter -> colour table -> uint8 RGB.
// Everything is float64 on values converted exactly from fp32.  The binning rounds every operation on its own (exact_f64.h):
// the tests recompute it with numpy from the returned coordinates and expect the same bins.  Contract and numbers: DESIGN.md section 12.
#include "jacobi.h"

namespace {

using sdt_exact::add_rn;
using sdt_exact::div_rn;
using sdt_exact::kMaxD;
using sdt_exact::kMaxTri;
using sdt_exact::mul_rn;
using sdt_exact::sub_rn;
using sdt_exact::tri_entry;

constexpr int kThreads = 256, kTileRows = 16, kMaxGrid = 256;
constexpr int kTriPerThread = (kMaxTri + kThreads - 1) / kThreads;  // 9
constexpr int64_t kMaxRows = (int64_t)1 << 30;

inline int moments_grid(int64_t n_rows) { return (int)std::min<int64_t>(kMaxGrid, (n_rows + kTileRows - 1) / kTileRows); }

// smallest power of two >= D (2 <= D <= 64): the column lanes of one row in the column-sum kernel
inline int pad_pow2(int D) {
    int p = 2;
    while (p < D) p <<= 1;
    return p;
}

// ---- moments ---------------------------------------------------------------------------------------------------------------------------
// thread (r, d) = (t / dpad, t % dpad) adds column d of rows b*R + r, + G*R, ... in ascending order; the R row lanes of a column are
// then added in order r = 0..R-1.  sums[b*64 + d], bad[b] = 1 + first row of this workgroup with a non-finite entry (0: none).
__global__ void __launch_bounds__(kThreads) sdt_code_pca_colsum_kernel(const float* __restrict__ x, int64_t N, int D, int dpad,
                                                                       double* __restrict__ sums, long long* __restrict__ bad) {
    __shared__ double s_acc[kThreads];
    __shared__ long long s_bad[kThreads];
    const int t = threadIdx.x, R = kThreads / dpad, r = t / dpad, d = t % dpad;
    double acc = 0.0;
    long long b = 0;
    if (d < D)
        for (int64_t n = (int64_t)blockIdx.x * R + r; n < N; n += (int64_t)gridDim.x * R) {
            const float v = x[n * D + d];
            if (b == 0 && !isfinite(v)) b = n + 1;
            acc = add_rn(acc, (double)v);
        }
    s_acc[t] = acc;
    s_bad[t] = b;
    __syncthreads();
    if (t < D) {
        double s = 0.0;
        for (int rr = 0; rr < R; ++rr) s = add_rn(s, s_acc[rr * dpad + t]);
        sums[(int64_t)blockIdx.x * kMaxD + t] = s;
    }
    if (t == 0) {
        long long m = 0;
        for (int i = 0; i < kThreads; ++i) {
            const long long v = s_bad[i];
            if (v != 0 && (m == 0 || v < m)) m = v;
        }
        bad[blockIdx.x] = m;
    }
}

// one workgroup: mean[d] = (sum of the G partials in workgroup order) / N; first_bad = the smallest non-zero bad[b]
__global__ void __launch_bounds__(kMaxD) sdt_code_pca_mean_kernel(const double* __restrict__ sums, const long long* __restrict__ bad, int G,
                                                                  int64_t N, int D, double* __restrict__ mean,
                                                                  long long* __restrict__ first_bad) {
    const int d = threadIdx.x;
    if (d < D) {
        double s = 0.0;
        for (int b = 0; b < G; ++b) s = add_rn(s, sums[(int64_t)b * kMaxD + d]);
        mean[d] = div_rn(s, (double)N);
    }
    if (d == 0) {
        long long m = 0;
        for (int b = 0; b < G; ++b) {
            const long long v = bad[b];
            if (v != 0 && (m == 0 || v < m)) m = v;
        }
        first_bad[0] = m;
    }
}

// workgroup b takes the 16-row tiles b, b + G, ...: the centred rows go to LDS, thread t owns the triangle entries t, t + 256, ...
// and adds (x[n,i] - mean[i]) * (x[n,j] - mean[j]) row by row.  prods[b*2080 + e].
__global__ void __launch_bounds__(kThreads) sdt_code_pca_cov_kernel(const float* __restrict__ x, int64_t N, int D, const double* __restrict__ mean,
                                                                    double* __restrict__ prods) {
    __shared__ double c[kTileRows][kMaxD];
    __shared__ double s_mean[kMaxD];
    const int t = threadIdx.x, T = D * (D + 1) / 2;
    if (t < D) s_mean[t] = mean[t];
    int ei[kTriPerThread], ej[kTriPerThread];
    double acc[kTriPerThread];
#pragma unroll
    for (int k = 0; k < kTriPerThread; ++k) {
        const int e = t + k * kThreads;
        ei[k] = ej[k] = 0;
        if (e < T) tri_entry(e, D, ei[k], ej[k]);
        acc[k] = 0.0;
    }
    __syncthreads();
    const int64_t tiles = (N + kTileRows - 1) / kTileRows;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        for (int e = t; e < kTileRows * D; e += kThreads) {
            const int r = e / D, d = e % D;
            const int64_t n = tile * kTileRows + r;
            c[r][d] = n < N ? sub_rn((double)x[n * D + d], s_mean[d]) : 0.0;  // a row past the end adds +0.0: no change
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kTriPerThread; ++k) {
            if (t + k * kThreads < T) {
                double a = acc[k];
                for (int r = 0; r < kTileRows; ++r) a = add_rn(a, mul_rn(c[r][ei[k]], c[r][ej[k]]));
                acc[k] = a;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kTriPerThread; ++k) {
        const int e = t + k * kThreads;
        if (e < T) prods[(int64_t)blockIdx.x * kMaxTri + e] = acc[k];
    }
}

// cov[i,j] = cov[j,i] = (sum of the G partials in workgroup order) / (N - 1)
__global__ void __launch_bounds__(kThreads) sdt_code_pca_cov_final_kernel(const double* __restrict__ prods, int G, int64_t N, int D,
                                                                          double* __restrict__ cov) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= D * (D + 1) / 2) return;
    double s = 0.0;
    for (int b = 0; b < G; ++b) s = add_rn(s, prods[(int64_t)b * kMaxTri + e]);
    s = div_rn(s, (double)(N - 1));
    int i, j;
    tri_entry(e, D, i, j);
    cov[i * D + j] = s;
    cov[j * D + i] = s;
}

// ---- eigen-decomposition -----------------------------------------------------------------------------------------------------------------
// One wave: the cyclic Jacobi, the ranking and the sign rule of jacobi.h, the n_comps leading components kept.
__global__ void __launch_bounds__(kMaxD) sdt_code_eigh_kernel(const double* __restrict__ cov, int D, int max_sweeps, double rel_tol, int n_comps,
                                                              double* __restrict__ evals, double* __restrict__ comps,
                                                              double* __restrict__ info, int32_t* __restrict__ err) {
    sdt_jacobi::eigh_one_wave(cov, D, max_sweeps, rel_tol, n_comps, evals, comps, info, err);
}

// ---- projection --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// min / max of the four values of every lane of the workgroup -> out[0..4) = min0, max0, min1, max1 (thread 0 writes)
__device__ __forceinline__ void block_minmax(double mn0, double mx0, double mn1, double mx1, double* out) {
    __shared__ double s_mm[kThreads / 64][4];
    const int w = threadIdx.x / 64;
    mn0 = wave_min_d(mn0);
    mx0 = wave_max_d(mx0);
    mn1 = wave_min_d(mn1);
    mx1 = wave_max_d(mx1);
    if (threadIdx.x % 64 == 0) {
        s_mm[w][0] = mn0;
        s_mm[w][1] = mx0;
        s_mm[w][2] = mn1;
        s_mm[w][3] = mx1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < kThreads / 64; ++i) {
            mn0 = fmin(mn0, s_mm[i][0]);
            mx0 = fmax(mx0, s_mm[i][1]);
            mn1 = fmin(mn1, s_mm[i][2]);
            mx1 = fmax(mx1, s_mm[i][3]);
        }
        out[0] = mn0;
        out[1] = mx0;
        out[2] = mn1;
        out[3] = mx1;
    }
}

// thread n: X[n,k] = sum over d ascending of (x[n,d] - mean[d]) * comp[k,d]; mm[b*4..] = this workgroup's min / max of both axes
__global__ void __launch_bounds__(kThreads) sdt_code_pca_project_kernel(const float* __restrict__ x, int64_t N, int D,
                                                                        const double* __restrict__ mean, const double* __restrict__ comps,
                                                                        double* __restrict__ X, double* __restrict__ mm) {
    __shared__ double s_mean[kMaxD], s_c0[kMaxD], s_c1[kMaxD];
    if (threadIdx.x < D) {
        s_mean[threadIdx.x] = mean[threadIdx.x];
        s_c0[threadIdx.x] = comps[threadIdx.x];
        s_c1[threadIdx.x] = comps[D + threadIdx.x];
    }
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const double inf = __builtin_huge_val();
    double x0 = 0.0, x1 = 0.0, mn0 = inf, mx0 = -inf, mn1 = inf, mx1 = -inf;
    if (n < N) {
        const float* row = x + n * D;
        for (int d = 0; d < D; ++d) {
            const double c = sub_rn((double)row[d], s_mean[d]);
            x0 = add_rn(x0, mul_rn(c, s_c0[d]));
            x1 = add_rn(x1, mul_rn(c, s_c1[d]));
        }
        X[2 * n] = x0;
        X[2 * n + 1] = x1;
        mn0 = mx0 = x0;
        mn1 = mx1 = x1;
    }
    block_minmax(mn0, mx0, mn1, mx1, mm + (int64_t)blockIdx.x * 4);
}

// one workgroup: limits[0..4) = min0, max0, min1, max1 over the PB partials; limits[4..8) = lo0, hi0, lo1, hi1, matplotlib's default
// margins: lo = min - 0.05 (max - min), hi = max + 0.05 (max - min); an axis without extent (hi <= lo) becomes [min - 0.5, max + 0.5]
__global__ void __launch_bounds__(kThreads) sdt_code_pca_limits_kernel(const double* __restrict__ mm, int PB, double* __restrict__ limits) {
    const double inf = __builtin_huge_val();
    double mn0 = inf, mx0 = -inf, mn1 = inf, mx1 = -inf;
    for (int b = threadIdx.x; b < PB; b += kThreads) {
        mn0 = fmin(mn0, mm[(int64_t)b * 4]);
        mx0 = fmax(mx0, mm[(int64_t)b * 4 + 1]);
        mn1 = fmin(mn1, mm[(int64_t)b * 4 + 2]);
        mx1 = fmax(mx1, mm[(int64_t)b * 4 + 3]);
    }
    __shared__ double s_out[4];
    block_minmax(mn0, mx0, mn1, mx1, s_out);
    if (threadIdx.x != 0) return;
    for (int a = 0; a < 2; ++a) {
        const double mn = s_out[2 * a], mx = s_out[2 * a + 1];
        const double pad = mul_rn(0.05, sub_rn(mx, mn));
        double lo = sub_rn(mn, pad), hi = add_rn(mx, pad);
        if (!(hi > lo)) {
            lo = sub_rn(mn, 0.5);
            hi = add_rn(mx, 0.5);
        }
        limits[2 * a] = mn;
        limits[2 * a + 1] = mx;
        limits[4 + 2 * a] = lo;
        limits[4 + 2 * a + 1] = hi;
    }
}

// ---- raster ------------------------------------------------------------------------------------------------------------------------------
// thread n: bin of point n = min(int(floor((X - lo) * (P / (hi - lo)))), P - 1) per axis, every operation rounded on its own; the row is
// flipped (y up).  The marker covers columns [col - (m-1)/2, col - (m-1)/2 + m) and the same rows, clipped to the plot rectangle.
// A point outside [lo, hi] on either axis, or not finite, is not drawn.
__global__ void __launch_bounds__(kThreads) sdt_code_pca_count_kernel(const double* __restrict__ X, int64_t N, const double* __restrict__ lim,
                                                                      int Pw, int Ph, int marker, uint32_t* __restrict__ counts) {
    const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    const double lo0 = lim[0], hi0 = lim[1], lo1 = lim[2], hi1 = lim[3];
    const double x0 = X[2 * n], x1 = X[2 * n + 1];
    if (!(x0 >= lo0 && x0 <= hi0 && x1 >= lo1 && x1 <= hi1)) return;
    const double sx = div_rn((double)Pw, sub_rn(hi0, lo0)), sy = div_rn((double)Ph, sub_rn(hi1, lo1));
    const double fx = floor(mul_rn(sub_rn(x0, lo0), sx)), fy = floor(mul_rn(sub_rn(x1, lo1), sy));
    const int col = fx >= (double)Pw ? Pw - 1 : (int)fx;
    const int row = Ph - 1 - (fy >= (double)Ph ? Ph - 1 : (int)fy);
    const int c0 = col - (marker - 1) / 2, r0 = row - (marker - 1) / 2;
    for (int dy = 0; dy < marker; ++dy)
        for (int dx = 0; dx < marker; ++dx) {
            const int cc = c0 + dx, rr = r0 + dy;
            if (cc >= 0 && cc < Pw && rr >= 0 && rr < Ph) atomicAdd(&counts[(int64_t)rr * Pw + cc], 1u);
        }
}

// thread per canvas pixel: inside the plot rectangle table[min(count, table_len - 1)], on the 1-pixel ring around it black, else white
__global__ void __launch_bounds__(kThreads) sdt_code_pca_colourise_kernel(const uint32_t* __restrict__ counts, const uint8_t* __restrict__ table,
                                                                          int table_len, int H, int W, int margin, int Pw, int Ph,
                                                                          uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const int py = (int)(i / W) - margin, px = (int)(i % W) - margin;
    uint8_t r = 255, g = 255, b = 255;
    if (px >= 0 && px < Pw && py >= 0 && py < Ph) {
        const uint32_t k = std::min<uint32_t>(counts[(int64_t)py * Pw + px], (uint32_t)(table_len - 1));
        r = table[3 * k];
        g = table[3 * k + 1];
        b = table[3 * k + 2];
    } else if (px >= -1 && px <= Pw && py >= -1 && py <= Ph) {
        r = g = b = 0;
    }
    out[3 * i] = r;
    out[3 * i + 1] = g;
    out[3 * i + 2] = b;
}

// workspace, in 8-byte words: G*64 column-sum partials | G*2080 product partials | G bad-row words | 4 min / max words per 256 rows
inline int64_t ws_words(int64_t N) {
    const int64_t G = moments_grid(N);
    return G * (kMaxD + kMaxTri + 1) + 4 * cdiv64(N, kThreads);
}

}  // namespace

void sdt_jacobi::launch_eigh(const double* cov, int dim, int max_sweeps, double rel_tol, int n_comps, double* evals, double* comps, double* info,
                             int32_t* err, void* stream) {
    hipLaunchKernelGGL(sdt_code_eigh_kernel, dim3(1), dim3(kMaxD), 0, (hipStream_t)stream, cov, dim, max_sweeps, rel_tol, n_comps, evals, comps,
                       info, err);
}

extern "C" int64_t sdt_code_pca_workspace_bytes(int64_t n_rows, int dim) {
    if (n_rows < 2 || n_rows > kMaxRows || dim < 2 || dim > kMaxD) return 0;
    return ws_words(n_rows) * 8;
}

extern "C" int sdt_code_pca_moments(const float* x, int64_t n_rows, int dim, void* workspace, int64_t workspace_bytes, double* mean,
                                    double* cov, int64_t* first_bad_row, void* stream) {
    SDT_CHECK_ARG(x != nullptr && workspace != nullptr && mean != nullptr && cov != nullptr && first_bad_row != nullptr, "null pointer");
    SDT_CHECK_ARG(n_rows >= 2 && n_rows <= kMaxRows, "n_rows must lie in [2, 2^30]");
    SDT_CHECK_ARG(dim >= 2 && dim <= kMaxD, "dim must lie in [2, 64]");
    SDT_CHECK_ARG(workspace_bytes >= sdt_code_pca_workspace_bytes(n_rows, dim), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int G = moments_grid(n_rows);
    double* sums = (double*)workspace;
    double* prods = sums + (int64_t)G * kMaxD;
    long long* bad = (long long*)(prods + (int64_t)G * kMaxTri);
    hipLaunchKernelGGL(sdt_code_pca_colsum_kernel, dim3(G), dim3(kThreads), 0, st, x, n_rows, dim, pad_pow2(dim), sums, bad);
    hipLaunchKernelGGL(sdt_code_pca_mean_kernel, dim3(1), dim3(kMaxD), 0, st, sums, bad, G, n_rows, dim, mean, (long long*)first_bad_row);
    hipLaunchKernelGGL(sdt_code_pca_cov_kernel, dim3(G), dim3(kThreads), 0, st, x, n_rows, dim, mean, prods);
    hipLaunchKernelGGL(sdt_code_pca_cov_final_kernel, dim3(cdiv(dim * (dim + 1) / 2, kThreads)), dim3(kThreads), 0, st, prods, G, n_rows, dim,
                       cov);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_code_pca_eigh(const double* cov, int dim, int max_sweeps, double rel_tol, double* evals, double* comps, double* info,
                                 int32_t* err, void* stream) {
    SDT_CHECK_ARG(cov != nullptr && evals != nullptr && comps != nullptr && info != nullptr && err != nullptr, "null pointer");
    SDT_CHECK_ARG(dim >= 2 && dim <= kMaxD, "dim must lie in [2, 64]");
    SDT_CHECK_ARG(max_sweeps >= 1 && max_sweeps <= 1000, "max_sweeps must lie in [1, 1000]");
    SDT_CHECK_ARG(rel_tol >= 0.0, "rel_tol must not be negative");
    sdt_jacobi::launch_eigh(cov, dim, max_sweeps, rel_tol, 2, evals, comps, info, err, stream);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_code_pca_project(const float* x, int64_t n_rows, int dim, const double* mean, const double* comps, double* X,
                                    void* workspace, int64_t workspace_bytes, double* limits, void* stream) {
    SDT_CHECK_ARG(x != nullptr && mean != nullptr && comps != nullptr && X != nullptr && workspace != nullptr && limits != nullptr,
                  "null pointer");
    SDT_CHECK_ARG(n_rows >= 2 && n_rows <= kMaxRows, "n_rows must lie in [2, 2^30]");
    SDT_CHECK_ARG(dim >= 2 && dim <= kMaxD, "dim must lie in [2, 64]");
    SDT_CHECK_ARG(workspace_bytes >= sdt_code_pca_workspace_bytes(n_rows, dim), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int PB = (int)cdiv64(n_rows, kThreads);
    double* mm = (double*)workspace + (int64_t)moments_grid(n_rows) * (kMaxD + kMaxTri + 1);
    hipLaunchKernelGGL(sdt_code_pca_project_kernel, dim3(PB), dim3(kThreads), 0, st, x, n_rows, dim, mean, comps, X, mm);
    hipLaunchKernelGGL(sdt_code_pca_limits_kernel, dim3(1), dim3(kThreads), 0, st, mm, PB, limits);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_code_pca_raster(const double* X, int64_t n_rows, const double* axis_limits, const uint8_t* table, int table_len, int H,
                                   int W, int margin, int marker_px, uint32_t* counts, int64_t counts_elems, uint8_t* out,
                                   int64_t out_bytes, void* stream) {
    SDT_CHECK_ARG(X != nullptr && axis_limits != nullptr && table != nullptr && counts != nullptr && out != nullptr, "null pointer");
    SDT_CHECK_ARG(n_rows >= 1 && n_rows <= kMaxRows, "n_rows must lie in [1, 2^30]");
    SDT_CHECK_ARG(table_len >= 1 && table_len <= (1 << 20), "table_len must lie in [1, 2^20]");
    SDT_CHECK_ARG(H > 0 && W > 0 && H <= 16384 && W <= 16384, "canvas must lie in [1, 16384] x [1, 16384]");
    SDT_CHECK_ARG(margin >= 1 && W - 2 * margin >= 1 && H - 2 * margin >= 1, "margin leaves no plot rectangle");
    SDT_CHECK_ARG(marker_px >= 1 && marker_px <= 64, "marker_px must lie in [1, 64]");
    const int Pw = W - 2 * margin, Ph = H - 2 * margin;
    SDT_CHECK_ARG(counts_elems >= (int64_t)Pw * Ph, "count buffer too small");
    SDT_CHECK_ARG(out_bytes >= (int64_t)H * W * 3, "output buffer too small");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sdt_code_pca_count_kernel, dim3((unsigned)cdiv64(n_rows, kThreads)), dim3(kThreads), 0, st, X, n_rows, axis_limits, Pw,
                       Ph, marker_px, counts);
    hipLaunchKernelGGL(sdt_code_pca_colourise_kernel, dim3((unsigned)cdiv64((int64_t)H * W, kThreads)), dim3(kThreads), 0, st, counts, table,
                       table_len, H, W, margin, Pw, Ph, out);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
