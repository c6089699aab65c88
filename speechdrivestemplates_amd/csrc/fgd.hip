// The epoch-level validation metric (core/utils/fgd.py:6-64 of the reference, called from voice2pose.py:432-446): the Frechet distance
// between the pose-encoder codes of the predicted and of the ground-truth poses, without the codes leaving the device.
//   accumulate : adds the rows of one validation step to a fixed-size state: row count, shift (= the first row the state ever saw), the sums
//                of (x - shift) and the upper triangle of the sums of (x - shift)(x - shift)^T.  One workgroup, rows walked in order per
//                entry: the state after rows r0..r1 does not depend on how they were cut into calls, and the same calls give the same bits.
//   finalize   : one wave.  Merges the states of each side in index order (Chan's pairwise update of n, mean, M2; the states may have
//                different shifts: one per rank after an all-gather), takes the leading dim_used x dim_used block, and evaluates
//                  FGD = |mean_A - mean_B|^2 + tr C_A + tr C_B - 2 sum_i sqrt(max(mu_i, 0)),  mu = eig(sym(S C_B S)),  S = C_A^(1/2)
//                with two cyclic Jacobi decompositions in LDS (the eigenvalues of S C_B S are those of C_A C_B: the reference's
//                tr sqrtm(C_A C_B) without a square root of a non-symmetric matrix).  The sweeps are sdt_jacobi::sweep of jacobi.h, the
//                routine the eigen kernel of code_pca.hip / code_axes.hip runs: there is no second copy.
// Everything is float64 on values converted exactly from fp32, every operation of finalize rounded on its own (exact_f64.h; M2 and the
// products stay exactly symmetric whichever lane computes an entry).  Contract and numbers: DESIGN.md section 13.
#include "jacobi.h"

namespace {

using sdt_exact::add_rn;
using sdt_exact::div_rn;
using sdt_exact::kLd;
using sdt_exact::kMaxD;
using sdt_exact::kMaxTri;
using sdt_exact::mul_rn;
using sdt_exact::ordered_sum;
using sdt_exact::sub_rn;
using sdt_exact::tri_entry;
using sdt_exact::tri_index;
using sdt_jacobi::trace_of;

constexpr int kAccThreads = 256, kTileRows = 32;
constexpr int kTriPerThread = (kMaxTri + kAccThreads - 1) / kAccThreads;  // 9
constexpr int kMaxStates = 64;  // states per side of one finalize (one per rank)
constexpr int64_t kMaxRows = (int64_t)1 << 30;

// state, in 8-byte words: [0] rows (int64) | [1] 1 + first non-finite row, 0: none (int64) | shift (dim) | s1 (dim) | s2 (dim (dim+1) / 2)
constexpr int kHdr = 2;
inline int64_t state_words(int dim) { return kHdr + 2 * (int64_t)dim + (int64_t)dim * (dim + 1) / 2; }

// ---- accumulate ------------------------------------------------------------------------------------------------------------------------
// One workgroup.  Feature row r = x0[r, 0..d0) ++ x1[r, 0..d1).  Tiles of 32 rows go to LDS as x - shift; thread t owns the triangle
// entries t, t + 256, ... and the column t of s1, continues them from the state and adds the rows in ascending order, one fma per row.
__global__ void __launch_bounds__(kAccThreads) sdt_fgd_accumulate_kernel(const float* __restrict__ x0, int d0, const float* __restrict__ x1, int d1,
                                                                         int64_t rows, double* __restrict__ state, long long rows_seen_base) {
    __shared__ double c[kTileRows][kMaxD];
    __shared__ double s_shift[kMaxD];
    __shared__ int s_bad;  // first row of this call with a non-finite entry (rows <= 2^30)
    const int t = threadIdx.x, D = d0 + d1, T = D * (D + 1) / 2;
    long long* hdr = (long long*)state;
    double* shift = state + kHdr;
    double* s1 = shift + D;
    double* s2 = s1 + D;
    const long long n0 = hdr[0], bad0 = hdr[1];
    if (t == 0) s_bad = 0x7fffffff;
    if (t < D) {
        double s;
        if (n0 == 0) {  // the first row this state sees fixes the shift (a non-finite entry: 0, the row is recorded below)
            const float v = t < d0 ? x0[t] : x1[t - d0];
            s = isfinite(v) ? (double)v : 0.0;
            shift[t] = s;
        } else {
            s = shift[t];
        }
        s_shift[t] = s;
    }
    int ei[kTriPerThread], ej[kTriPerThread];
    double acc[kTriPerThread];
#pragma unroll
    for (int k = 0; k < kTriPerThread; ++k) {
        const int e = t + k * kAccThreads;
        ei[k] = ej[k] = 0;
        acc[k] = 0.0;
        if (e < T) {
            tri_entry(e, D, ei[k], ej[k]);
            acc[k] = s2[e];
        }
    }
    double acc1 = t < D ? s1[t] : 0.0;
    __syncthreads();
    for (int64_t base = 0; base < rows; base += kTileRows) {
        const int nr = (int)std::min<int64_t>(kTileRows, rows - base);
        for (int e = t; e < nr * D; e += kAccThreads) {
            const int r = e / D, d = e % D;
            const int64_t n = base + r;
            const float v = d < d0 ? x0[n * d0 + d] : x1[n * d1 + (d - d0)];
            if (!isfinite(v)) atomicMin(&s_bad, (int)n);  // (integer atomic in LDS: exact in any order)
            c[r][d] = sub_rn((double)v, s_shift[d]);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kTriPerThread; ++k) {
            if (t + k * kAccThreads < T) {
                double a = acc[k];
                for (int r = 0; r < nr; ++r) a = fma(c[r][ei[k]], c[r][ej[k]], a);
                acc[k] = a;
            }
        }
        if (t < D)
            for (int r = 0; r < nr; ++r) acc1 = add_rn(acc1, c[r][t]);
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kTriPerThread; ++k) {
        const int e = t + k * kAccThreads;
        if (e < T) s2[e] = acc[k];
    }
    if (t < D) s1[t] = acc1;
    if (t == 0) {  // (every thread read hdr before the first barrier)
        hdr[0] = n0 + (long long)rows;
        if (bad0 == 0 && s_bad != 0x7fffffff) hdr[1] = rows_seen_base + (long long)s_bad + 1;
    }
}

// ---- finalize ----------------------------------------------------------------------------------------------------------------------------
struct StateList {
    const double* a[kMaxStates];
    const double* b[kMaxStates];
};

// Lane k merges column k of the states p[0..ns) (dim x dim, leading D x D block): C[i*kLd + k] = covariance (ddof 1), mean[k].
// -> rows; bad = 1 + the first non-finite row of the first state that recorded one.  C is left as M2 when rows < 2.
__device__ long long merge_side(const double* const* p, int ns, int dim, int D, double* C, double* mean, long long& bad) {
    const int k = threadIdx.x;
    long long n = 0;
    bad = 0;
    double mk = 0.0;  // this lane's entry of the running mean
    for (int s = 0; s < ns; ++s) {
        const double* st = p[s];
        const long long* hdr = (const long long*)st;
        const long long ns_rows = hdr[0];
        if (bad == 0 && hdr[1] != 0) bad = hdr[1];
        if (ns_rows == 0) continue;  // (uniform: every lane reads the same word)
        const double* shift = st + kHdr;
        const double* s1 = shift + dim;
        const double* s2 = s1 + dim;
        const double fn = (double)ns_rows;
        if (n == 0) {  // the first state with rows: mean = shift + s1 / n, M2 = s2 - s1 s1^T / n
            if (k < D) {
                mk = add_rn(shift[k], div_rn(s1[k], fn));
                mean[k] = mk;
                for (int i = 0; i < D; ++i)
                    C[i * kLd + k] = sub_rn(s2[tri_index(i, k, dim)], div_rn(mul_rn(s1[i], s1[k]), fn));
            }
            n = ns_rows;
            __syncthreads();
            continue;
        }
        // Chan: delta = mean_s - mean; M2 += M2_s + delta delta^T n n_s / (n + n_s); mean += delta n_s / (n + n_s)
        const double fa = (double)n, ft = (double)(n + ns_rows);
        const double w = div_rn(mul_rn(fa, fn), ft);
        if (k < D) {
            const double dk = sub_rn(add_rn(shift[k], div_rn(s1[k], fn)), mk);
            for (int i = 0; i < D; ++i) {
                const double di = sub_rn(add_rn(shift[i], div_rn(s1[i], fn)), mean[i]);
                const double m2s = sub_rn(s2[tri_index(i, k, dim)], div_rn(mul_rn(s1[i], s1[k]), fn));
                C[i * kLd + k] = add_rn(C[i * kLd + k], add_rn(m2s, mul_rn(mul_rn(di, dk), w)));
            }
            mk = add_rn(mk, div_rn(mul_rn(dk, fn), ft));
        }
        __syncthreads();  // every lane has read the old mean
        if (k < D) mean[k] = mk;
        n += ns_rows;
        __syncthreads();
    }
    if (n >= 2 && k < D) {
        const double den = (double)(n - 1);
        for (int i = 0; i < D; ++i) C[i * kLd + k] = div_rn(C[i * kLd + k], den);
    }
    __syncthreads();
    return n;
}

// One wave, three LDS matrices (99 840 bytes of gfx950's 160 KB): P = C_A, then S, then sym(S C_B S); Q = C_B, then S C_B S; R = V^T, then C_B S.
__global__ void __launch_bounds__(kMaxD) sdt_fgd_finalize_kernel(StateList st, int num_states, int dim, int D, int max_sweeps, double rel_tol,
                                                                 double* __restrict__ out, int32_t* __restrict__ err) {
    __shared__ double P[kMaxD * kLd];
    __shared__ double Q[kMaxD * kLd];
    __shared__ double R[kMaxD * kLd];
    __shared__ double mean_a[kMaxD], mean_b[kMaxD], red[kMaxD], lam[kMaxD];
    const int k = threadIdx.x;
    const bool active = k < D;
    const double nan = __builtin_nan("");
    long long bad_a, bad_b;
    const long long n_a = merge_side(st.a, num_states, dim, D, P, mean_a, bad_a);
    const long long n_b = merge_side(st.b, num_states, dim, D, Q, mean_b, bad_b);
    int error = 0;
    if (n_a < 2 || n_b < 2) error |= 2;
    if (bad_a != 0 || bad_b != 0) error |= 4;
    double fgd = nan, gap2 = nan, tr_a = nan, tr_b = nan, tr_root = nan, off1 = nan, off2 = nan, min1 = nan, min2 = nan;
    double frob;  // (of each decomposed matrix: not reported)
    int sweeps1 = 0, sweeps2 = 0;
    if (error == 0) {  // (uniform)
        if (active) red[k] = mul_rn(sub_rn(mean_a[k], mean_b[k]), sub_rn(mean_a[k], mean_b[k]));
        __syncthreads();
        gap2 = ordered_sum(red, D);
        tr_a = trace_of(P, red, D);
        tr_b = trace_of(Q, red, D);
        // C_A = V Lambda V^T
        if (!sdt_jacobi::sweep<true>(P, R, red, D, max_sweeps, rel_tol, sweeps1, off1, frob)) error |= 1;
        __syncthreads();
        if (active) red[k] = P[k * kLd + k];
        __syncthreads();
        min1 = red[0];
        for (int i = 1; i < D; ++i) min1 = fmin(min1, red[i]);
        if (active) lam[k] = sqrt(fmax(red[k], 0.0));
        __syncthreads();
        // S = V sqrt(max(Lambda, 0)) V^T -> P (lane j: column j; R[m][i] is a broadcast read).  The sum over m is in the same order for
        // (i, j) and (j, i) and the products commute: S is symmetric to the bit.
        if (active)
            for (int i = 0; i < D; ++i) {
                double s = 0.0;
                for (int m = 0; m < D; ++m) s = add_rn(s, mul_rn(mul_rn(R[m * kLd + i], R[m * kLd + k]), lam[m]));
                P[i * kLd + k] = s;
            }
        __syncthreads();
        // C_B S -> R, then S (C_B S) -> Q
        if (active)
            for (int i = 0; i < D; ++i) {
                double s = 0.0;
                for (int m = 0; m < D; ++m) s = add_rn(s, mul_rn(Q[i * kLd + m], P[m * kLd + k]));
                R[i * kLd + k] = s;
            }
        __syncthreads();
        if (active)
            for (int i = 0; i < D; ++i) {
                double s = 0.0;
                for (int m = 0; m < D; ++m) s = add_rn(s, mul_rn(P[i * kLd + m], R[m * kLd + k]));
                Q[i * kLd + k] = s;
            }
        __syncthreads();
        // sym(.) -> P
        if (active)
            for (int i = 0; i < D; ++i) P[i * kLd + k] = mul_rn(0.5, add_rn(Q[i * kLd + k], Q[k * kLd + i]));
        if (!sdt_jacobi::sweep<false>(P, R, red, D, max_sweeps, rel_tol, sweeps2, off2, frob)) error |= 1;  // (begins with a barrier)
        __syncthreads();
        if (active) red[k] = P[k * kLd + k];
        __syncthreads();
        min2 = red[0];
        for (int i = 1; i < D; ++i) min2 = fmin(min2, red[i]);
        __syncthreads();
        if (active) red[k] = sqrt(fmax(red[k], 0.0));
        __syncthreads();
        tr_root = ordered_sum(red, D);
        fgd = sub_rn(add_rn(add_rn(gap2, tr_a), tr_b), mul_rn(2.0, tr_root));  // (kept with error bit 0: the caller decides)
    }
    if (k == 0) {
        out[0] = fgd;
        out[1] = gap2;
        out[2] = tr_a;
        out[3] = tr_b;
        out[4] = tr_root;
        out[5] = (double)n_a;
        out[6] = (double)n_b;
        out[7] = (double)sweeps1;
        out[8] = off1;
        out[9] = (double)sweeps2;
        out[10] = off2;
        out[11] = min1;
        out[12] = min2;
        out[13] = (double)(bad_a - 1);
        out[14] = (double)(bad_b - 1);
        out[15] = 0.0;
        err[0] = error;
    }
}

}  // namespace

extern "C" int64_t sdt_fgd_state_bytes(int dim) {
    if (dim < 2 || dim > kMaxD) return 0;
    return state_words(dim) * 8;
}

extern "C" int sdt_fgd_accumulate(const float* x0, int d0, const float* x1, int d1, int64_t rows, void* state, int64_t state_bytes,
                                  int64_t rows_seen_base, void* stream) {
    SDT_CHECK_ARG(d0 >= 1 && d1 >= 0 && d0 <= kMaxD && d1 <= kMaxD, "d0 must lie in [1, 64] and d1 in [0, 64]");
    SDT_CHECK_ARG(d0 + d1 >= 2 && d0 + d1 <= kMaxD, "dim = d0 + d1 must lie in [2, 64]");
    SDT_CHECK_ARG(x0 != nullptr && state != nullptr, "null pointer");
    SDT_CHECK_ARG((x1 != nullptr) == (d1 > 0), "x1 must be NULL exactly when d1 is 0");
    SDT_CHECK_ARG(rows >= 1 && rows <= kMaxRows, "rows must lie in [1, 2^30]");
    SDT_CHECK_ARG(rows_seen_base >= 0, "rows_seen_base must not be negative");
    SDT_CHECK_ARG(state_bytes >= sdt_fgd_state_bytes(d0 + d1), "state too small");
    SDT_CHECK_ARG(((uintptr_t)state & 7) == 0, "state must be 8-byte aligned");
    hipLaunchKernelGGL(sdt_fgd_accumulate_kernel, dim3(1), dim3(kAccThreads), 0, (hipStream_t)stream, x0, d0, x1, d1, rows, (double*)state,
                       (long long)rows_seen_base);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_fgd_finalize(const void* const* states_a, const void* const* states_b, int num_states, int dim, int dim_used, int max_sweeps,
                                double rel_tol, double* out, int32_t* err, void* stream) {
    SDT_CHECK_ARG(dim >= 2 && dim <= kMaxD, "dim must lie in [2, 64]");
    SDT_CHECK_ARG(dim_used >= 2 && dim_used <= dim, "dim_used must lie in [2, dim]");
    SDT_CHECK_ARG(num_states >= 1 && num_states <= kMaxStates, "num_states must lie in [1, 64]");
    SDT_CHECK_ARG(states_a != nullptr && states_b != nullptr && out != nullptr && err != nullptr, "null pointer");
    SDT_CHECK_ARG(max_sweeps >= 1 && max_sweeps <= 1000, "max_sweeps must lie in [1, 1000]");
    SDT_CHECK_ARG(rel_tol >= 0.0, "rel_tol must not be negative");
    StateList st;
    for (int i = 0; i < kMaxStates; ++i) {
        const bool used = i < num_states;
        SDT_CHECK_ARG(!used || (states_a[i] != nullptr && states_b[i] != nullptr), "null state pointer");
        SDT_CHECK_ARG(!used || ((((uintptr_t)states_a[i]) | ((uintptr_t)states_b[i])) & 7) == 0, "states must be 8-byte aligned");
        st.a[i] = used ? (const double*)states_a[i] : nullptr;
        st.b[i] = used ? (const double*)states_b[i] : nullptr;
    }
    hipLaunchKernelGGL(sdt_fgd_finalize_kernel, dim3(1), dim3(kMaxD), 0, (hipStream_t)stream, st, num_states, dim, dim_used, max_sweeps, rel_tol,
                       out, err);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
