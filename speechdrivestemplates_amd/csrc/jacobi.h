// Device code shared by code_pca.hip (two components, the epoch figure) and code_axes.hip (all components): float64 operations each
// rounded on its own, and the one-wave cyclic Jacobi of a D x D covariance, 2 <= D <= 64, with the ranking and the sign rule.
// Both kernels run the same statements, so the eigenpairs they have in common carry the same bits.
#pragma once
#include "common.h"

namespace sdt_jacobi {

constexpr int kMaxD = 64;
constexpr int kLd = kMaxD + 1;  // pitch of the Jacobi matrix in LDS: the mirror writes A[k][p] of 64 lanes fall on different banks

// float64 operations each rounded on its own (see speaker_stats.hip: HIP's own *_rn are plain operators under the default -ffp-contract)
__device__ __forceinline__ double add_rn(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ double sub_rn(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ double mul_rn(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double div_rn(double a, double b) {
#pragma clang fp contract(off)
    return a / b;
}

// sum of red[0..D) in index order, the same value in every lane
__device__ __forceinline__ double ordered_sum(const double* red, int D) {
    double s = 0.0;
    for (int i = 0; i < D; ++i) s = add_rn(s, red[i]);
    return s;
}

// One wave of kMaxD lanes (the whole workgroup).  Lane k owns column k of the symmetric matrix A (kept whole: rows p and q are read along
// k, the mirror entries are written back) and column k of V^T.  Row-cyclic sweeps over the pairs p < q; a rotation (Rutishauser's
// formulas) zeroes A[p][q]:
//   theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c.
// Before each sweep: off = sqrt(sum of squared off-diagonal entries); stop when off <= rel_tol * ||C||_F, error bit 0 if max_sweeps
// sweeps did not get there (NaN never compares true, so a non-finite matrix ends the same way); bit 1: trace(C) is not positive.
// info = [sweeps done, final off, ||C||_F, trace(C)].  evals (D) are ranked in descending order (ties: the lower column first); the
// n_comps leading eigenvectors go to comps (n_comps, D), each signed so that its entry of largest magnitude (first of equals) is positive.
__device__ __forceinline__ void eigh_one_wave(const double* __restrict__ cov, int D, int max_sweeps, double rel_tol, int n_comps,
                                              double* __restrict__ evals, double* __restrict__ comps, double* __restrict__ info,
                                              int32_t* __restrict__ err) {
    __shared__ double A[kMaxD * kLd];
    __shared__ double Vt[kMaxD * kMaxD];
    __shared__ double red[kMaxD];
    const int k = threadIdx.x;
    const bool active = k < D;
    if (active)
        for (int i = 0; i < D; ++i) {
            A[i * kLd + k] = cov[i * D + k];
            Vt[i * kMaxD + k] = i == k ? 1.0 : 0.0;
        }
    __syncthreads();
    if (active) {
        double s = 0.0;
        for (int i = 0; i < D; ++i) s = add_rn(s, mul_rn(A[i * kLd + k], A[i * kLd + k]));
        red[k] = s;
    }
    __syncthreads();
    const double frob = sqrt(ordered_sum(red, D));
    __syncthreads();
    if (active) red[k] = A[k * kLd + k];
    __syncthreads();
    const double trace = ordered_sum(red, D);
    const double tol = mul_rn(rel_tol, frob);

    int sweeps = 0, error = 0;
    double off = 0.0;
    for (;;) {
        __syncthreads();
        if (active) {
            double s = 0.0;
            for (int i = 0; i < D; ++i)
                if (i != k) s = add_rn(s, mul_rn(A[i * kLd + k], A[i * kLd + k]));
            red[k] = s;
        }
        __syncthreads();
        off = sqrt(ordered_sum(red, D));
        if (off <= tol) break;
        if (sweeps == max_sweeps) {
            error |= 1;
            break;
        }
        for (int p = 0; p < D - 1; ++p)
            for (int q = p + 1; q < D; ++q) {
                const double apq = A[p * kLd + q];  // the same address in every lane: a broadcast read
                if (apq == 0.0) continue;            // (uniform)
                const double app = A[p * kLd + p], aqq = A[q * kLd + q];
                const double theta = div_rn(sub_rn(aqq, app), mul_rn(2.0, apq));
                const double t = div_rn(copysign(1.0, theta), add_rn(fabs(theta), sqrt(add_rn(mul_rn(theta, theta), 1.0))));
                const double c = div_rn(1.0, sqrt(add_rn(mul_rn(t, t), 1.0)));
                const double s = mul_rn(t, c);
                double akp = 0.0, akq = 0.0, vp = 0.0, vq = 0.0;
                if (active) {
                    akp = A[p * kLd + k];
                    akq = A[q * kLd + k];
                    vp = Vt[p * kMaxD + k];
                    vq = Vt[q * kMaxD + k];
                }
                __syncthreads();  // every lane has read a_pp, a_qq, a_pq before lanes p and q overwrite them
                if (active) {
                    if (k == p) {
                        A[p * kLd + p] = sub_rn(app, mul_rn(t, apq));
                        A[p * kLd + q] = 0.0;
                    } else if (k == q) {
                        A[q * kLd + q] = add_rn(aqq, mul_rn(t, apq));
                        A[q * kLd + p] = 0.0;
                    } else {
                        const double np = sub_rn(mul_rn(c, akp), mul_rn(s, akq)), nq = add_rn(mul_rn(s, akp), mul_rn(c, akq));
                        A[p * kLd + k] = np;
                        A[q * kLd + k] = nq;
                        A[k * kLd + p] = np;
                        A[k * kLd + q] = nq;
                    }
                    Vt[p * kMaxD + k] = sub_rn(mul_rn(c, vp), mul_rn(s, vq));
                    Vt[q * kMaxD + k] = add_rn(mul_rn(s, vp), mul_rn(c, vq));
                }
                __syncthreads();
            }
        ++sweeps;
    }
    if (!(trace > 0.0)) error |= 2;

    // rank of eigenvalue k in descending order (ties: the lower index first)
    __syncthreads();
    if (active) red[k] = A[k * kLd + k];
    __syncthreads();
    if (active) {
        const double lam = red[k];
        int rank = 0;
        for (int j = 0; j < D; ++j) {
            const double lj = red[j];
            if (lj > lam || (lj == lam && j < k)) ++rank;
        }
        if (lam != lam) rank = k;  // NaN (error bit 0 is set): keep the writes inside the buffers
        evals[rank] = lam;
        if (rank < n_comps) {  // eigenvector k = row k of V^T; its entry of largest magnitude (first of equals) is made positive
            double big = -1.0, sign = 1.0;
            for (int i = 0; i < D; ++i) {
                const double v = Vt[k * kMaxD + i];
                if (fabs(v) > big) {
                    big = fabs(v);
                    sign = v < 0.0 ? -1.0 : 1.0;
                }
            }
            for (int i = 0; i < D; ++i) comps[rank * D + i] = mul_rn(sign, Vt[k * kMaxD + i]);
        }
    }
    if (k == 0) {
        info[0] = (double)sweeps;
        info[1] = off;
        info[2] = frob;
        info[3] = trace;
        err[0] = error;
    }
}

}  // namespace sdt_jacobi
