// The one-wave cyclic Jacobi of a symmetric D x D float64 matrix in LDS, 2 <= D <= 64, every operation rounded on its own.  There is one
// copy of the sweeps: the eigen kernel behind sdt_code_pca_eigh / sdt_code_axes_eigh (code_pca.hip; ranking and sign rule below) and both
// decompositions of sdt_fgd_finalize (fgd.hip) run these statements, so equal matrices give equal bits whoever asks.
#pragma once
#include "exact_f64.h"

namespace sdt_jacobi {

using sdt_exact::add_rn;
using sdt_exact::div_rn;
using sdt_exact::kLd;
using sdt_exact::kMaxD;
using sdt_exact::mul_rn;
using sdt_exact::ordered_sum;
using sdt_exact::sub_rn;

// trace of the D x D matrix M (pitch kLd), diagonal added in index order; the same value in every lane
__device__ __forceinline__ double trace_of(const double* M, double* red, int D) {
    const int k = threadIdx.x;
    __syncthreads();
    if (k < D) red[k] = M[k * kLd + k];
    __syncthreads();
    const double s = ordered_sum(red, D);
    __syncthreads();
    return s;
}

// One wave of kMaxD lanes (the whole workgroup); A, Vt (both pitch kLd) and red (kMaxD) are the caller's, in LDS.  Lane k owns column k of
// the symmetric matrix A (kept whole: rows p and q are read along k, the mirror entries are written back) and, with kVectors, column k of
// V^T, which starts as the identity (Vt[k][:] = eigenvector of A[k][k] at the end).  Row-cyclic sweeps over the pairs p < q; a rotation
// (Rutishauser's formulas) zeroes A[p][q]:
//   theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c.
// Before each sweep off = sqrt(sum of squared off-diagonal entries); stops at off <= rel_tol * frob, frob = ||A||_F of the matrix given
// (-> true), or after max_sweeps sweeps (-> false; NaN never compares true, so a non-finite matrix ends this way).
template <bool kVectors>
__device__ bool sweep(double* A, double* Vt, double* red, int D, int max_sweeps, double rel_tol, int& sweeps, double& off, double& frob) {
    const int k = threadIdx.x;
    const bool active = k < D;
    __syncthreads();  // the caller's last write to A
    if (active) {
        double s = 0.0;
        for (int i = 0; i < D; ++i) {
            s = add_rn(s, mul_rn(A[i * kLd + k], A[i * kLd + k]));
            if (kVectors) Vt[i * kLd + k] = i == k ? 1.0 : 0.0;
        }
        red[k] = s;
    }
    __syncthreads();
    frob = sqrt(ordered_sum(red, D));
    const double tol = mul_rn(rel_tol, frob);
    sweeps = 0;
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
        if (off <= tol) return true;
        if (sweeps == max_sweeps) return false;
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
                    if (kVectors) {
                        vp = Vt[p * kLd + k];
                        vq = Vt[q * kLd + k];
                    }
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
                    if (kVectors) {
                        Vt[p * kLd + k] = sub_rn(mul_rn(c, vp), mul_rn(s, vq));
                        Vt[q * kLd + k] = add_rn(mul_rn(s, vp), mul_rn(c, vq));
                    }
                }
                __syncthreads();
            }
        ++sweeps;
    }
}

// The eigen-decomposition of the covariance cov (D, D): load, trace, sweep, then the ranking and the sign rule.  Error bit 0: max_sweeps
// sweeps did not converge; bit 1: trace(C) is not positive.  info = [sweeps done, final off, ||C||_F, trace(C)].  evals (D) are ranked in
// descending order (ties: the lower column first); the n_comps leading eigenvectors go to comps (n_comps, D), each signed so that its entry
// of largest magnitude (first of equals) is positive.
__device__ __forceinline__ void eigh_one_wave(const double* __restrict__ cov, int D, int max_sweeps, double rel_tol, int n_comps,
                                              double* __restrict__ evals, double* __restrict__ comps, double* __restrict__ info,
                                              int32_t* __restrict__ err) {
    __shared__ double A[kMaxD * kLd];
    __shared__ double Vt[kMaxD * kLd];
    __shared__ double red[kMaxD];
    const int k = threadIdx.x;
    const bool active = k < D;
    if (active)
        for (int i = 0; i < D; ++i) A[i * kLd + k] = cov[i * D + k];
    const double trace = trace_of(A, red, D);
    int sweeps;
    double off, frob;
    int error = sweep<true>(A, Vt, red, D, max_sweeps, rel_tol, sweeps, off, frob) ? 0 : 1;
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
                const double v = Vt[k * kLd + i];
                if (fabs(v) > big) {
                    big = fabs(v);
                    sign = v < 0.0 ? -1.0 : 1.0;
                }
            }
            for (int i = 0; i < D; ++i) comps[rank * D + i] = mul_rn(sign, Vt[k * kLd + i]);
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

// the one eigen kernel's launcher (code_pca.hip); the two entry points validate their own arguments first and check the launch after
void launch_eigh(const double* cov, int dim, int max_sweeps, double rel_tol, int n_comps, double* evals, double* comps, double* info,
                 int32_t* err, void* stream);

}  // namespace sdt_jacobi
