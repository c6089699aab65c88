// float64 device arithmetic that is reproducible to the bit, shared by speaker_stats.hip, code_pca.hip, code_axes.hip, fgd.hip, jacobi.h and,
// through exact_lanes.h (the lane helpers) and record_table.h, by clip_metrics.hip, sync_metrics.hip, long_demo.hip and augment.hip:
// the four operations each rounded on its own, the ordered sum, and the constants and the triangle indexing of the 64-wide problem.
#pragma once
#include "common.h"

namespace sdt_exact {

constexpr int kMaxD = 64;
constexpr int kLd = kMaxD + 1;  // pitch of a D x D matrix in LDS: a row read along the lanes and a column read along the lanes both spread over the banks
constexpr int kMaxTri = kMaxD * (kMaxD + 1) / 2;  // 2080 upper-triangle entries at D = 64

// float64 operations each rounded on its own.  HIP's mul_rn / add_rn are plain operators compiled under the default
// -ffp-contract, so x*w + om*q made of them still becomes an FMA; these carry the pragma in their own bodies.
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

// entry e of the upper triangle, row-major: (0,0) (0,1) .. (0,D-1) (1,1) ..
__device__ __forceinline__ void tri_entry(int e, int D, int& i, int& j) {
    i = 0;
    while (e >= D - i) {
        e -= D - i;
        ++i;
    }
    j = i + e;
}
// index of entry (i, j) of that triangle, any order of i and j
__device__ __forceinline__ int tri_index(int i, int j, int D) {
    const int a = i < j ? i : j, b = i < j ? j : i;
    return a * D - a * (a - 1) / 2 + (b - a);
}

}  // namespace sdt_exact
