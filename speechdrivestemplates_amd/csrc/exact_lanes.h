// The lane helpers of the bit-exact metric kernels, shared by clip_metrics.hip, sync_metrics.hip, long_demo.hip, augment.hip and motion_dist.hip: these are the
// summation order of their contracts (_exact_model.py holds the same operations in numpy).
#pragma once
#include "exact_f64.h"

namespace sdt_exact {

// the xor butterfly of one wave: v += shfl_xor(v, o) for o = 32, 16, 8, 4, 2, 1 (addition commutes, so every lane ends with the same bits)
__device__ __forceinline__ double butterfly_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = add_rn(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int64_t butterfly_count(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double norm2(double x, double y) { return add_rn(mul_rn(x, x), mul_rn(y, y)); }
__device__ __forceinline__ bool in_part(int p, int part) { return p == 0 || part == p - 1; }  // p: 0 all, 1 body, 2 face, 3 hands
__device__ __forceinline__ int64_t bits_of(double v) { return __double_as_longlong(v); }
__device__ __forceinline__ double double_of(int64_t v) { return __longlong_as_double(v); }
__device__ __forceinline__ bool finite_d(double v) { return fabs(v) < __builtin_huge_val(); }  // false for NaN and +-inf

}  // namespace sdt_exact
