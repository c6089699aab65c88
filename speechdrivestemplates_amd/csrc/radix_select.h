// The pieces of the exact float64 radix select that code_axes.hip (quantiles of the projected table) and speech_gate.hip (the noise
// floor of the hop energies) share: the order-preserving uint64 image of a float64 and the choice of one 8-bit digit from a 256-bin
// histogram.  A select is 8 passes from the top byte down: count the digits of the elements whose higher bytes equal the surviving
// prefix, then pick the digit whose cumulative count passes the remaining rank.  Integers only: the result is one of the inputs.
#pragma once
#include "common.h"

namespace sdt_select {

// float64 bits -> uint64 with the same order (negative numbers: all bits flipped; others: the sign bit set); -0.0 sorts just below +0.0
__device__ __forceinline__ unsigned long long order_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double order_value(unsigned long long key) {
    const unsigned long long b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
    return __longlong_as_double((long long)b);
}

// the digit whose cumulative count passes the remaining rank, which is reduced by the counts below it
__device__ __forceinline__ int pick_digit(const uint32_t* cnt, long long* remain) {
    long long rem = *remain;
    int digit = 255;  // (counts of a consistent state always reach the rank; 255 keeps a corrupted one inside the table)
    for (int d = 0; d < 256; ++d) {
        const long long c = (long long)cnt[d];
        if (rem < c) {
            digit = d;
            break;
        }
        rem -= c;
    }
    *remain = rem;
    return digit;
}

}  // namespace sdt_select
