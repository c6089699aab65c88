// The record-table protocol of the per-clip validation metrics, shared by clip_metrics.hip, sync_metrics.hip and motion_dist.hip (DESIGN.md section 22 states it;
// _record_table.py is the host side).  A table is (N + 1, cols) int64: one record per clip of the validation set, then a header row whose
// word 0 counts the clip indices outside the table.  Under data parallelism there is one table per rank, and per clip the lowest rank whose
// record has its seen word set gives the record.  The epoch sum runs over chunks of 64 clips in index order, then over the chunk partials in
// order.  The word layouts, what each word adds up and the final divisions belong to the families.
#pragma once
#include "exact_lanes.h"

namespace sdt_table {

constexpr int kMaxRanks = 64;
constexpr int kChunk = 64;  // clips per chunk of the epoch sum

struct Tables {
    const int64_t* t[kMaxRanks];
};

// the first ``ranks`` of ``tables`` into ``tb`` (the rest null) -> false if one of them is null
inline bool fill_tables(Tables& tb, const void* const* tables, int ranks) {
    for (int r = 0; r < kMaxRanks; ++r) {
        if (r < ranks && !tables[r]) return false;
        tb.t[r] = r < ranks ? (const int64_t*)tables[r] : nullptr;
    }
    return true;
}

// the record of clip n from the lowest rank that has seen it, or nullptr
__device__ __forceinline__ const int64_t* first_seen(const Tables& tb, int ranks, int64_t n, int cols, int seen) {
    for (int r = 0; r < ranks; ++r) {
        const int64_t* cand = tb.t[r] + (size_t)n * cols;
        if (cand[seen] != 0) return cand;
    }
    return nullptr;
}

// the header row: a commit whose clip index lies outside the table writes nothing but this count (the only atomic, an integer one)
__device__ __forceinline__ void count_index_error(int64_t* table, int64_t N, int cols) {
    atomicAdd(reinterpret_cast<unsigned long long*>(table + (size_t)N * cols), 1ull);
}
__device__ __forceinline__ int64_t index_errors(const Tables& tb, int ranks, int64_t N, int cols) {
    int64_t e = 0;
    for (int r = 0; r < ranks; ++r) e += tb.t[r][(size_t)N * cols];
    return e;
}

// word c of the chunk partials (``words`` each), summed in chunk order
__device__ __forceinline__ double chunk_sum_f64(const int64_t* __restrict__ work, int64_t chunks, int words, int c) {
    double s = 0.0;
    for (int64_t i = 0; i < chunks; ++i) s = sdt_exact::add_rn(s, sdt_exact::double_of(work[(size_t)i * words + c]));
    return s;
}
__device__ __forceinline__ int64_t chunk_sum_i64(const int64_t* __restrict__ work, int64_t chunks, int words, int c) {
    int64_t h = 0;
    for (int64_t i = 0; i < chunks; ++i) h += work[(size_t)i * words + c];
    return h;
}

__device__ __forceinline__ double quotient(double x, int64_t n) { return n == 0 ? 0.0 : sdt_exact::div_rn(x, (double)n); }

}  // namespace sdt_table
