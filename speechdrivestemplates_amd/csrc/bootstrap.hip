// Bootstrap over the clips of a record table (TEST.BOOTSTRAP; include/sdt_hip.h states the layouts, DESIGN.md section 34 the contract;
// bootstrap.stages_model in Python is the same operations in the same order).  Four stages:
//   dense      the live records (seen, not nonfinite -- in both table sets of the paired form) of the merged tables, in clip order, as rows
//              of 39 words, and the un-resampled sums of those records in the order of the epoch stage (chunks of 64 clips of the TABLE);
//   sums       generic: replicate r draws n rows with Philox4x32-10 and sums them in chunks of 64 DRAWS in draw order, then the chunk
//              partials in order; float words through add_rn, integer words exactly;
//   values     the final divisions of sdt_clip_metrics_epoch on every sum row (clip_epoch_final_kernel of clip_metrics.hip is the original:
//              the same operations on the same operands, so the point row carries the epoch's bits);
//   intervals  per column the order statistics at two ranks by the exact radix select of radix_select.h, and the signs of a difference.
// Every wave owns its outputs and adds in a fixed order, so no result depends on the grid.  The only atomics are integer ones on LDS counters.
#include "philox.h"
#include "radix_select.h"
#include "record_table.h"

using namespace sdt_exact;
using namespace sdt_table;

namespace {

constexpr int kCols = SDT_CLIP_METRICS_COLS;      // words of a record
constexpr int kWords = SDT_BOOTSTRAP_CLIP_WORDS;  // words of a dense row: 20 float sums, 16 hit counts, 3 derived counts
constexpr int kFloats = 20;
constexpr int kValues = SDT_BOOTSTRAP_CLIP_VALUES;
constexpr int kSeen = 36, kCopies = 37, kNonfinite = 38, kFrames = 39;  // words of a record
constexpr int kPos = 36, kVel = 37, kPair = 38;  // derived words of a dense row: copies * frames, copies * (frames - 1), pairs * frames
constexpr int kDenseWork = SDT_BOOTSTRAP_DENSE_WORK;  // per chunk: live mask, first dense row, partial of set A, partial of set B
constexpr int kMaxAlphas = 4;
constexpr uint32_t kPurpose = 3;  // counter word 1 (0 .. 2 belong to augment.hip and pose_augment.hip)

struct PartSizes {
    int64_t n[4];
};

__device__ __forceinline__ const int64_t* live_record(const Tables& tb, int ranks, int64_t n) {
    const int64_t* rec = first_seen(tb, ranks, n, kCols, kSeen);
    return rec && rec[kNonfinite] == 0 ? rec : nullptr;
}

// ---- stage 1 ---------------------------------------------------------------------------------------------------------------------------------
// one wave per chunk of 64 clips, lane j holds clip n0 + j: the chunk's mask of live clips
__global__ __launch_bounds__(64) void dense_flag_kernel(Tables ta, int ranks_a, Tables tb, int ranks_b, int64_t N, int64_t* __restrict__ work) {
    const int64_t n = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    bool live = n < N && live_record(ta, ranks_a, n) != nullptr;
    if (live && ranks_b > 0) live = live_record(tb, ranks_b, n) != nullptr;
    const unsigned long long mask = __ballot(live);
    if (threadIdx.x == 0) work[(size_t)blockIdx.x * kDenseWork] = (int64_t)mask;
}

// one wave: the first dense row of every chunk (an exclusive prefix sum of integers) and the number of live clips
__global__ __launch_bounds__(64) void dense_scan_kernel(int64_t* __restrict__ work, int64_t chunks, int64_t* __restrict__ n_out) {
    const int lane = threadIdx.x;
    const int64_t per = (chunks + 63) / 64;
    const int64_t c0 = lane * per < chunks ? lane * per : chunks, c1 = c0 + per < chunks ? c0 + per : chunks;
    long long own = 0;
    for (int64_t c = c0; c < c1; ++c) own += __popcll((unsigned long long)work[(size_t)c * kDenseWork]);
    long long incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    long long off = incl - own;
    for (int64_t c = c0; c < c1; ++c) {
        work[(size_t)c * kDenseWork + 1] = off;
        off += __popcll((unsigned long long)work[(size_t)c * kDenseWork]);
    }
    if (lane == 63) n_out[0] = incl;
}

// one wave per (chunk, table set): word c of the chunk's live records into their dense rows, in clip order, and word c of the chunk's partial
__global__ __launch_bounds__(64) void dense_scatter_kernel(Tables ta, int ranks_a, Tables tb, int ranks_b, int64_t* __restrict__ work,
                                                           int64_t* __restrict__ dense_a, int64_t* __restrict__ dense_b) {
    const int c = threadIdx.x;
    const bool second = blockIdx.y == 1;
    const Tables& t = second ? tb : ta;
    const int ranks = second ? ranks_b : ranks_a;
    int64_t* dense = second ? dense_b : dense_a;
    int64_t* w = work + (size_t)blockIdx.x * kDenseWork;
    const unsigned long long mask = (unsigned long long)w[0];
    int64_t row = w[1];
    const int64_t n0 = (int64_t)blockIdx.x * kChunk;
    double s = 0.0;
    int64_t h = 0;
    for (int j = 0; j < kChunk; ++j) {
        if (!((mask >> j) & 1ull)) continue;
        const int64_t* rec = first_seen(t, ranks, n0 + j, kCols, kSeen);
        if (rec && c < kWords) {  // (the mask says there is one)
            int64_t v;
            if (c < kSeen) {
                v = rec[c];
            } else {
                const int64_t copies = rec[kCopies], frames = rec[kFrames];
                v = c == kPos ? copies * frames : c == kVel ? copies * (frames - 1) : copies * (copies - 1) / 2 * frames;
            }
            dense[(size_t)row * kWords + c] = v;
            if (c < kFloats) s = add_rn(s, double_of(v));
            else h += v;
        }
        ++row;
    }
    if (c < kWords) w[2 + (second ? kWords : 0) + c] = c < kFloats ? bits_of(s) : h;
}

// one wave per table set: the chunk partials in order
__global__ __launch_bounds__(64) void dense_point_kernel(const int64_t* __restrict__ work, int64_t chunks, int64_t* __restrict__ point_a,
                                                         int64_t* __restrict__ point_b) {
    const int c = threadIdx.x;
    const int64_t* w = work + 2 + (blockIdx.x == 1 ? kWords : 0);
    int64_t* out = blockIdx.x == 1 ? point_b : point_a;
    if (c < kFloats) out[c] = bits_of(chunk_sum_f64(w, chunks, kDenseWork, c));
    else if (c < kWords) out[c] = chunk_sum_i64(w, chunks, kDenseWork, c);
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------------------------------
// draw i of replicate r: word i & 3 of the block with the counter (i >> 2, purpose, r, 0), scaled to [0, n)
__device__ __forceinline__ int64_t draw_row(int64_t i, uint32_t r, sdt_philox::Key key, int64_t n) {
    const sdt_philox::Words p = sdt_philox::philox4x32((uint32_t)(i >> 2), kPurpose, r, 0u, key);
    const int q = (int)(i & 3);
    const uint32_t word = q == 0 ? p.w[0] : q == 1 ? p.w[1] : q == 2 ? p.w[2] : p.w[3];
    return (int64_t)(((unsigned long long)word * (unsigned long long)n) >> 32);
}

// one wave per (chunk of 64 draws, replicate): lane j makes draw j of the chunk, lane c adds word c of the drawn rows in draw order
__global__ __launch_bounds__(64) void replicate_chunk_kernel(const int64_t* __restrict__ dense, int64_t n, int words, int floats,
                                                             sdt_philox::Key key, int64_t chunks, int64_t* __restrict__ work) {
    const int c = threadIdx.x;
    const uint32_t r = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * kChunk;
    const long long mine = draw_row(i0 + c, r, key, n);  // (< n for every lane, also past the last draw)
    const int m = n - i0 < kChunk ? (int)(n - i0) : kChunk;
    double s = 0.0;
    int64_t h = 0;
    for (int j = 0; j < m; ++j) {
        const long long row = __shfl(mine, j, 64);
        if (c < words) {
            const int64_t v = dense[(size_t)row * words + c];
            if (c < floats) s = add_rn(s, double_of(v));
            else h += v;
        }
    }
    if (c < words) work[((size_t)r * chunks + blockIdx.x) * words + c] = c < floats ? bits_of(s) : h;
}

// one wave per replicate: the chunk partials in order
__global__ __launch_bounds__(64) void replicate_final_kernel(const int64_t* __restrict__ work, int64_t chunks, int words, int floats,
                                                             int64_t* __restrict__ sums) {
    const int c = threadIdx.x;
    const int64_t* w = work + (size_t)blockIdx.x * chunks * words;
    int64_t* out = sums + (size_t)blockIdx.x * words;
    if (c < floats) out[c] = bits_of(chunk_sum_f64(w, chunks, words, c));
    else if (c < words) out[c] = chunk_sum_i64(w, chunks, words, c);
}

// ---- stage 3 ---------------------------------------------------------------------------------------------------------------------------------
// one wave per sum row: lane c gives value word c, as clip_epoch_final_kernel does from the epoch's totals
__global__ __launch_bounds__(64) void clip_values_kernel(const int64_t* __restrict__ sums, PartSizes ps, int A, int64_t* __restrict__ values,
                                                         int64_t* __restrict__ pair_frames) {
    __shared__ int64_t tot[kWords];
    const int c = threadIdx.x;
    if (c < kWords) tot[c] = sums[(size_t)blockIdx.x * kWords + c];
    __syncthreads();
    const int p = c & 3;
    const int64_t n_pos = tot[kPos] * ps.n[p], n_vel = tot[kVel] * ps.n[p], n_div = tot[kPair] * ps.n[p];
    int64_t* out = values + (size_t)blockIdx.x * kValues;
    if (c < 4) {
        out[c] = bits_of(quotient(double_of(tot[c]), n_pos));
    } else if (c < 20) {
        out[c] = bits_of((c - 4) / 4 < A ? quotient((double)tot[20 + c - 4], n_pos) : 0.0);
    } else if (c < 24) {
        double s = 0.0;
        for (int a = 0; a < A; ++a) s = add_rn(s, quotient((double)tot[20 + a * 4 + p], n_pos));
        out[c] = bits_of(div_rn(s, (double)A));
    } else if (c < 28) {
        const double den = double_of(tot[8 + p]);
        out[c] = bits_of(den == 0.0 ? 0.0 : div_rn(double_of(tot[4 + p]), den));
    } else if (c < 32) {
        out[c] = bits_of(quotient(double_of(tot[12 + p]), n_vel));
    } else if (c < kValues) {
        out[c] = bits_of(quotient(double_of(tot[16 + p]), n_div));
    } else if (c == kValues) {
        pair_frames[blockIdx.x] = tot[kPair];
    }
}

__global__ __launch_bounds__(256) void diff_kernel(const double* __restrict__ a, const double* __restrict__ b, int64_t n, double* __restrict__ d) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) d[i] = sub_rn(a[i], b[i]);
}

// ---- stage 4 ---------------------------------------------------------------------------------------------------------------------------------
// one workgroup per (column, end of the interval): the order statistic at rank a resp. R - 1 - a of the column's R values, eight digit passes
__global__ __launch_bounds__(256) void interval_select_kernel(const double* __restrict__ values, int64_t R, int cols, int64_t a,
                                                              double* __restrict__ lohi, int64_t* __restrict__ counts) {
    __shared__ uint32_t cnt[256];
    __shared__ uint32_t sign[3];
    __shared__ unsigned long long prefix_s;
    __shared__ long long remain_s;
    const int t = threadIdx.x, col = blockIdx.x, high = blockIdx.y;
    if (t == 0) {
        prefix_s = 0ull;
        remain_s = high ? R - 1 - a : a;
    }
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        cnt[t] = 0u;
        __syncthreads();
        const unsigned long long prefix = prefix_s;
        for (int64_t r = t; r < R; r += 256) {
            const unsigned long long key = sdt_select::order_key(values[(size_t)r * cols + col]);
            if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&cnt[(key >> shift) & 255ull], 1u);
        }
        __syncthreads();
        if (t == 0) {
            long long rem = remain_s;
            const int digit = sdt_select::pick_digit(cnt, &rem);
            remain_s = rem;
            prefix_s = (prefix << 8) | (unsigned long long)digit;
        }
        __syncthreads();
    }
    if (t == 0) lohi[(size_t)col * 2 + high] = sdt_select::order_value(prefix_s);
    if (counts && !high) {  // the signs of the column (a NaN has none)
        if (t < 3) sign[t] = 0u;
        __syncthreads();
        uint32_t neg = 0, pos = 0, zero = 0;
        for (int64_t r = t; r < R; r += 256) {
            const double v = values[(size_t)r * cols + col];
            neg += v < 0.0;
            pos += v > 0.0;
            zero += v == 0.0;
        }
        atomicAdd(&sign[0], neg);
        atomicAdd(&sign[1], pos);
        atomicAdd(&sign[2], zero);
        __syncthreads();
        if (t < 3) counts[(size_t)col * 3 + t] = (int64_t)sign[t];
    }
}

}  // namespace

extern "C" int sdt_clip_metrics_replicate_dense(const void* const* tables_a, int ranks_a, const void* const* tables_b, int ranks_b, int64_t N,
                                                void* work, void* dense_a, void* dense_b, void* point_a, void* point_b, int64_t* n_out,
                                                void* stream) {
    SDT_CHECK_ARG(tables_a && work && dense_a && point_a && n_out, "null pointer");
    SDT_CHECK_ARG(ranks_a >= 1 && ranks_a <= kMaxRanks, "tables outside [1, 64]");
    SDT_CHECK_ARG(ranks_b >= 0 && ranks_b <= kMaxRanks, "tables of the second set outside [0, 64]");
    SDT_CHECK_ARG((ranks_b > 0) == (tables_b != nullptr) && (ranks_b > 0) == (dense_b != nullptr) && (ranks_b > 0) == (point_b != nullptr),
                  "the second set's tables, dense rows and point row come together");
    SDT_CHECK_ARG(N >= 1 && cdiv64(N, kChunk) <= 0x7fffffff, "bad number of clips");
    Tables ta, tb;
    SDT_CHECK_ARG(fill_tables(ta, tables_a, ranks_a), "null table");
    if (ranks_b > 0) SDT_CHECK_ARG(fill_tables(tb, tables_b, ranks_b), "null table in the second set");
    else fill_tables(tb, tables_a, 0);
    const int64_t chunks = cdiv64(N, kChunk);
    const unsigned sets = ranks_b > 0 ? 2u : 1u;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dense_flag_kernel, dim3((unsigned)chunks), dim3(64), 0, s, ta, ranks_a, tb, ranks_b, N, (int64_t*)work);
    hipLaunchKernelGGL(dense_scan_kernel, dim3(1), dim3(64), 0, s, (int64_t*)work, chunks, n_out);
    hipLaunchKernelGGL(dense_scatter_kernel, dim3((unsigned)chunks, sets), dim3(64), 0, s, ta, ranks_a, tb, ranks_b, (int64_t*)work,
                       (int64_t*)dense_a, (int64_t*)dense_b);
    hipLaunchKernelGGL(dense_point_kernel, dim3(sets), dim3(64), 0, s, (const int64_t*)work, chunks, (int64_t*)point_a, (int64_t*)point_b);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_bootstrap_sums(const void* dense, int64_t n, int words, int float_words, int replicates, uint64_t seed, void* work,
                                  void* sums, void* stream) {
    SDT_CHECK_ARG(dense && work && sums, "null pointer");
    SDT_CHECK_ARG(words >= 1 && words <= 64 && float_words >= 0 && float_words <= words, "words outside [1, 64] or float words outside [0, words]");
    SDT_CHECK_ARG(n >= 1 && n <= 0x7fffffff, "rows outside [1, 2^31)");
    SDT_CHECK_ARG(replicates >= 1 && replicates <= 65535, "replicates outside [1, 65535]");
    const int64_t chunks = cdiv64(n, kChunk);
    const sdt_philox::Key key = {(uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32)};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(replicate_chunk_kernel, dim3((unsigned)chunks, (unsigned)replicates), dim3(64), 0, s, (const int64_t*)dense, n, words,
                       float_words, key, chunks, (int64_t*)work);
    hipLaunchKernelGGL(replicate_final_kernel, dim3((unsigned)replicates), dim3(64), 0, s, (const int64_t*)work, chunks, words, float_words,
                       (int64_t*)sums);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_clip_metrics_replicate_values(const void* sums, int64_t rows, const int64_t* part_sizes, int num_alphas, void* values,
                                                 void* pair_frames, void* stream) {
    SDT_CHECK_ARG(sums && part_sizes && values && pair_frames, "null pointer");
    SDT_CHECK_ARG(rows >= 1 && rows <= 0x7fffffff, "rows outside [1, 2^31)");
    SDT_CHECK_ARG(num_alphas >= 1 && num_alphas <= kMaxAlphas, "number of alphas outside [1, 4]");
    PartSizes ps;
    for (int p = 0; p < 4; ++p) {
        SDT_CHECK_ARG(part_sizes[p] >= 0 && part_sizes[p] <= 128, "part size outside [0, 128]");
        ps.n[p] = part_sizes[p];
    }
    hipLaunchKernelGGL(clip_values_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, (const int64_t*)sums, ps, num_alphas,
                       (int64_t*)values, (int64_t*)pair_frames);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_bootstrap_diff_f64(const double* a, const double* b, int64_t n, double* d, void* stream) {
    SDT_CHECK_ARG(a && b && d && n >= 1 && cdiv64(n, 256) <= 0x7fffffff, "bad argument");
    hipLaunchKernelGGL(diff_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, (hipStream_t)stream, a, b, n, d);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_bootstrap_intervals_f64(const double* values, int64_t replicates, int cols, int64_t rank, double* lohi, int64_t* counts,
                                           void* stream) {
    SDT_CHECK_ARG(values && lohi, "null pointer");
    SDT_CHECK_ARG(replicates >= 1 && replicates <= 0x7fffffff, "replicates outside [1, 2^31)");
    SDT_CHECK_ARG(cols >= 1 && cols <= 65535, "columns outside [1, 65535]");
    SDT_CHECK_ARG(rank >= 0 && 2 * rank < replicates, "rank outside [0, replicates / 2)");
    hipLaunchKernelGGL(interval_select_kernel, dim3((unsigned)cols, 2u), dim3(256), 0, (hipStream_t)stream, values, replicates, cols, rank, lohi,
                       counts);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
