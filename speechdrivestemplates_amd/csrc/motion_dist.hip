// Histograms of speed, acceleration and jerk magnitudes of final float64 poses and their Hellinger distances (TEST.MOTION_DIST;
// include/sdt_hip.h states the record layout, DESIGN.md section 31 the contract; motion_dist.motion_dist_model / epoch_model in Python are the
// same operations in the same order).
//
// Differences are successive, each subtraction rounded on its own: d1(t) = x(t+1) - x(t), d2(t) = d1(t+1) - d1(t), d3(t) = d2(t+1) - d2(t).
// A term's bin is the number of squared inner edges <= dx^2 + dy^2 (compared on squares: no count depends on the square root); a NaN is
// counted nowhere and flags the record.  Orders of summation, all fixed:
//   inside a frame   lane k holds keypoint k's sqrt term (+0.0 outside the part and for k >= K); the two waves of a source each run the xor
//                    butterfly, then wave 0 + wave 1;
//   over the frames  the T - o frame sums of order o serially, from +0.0;
//   over the copies  j = 0 .. m-1, serially;
//   over the clips   chunks of 64 clips in index order, then the chunk partials in order.
// Every multiply, add, subtract and divide goes through sdt_exact::*_rn (no FMA); counts are integers.  No floating-point atomics: the
// histogram counters are integer atomics in LDS, one copy per wave, flushed once per row; the only global atomic is the integer count of
// clip indices outside the table.
#include "record_table.h"

using namespace sdt_exact;
using namespace sdt_table;

namespace {

constexpr int kCols = SDT_MOTION_DIST_COLS;  // words of a record
constexpr int kBins = 32, kEdges = kBins - 1, kOrders = 3;
constexpr int kSrcCounts = kOrders * 3 * kBins;  // 288 counts of one source: [order][body, face, hands][bin]
constexpr int kFloats = 24;                      // mag_sum[source][order][part of 4]
constexpr int kCount0 = kFloats;                 // packed counts: count i of 576 in word 24 + i / 2, even i in the low half
constexpr int kSeen = 312, kCopies = 313, kNonfinite = 314, kFrames = 315;
constexpr int kMaxK = 128;
constexpr int kMaxCopies = 16;
constexpr int kMaxT = 65536;
constexpr int kTile = 16;  // frames whose per-wave sums wait in LDS for the serial sum over t
// words of a chunk partial: [0, 24) the float sums, then three blocks of 288 int64 counts (the prediction; the ground truth of the clips with an
// even index; of those with an odd index), 888 clips with a record, 889 of them left out as nonfinite
constexpr int kChunkWords = 896, kChunkPred = 24, kChunkEven = 312, kChunkOdd = 600, kChunkSeen = 888, kChunkBad = 889;
constexpr int kHalfHist = kOrders * 4 * kBins;  // one source's merged histograms: [order][all, body, face, hands][bin]

// the number of squared inner edges <= q (q is not a NaN): the upper bound of a non-decreasing table of 31
__device__ __forceinline__ int bin_of(const double* __restrict__ e2, double q) {
    int lo = 0;
#pragma unroll
    for (int step = 16; step > 0; step >>= 1)
        if (e2[lo + step - 1] <= q) lo += step;
    return lo;
}

// one workgroup of four waves per row: waves 0, 1 hold the prediction's keypoints (lane k of the pair is keypoint k), waves 2, 3 the ground
// truth's.  The three differences ride in registers along t, so every pose is read once.
__global__ __launch_bounds__(256) void motion_rows_kernel(const double* __restrict__ pred, const double* __restrict__ gt,
                                                          const uint8_t* __restrict__ parts, const double* __restrict__ edges, int T, int K,
                                                          int64_t* __restrict__ rows) {
    __shared__ double e2[kOrders][kBins];  // (31 used)
    __shared__ unsigned H[2][2][kSrcCounts];
    __shared__ double sred[2][2][kTile][12];
    const int tid = threadIdx.x, src = tid >> 7, k = tid & 127, half = k >> 6, lane = tid & 63;
    const bool on = k < K;
    for (int i = tid; i < 2 * 2 * kSrcCounts; i += 256) (&H[0][0][0])[i] = 0u;
    if (tid < kOrders * kEdges) e2[tid / kEdges][tid % kEdges] = edges[(size_t)(tid / kEdges) * 2 * kEdges + kEdges + tid % kEdges];
    const double* x = (src ? gt : pred) + (size_t)blockIdx.x * T * 2 * K;
    const int part = on ? (parts[k] < 2 ? parts[k] : 2) : -1;  // (a byte outside {0, 1, 2} must not index past the counters)
    unsigned* hist = &H[src][half][0];
    double px = 0.0, py = 0.0, p1x = 0.0, p1y = 0.0, p2x = 0.0, p2y = 0.0;  // x(t-1), d1(t-2), d2(t-3)
    double nx = 0.0, ny = 0.0;
    if (on) {
        nx = x[k];
        ny = x[K + k];
    }
    double acc = 0.0;  // thread c < 24: mag_sum word c
    bool nan_term = false;
    const int co = (tid % 12) >> 2;  // the order of word c = tid
    __syncthreads();
    for (int t0 = 0; t0 < T; t0 += kTile) {
        const int nt = T - t0 < kTile ? T - t0 : kTile;
        for (int i = 0; i < nt; ++i) {
            const int t = t0 + i;
            const double cx = nx, cy = ny;
            if (on && t + 1 < T) {
                nx = x[(size_t)(t + 1) * 2 * K + k];
                ny = x[(size_t)(t + 1) * 2 * K + K + k];
            }
            double d[kOrders][2];
            d[0][0] = sub_rn(cx, px), d[0][1] = sub_rn(cy, py);
            d[1][0] = sub_rn(d[0][0], p1x), d[1][1] = sub_rn(d[0][1], p1y);
            d[2][0] = sub_rn(d[1][0], p2x), d[2][1] = sub_rn(d[1][1], p2y);
            px = cx, py = cy, p1x = d[0][0], p1y = d[0][1], p2x = d[1][0], p2y = d[1][1];
#pragma unroll
            for (int o = 0; o < kOrders; ++o) {
                const bool have = on && t > o;  // frame t completes the order-(o+1) term d(t - o - 1)
                double term = 0.0;
                if (have) {
                    const double q = norm2(d[o][0], d[o][1]);
                    term = sqrt(q);
                    if (q != q) nan_term = true;
                    else atomicAdd(&hist[(o * 3 + part) * kBins + bin_of(e2[o], q)], 1u);
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const double v = butterfly_sum(have && in_part(p, part) ? term : 0.0);
                    if (lane == 0) sred[src][half][i][o * 4 + p] = v;
                }
            }
        }
        __syncthreads();
        if (tid < kFloats) {
            const int s = tid / 12, r = tid % 12;
            for (int i = 0; i < nt; ++i)
                if (t0 + i > co) acc = add_rn(acc, add_rn(sred[s][0][i][r], sred[s][1][i][r]));
        }
        __syncthreads();
    }
    const int nonfinite = __syncthreads_or(nan_term || (tid < kFloats && !finite_d(acc)));
    int64_t* out = rows + (size_t)blockIdx.x * kCols;
    if (tid < kFloats) out[tid] = bits_of(acc);
    for (int w = tid; w < kSrcCounts; w += 256) {  // word w of the packed counts: counts 2 w and 2 w + 1 of the 576
        const int s = w / (kSrcCounts / 2), j = 2 * (w % (kSrcCounts / 2));
        const uint64_t lo = H[s][0][j] + H[s][1][j], hi = H[s][0][j + 1] + H[s][1][j + 1];
        out[kCount0 + w] = (int64_t)(lo | (hi << 32));
    }
    if (tid == 252) out[kSeen] = 1;
    else if (tid == 253) out[kCopies] = 1;
    else if (tid == 254) out[kNonfinite] = nonfinite ? 1 : 0;
    else if (tid == 255) out[kFrames] = T;
}

// one workgroup of five waves per clip of the call: thread c forms word c of the clip's record, into row clip_index[b] of the table
__global__ __launch_bounds__(320) void motion_commit_kernel(const int64_t* __restrict__ rows, const int64_t* __restrict__ clip_index, int B, int m,
                                                            int T, int64_t* __restrict__ table, int64_t N) {
    const int b = blockIdx.x, c = threadIdx.x;
    double s = 0.0;
    uint64_t lo = 0, hi = 0;
    int64_t h = 0;
    if (c < kFloats) {
        for (int j = 0; j < m; ++j) s = add_rn(s, double_of(rows[((size_t)j * B + b) * kCols + c]));
    } else if (c < kSeen) {
        for (int j = 0; j < m; ++j) {
            const uint64_t w = (uint64_t)rows[((size_t)j * B + b) * kCols + c];
            lo += w & 0xffffffffull;
            hi += w >> 32;
        }
    } else if (c == kNonfinite) {
        for (int j = 0; j < m; ++j) h += rows[((size_t)j * B + b) * kCols + c];
    }
    const int nonfinite = __syncthreads_or((c < kFloats && !finite_d(s)) || (c == kNonfinite && h != 0));
    const int64_t idx = clip_index[b];
    if (idx < 0 || idx >= N) {  // writes nothing but the header's count
        if (c == 0) count_index_error(table, N, kCols);
        return;
    }
    int64_t* out = table + (size_t)idx * kCols;
    if (c < kFloats) out[c] = bits_of(s);
    else if (c < kSeen) out[c] = (int64_t)(lo | (hi << 32));  // (a clip has m (T - o) |part| <= m T K < 2^31 terms: no half overflows)
    else if (c == kSeen) out[c] = 1;
    else if (c == kCopies) out[c] = m;
    else if (c == kNonfinite) out[c] = nonfinite ? 1 : 0;
    else if (c == kFrames) out[c] = T;
}

__device__ __forceinline__ int64_t count_of(const int64_t* rec, int i) {  // count i of the record's 576
    const uint64_t w = (uint64_t)rec[kCount0 + (i >> 1)];
    return (int64_t)((i & 1) ? w >> 32 : w & 0xffffffffull);
}

// one workgroup per chunk of 64 clips: thread c forms words c, c + 256, .. of the chunk's partial, clips in index order, each from the lowest
// rank that has seen it
__global__ __launch_bounds__(256) void motion_epoch_chunk_kernel(Tables tb, int ranks, int64_t N, int64_t* __restrict__ work) {
    __shared__ const int64_t* srec[kChunk];
    const int tid = threadIdx.x;
    const int64_t n0 = (int64_t)blockIdx.x * kChunk, n1 = n0 + kChunk < N ? n0 + kChunk : N;
    if (tid < kChunk) srec[tid] = n0 + tid < n1 ? first_seen(tb, ranks, n0 + tid, kCols, kSeen) : nullptr;
    __syncthreads();
    for (int c = tid; c < kChunkWords; c += 256) {
        double s = 0.0;
        int64_t h = 0;
        for (int i = 0; i < (int)(n1 - n0); ++i) {
            const int64_t* rec = srec[i];
            if (!rec) continue;
            const bool bad = rec[kNonfinite] != 0;
            if (c == kChunkSeen) h += 1;
            else if (c == kChunkBad) h += bad ? 1 : 0;
            else if (bad) continue;
            else if (c < kFloats) s = add_rn(s, double_of(rec[c]));
            else if (c < kChunkEven) h += count_of(rec, c - kChunkPred);
            else if (c < kChunkOdd) h += ((n0 + i) & 1) ? 0 : count_of(rec, kSrcCounts + c - kChunkEven);
            else if (c < kChunkSeen) h += ((n0 + i) & 1) ? count_of(rec, kSrcCounts + c - kChunkOdd) : 0;
        }
        work[(size_t)blockIdx.x * kChunkWords + c] = c < kFloats ? bits_of(s) : h;
    }
}

// Bhattacharyya coefficient and Hellinger distance of two histograms of 32 int64 counts; 0.0 both if either is empty
__device__ __forceinline__ void hellinger(const int64_t* a, const int64_t* b, double& bc, double& hd) {
    int64_t na = 0, nb = 0;
    for (int i = 0; i < kBins; ++i) na += a[i], nb += b[i];
    bc = 0.0, hd = 0.0;
    if (na == 0 || nb == 0) return;
    for (int i = 0; i < kBins; ++i) bc = add_rn(bc, sqrt(mul_rn(div_rn((double)a[i], (double)na), div_rn((double)b[i], (double)nb))));
    const double d = sub_rn(1.0, bc);
    hd = sqrt(d < 0.0 ? 0.0 : d);
}

// one workgroup: the chunk partials in order, "all" as the sum of the three parts, then the distances and the ratios
__global__ __launch_bounds__(256) void motion_epoch_final_kernel(Tables tb, int ranks, int64_t N, const int64_t* __restrict__ work, int64_t chunks,
                                                                 int64_t* __restrict__ out, int64_t* __restrict__ hist) {
    __shared__ int64_t tot[kChunkWords];
    __shared__ int64_t cnt[4][kOrders][4][kBins];  // the prediction, the ground truth, its even-index clips, its odd-index clips
    __shared__ int64_t errors;
    const int tid = threadIdx.x;
    for (int c = tid; c < kChunkWords; c += 256)
        tot[c] = c < kFloats ? bits_of(chunk_sum_f64(work, chunks, kChunkWords, c)) : chunk_sum_i64(work, chunks, kChunkWords, c);
    if (tid == 255) errors = index_errors(tb, ranks, N, kCols);
    __syncthreads();
    for (int i = tid; i < kHalfHist; i += 256) {
        const int o = i / (4 * kBins), p = i / kBins % 4, b = i % kBins;
        int64_t v[3] = {0, 0, 0};
        for (int part = 0; part < 3; ++part) {
            if (p != 0 && part != p - 1) continue;
            const int j = (o * 3 + part) * kBins + b;
            v[0] += tot[kChunkPred + j], v[1] += tot[kChunkEven + j], v[2] += tot[kChunkOdd + j];
        }
        cnt[0][o][p][b] = v[0], cnt[1][o][p][b] = v[1] + v[2], cnt[2][o][p][b] = v[1], cnt[3][o][p][b] = v[2];
        hist[i] = v[0];
        hist[kHalfHist + i] = v[1] + v[2];
    }
    __syncthreads();
    if (tid < 24) {  // 12 (order, part) pairs of the distance, then 12 of its noise floor
        const int kind = tid / 12, r = tid % 12;
        double bc, hd;
        hellinger(cnt[2 * kind][r / 4][r % 4], cnt[2 * kind + 1][r / 4][r % 4], bc, hd);
        out[24 * kind + r] = bits_of(hd);
        out[24 * kind + 12 + r] = bits_of(bc);
    } else if (tid < 36) {
        const int r = tid - 24;
        const double den = double_of(tot[12 + r]);
        out[48 + r] = bits_of(den == 0.0 ? 0.0 : div_rn(double_of(tot[r]), den));
    } else if (tid == 60) {
        out[tid] = tot[kChunkSeen];
    } else if (tid == 61) {
        out[tid] = tot[kChunkBad];
    } else if (tid == 62) {
        out[tid] = errors;
    } else if (tid == 63) {
        out[tid] = 0;
    }
}

}  // namespace

extern "C" int sdt_motion_dist_rows_f64(const double* pred, const double* gt, const uint8_t* parts, const double* edges, int R, int T, int K,
                                        void* rows, void* stream) {
    SDT_CHECK_ARG(pred && gt && parts && edges && rows, "null pointer");
    SDT_CHECK_ARG(K >= 1 && K <= kMaxK, "K outside [1, 128]");
    SDT_CHECK_ARG(R >= 1 && T >= 1 && T <= kMaxT, "bad dims (R >= 1, T in [1, 65536])");
    hipLaunchKernelGGL(motion_rows_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, pred, gt, parts, edges, T, K, (int64_t*)rows);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_motion_dist_commit(const void* rows, const int64_t* clip_index, int B, int m, int T, int K, void* table, int64_t N,
                                      void* stream) {
    SDT_CHECK_ARG(rows && clip_index && table, "null pointer");
    SDT_CHECK_ARG(m >= 1 && m <= kMaxCopies, "copies outside [1, 16]");
    SDT_CHECK_ARG(K >= 1 && K <= kMaxK, "K outside [1, 128]");
    SDT_CHECK_ARG(B >= 1 && T >= 1 && T <= kMaxT && N >= 1, "bad dims (B >= 1, T in [1, 65536], N >= 1)");
    SDT_CHECK_ARG((int64_t)m * T * K <= 0x7fffffff, "m * T * K must stay below 2^31 (a clip's counts are packed as int32)");
    hipLaunchKernelGGL(motion_commit_kernel, dim3(B), dim3(320), 0, (hipStream_t)stream, (const int64_t*)rows, clip_index, B, m, T,
                       (int64_t*)table, N);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int64_t sdt_motion_dist_epoch_work_words(int64_t N) { return N < 1 ? 0 : cdiv64(N, kChunk) * kChunkWords; }

extern "C" int sdt_motion_dist_epoch(const void* const* tables, int ranks, int64_t N, void* work, void* out, void* hist, void* stream) {
    SDT_CHECK_ARG(tables && work && out && hist, "null pointer");
    SDT_CHECK_ARG(ranks >= 1 && ranks <= kMaxRanks, "tables outside [1, 64]");
    SDT_CHECK_ARG(N >= 1 && cdiv64(N, kChunk) <= 0x7fffffff, "bad number of clips");
    Tables tb;
    SDT_CHECK_ARG(fill_tables(tb, tables, ranks), "null table");
    const int64_t chunks = cdiv64(N, kChunk);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(motion_epoch_chunk_kernel, dim3((unsigned)chunks), dim3(256), 0, s, tb, ranks, N, (int64_t*)work);
    hipLaunchKernelGGL(motion_epoch_final_kernel, dim3(1), dim3(256), 0, s, tb, ranks, N, (const int64_t*)work, chunks, (int64_t*)out,
                       (int64_t*)hist);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
