// Per-clip validation metrics on final float64 poses (TEST.CLIP_METRICS; include/sdt_hip.h states the record layout, DESIGN.md section 22 the
// contract; clip_metrics.clip_metrics_model / epoch_model in Python are the same operations in the same order).
//
// Orders of summation, all fixed:
//   inside a frame   lane k holds keypoint k's term (+0.0 outside the part and for k >= K); the two waves each run the xor butterfly
//                    v += shfl_xor(v, o) for o = 32, 16, 8, 4, 2, 1 (addition commutes, so every lane ends with the same bits), then
//                    wave 0 + wave 1;
//   over the frames  t = 0 .. T-1, serially (the speed columns of frame T-1 are +0.0);
//   over the copies  j = 0 .. m-1, serially; diversity: every lane adds its pair terms in lexicographic (i, j) order before the butterfly;
//   over the clips   chunks of 64 clips in index order, then the chunk partials in order.
// Every multiply, add and subtract goes through sdt_exact::mul_rn / add_rn / sub_rn (no FMA); counts are integers.  No floating-point atomics:
// the only atomic is the integer count of clip indices outside the table.
#include "record_table.h"

using namespace sdt_exact;
using namespace sdt_table;

namespace {

constexpr int kCols = SDT_CLIP_METRICS_COLS;  // words of a record
constexpr int kFrameWords = 32;               // per-frame partial: 16 float64 sums {l2, speed_pred, speed_gt, vel_l2} x 4 parts, 16 int64 hit counts
constexpr int kMaxK = 128;
constexpr int kMaxCopies = 16;
constexpr int kMaxAlphas = 4;
constexpr int kChunkWords = 48;  // per-chunk partial: the 36 summed record words and the counters below
// words of a chunk partial beyond the record's sums: 36 clips with a record, 37 sum of copies * frames, 38 clips left out as nonfinite,
// 39 sum of copies * (frames - 1), 40 sum of copies (copies - 1) / 2 * frames
constexpr int kSeen = 36, kCopies = 37, kNonfinite = 38, kFrames = 39, kPairFrames = 40;

struct Alphas {
    double a[kMaxAlphas];
};
struct PartSizes {
    int64_t n[4];
};

// one workgroup of 128 threads per (row, frame); thread k handles keypoint k
__global__ __launch_bounds__(128) void clip_rows_frame_kernel(const double* __restrict__ pred, const double* __restrict__ gt,
                                                              const uint8_t* __restrict__ parts, Alphas al, int A, int T, int K,
                                                              int64_t* __restrict__ work) {
    __shared__ double sred[2][16];
    __shared__ double sbox[2][4];
    __shared__ int scount[2][16];
    const int rt = blockIdx.x, t = rt % T, k = threadIdx.x, wave = k >> 6, lane = k & 63;
    const bool on = k < K;
    const size_t base = (size_t)rt * 2 * K;
    double px = 0.0, py = 0.0, gx = 0.0, gy = 0.0;
    int part = -1;
    if (on) {
        px = pred[base + k];
        py = pred[base + K + k];
        gx = gt[base + k];
        gy = gt[base + K + k];
        part = parts[k];
    }
    // the ground truth's bounding box over all K keypoints (fmin / fmax skip a NaN; order does not matter to them)
    const double inf = __builtin_huge_val();
    double box[4] = {on ? gx : inf, on ? gx : -inf, on ? gy : inf, on ? gy : -inf};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        box[0] = fmin(box[0], __shfl_xor(box[0], o, 64));
        box[1] = fmax(box[1], __shfl_xor(box[1], o, 64));
        box[2] = fmin(box[2], __shfl_xor(box[2], o, 64));
        box[3] = fmax(box[3], __shfl_xor(box[3], o, 64));
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sbox[wave][i] = box[i];
    }
    double term[4] = {0.0, 0.0, 0.0, 0.0};  // keypoint distance, speed of the prediction, speed of the ground truth, velocity error
    double d2 = 0.0;
    if (on) {
        d2 = norm2(sub_rn(px, gx), sub_rn(py, gy));
        term[0] = sqrt(d2);
        if (t + 1 < T) {  // frame t also reads frame t + 1 of its own row
            const size_t next = base + (size_t)2 * K;
            const double vpx = sub_rn(pred[next + k], px), vpy = sub_rn(pred[next + K + k], py);
            const double vgx = sub_rn(gt[next + k], gx), vgy = sub_rn(gt[next + K + k], gy);
            term[1] = sqrt(norm2(vpx, vpy));
            term[2] = sqrt(norm2(vgx, vgy));
            term[3] = sqrt(norm2(sub_rn(vpx, vgx), sub_rn(vpy, vgy)));
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const double v = butterfly_sum(on && in_part(p, part) ? term[q] : 0.0);
            if (lane == 0) sred[wave][q * 4 + p] = v;
        }
    __syncthreads();
    const double side_x = sub_rn(fmax(sbox[0][1], sbox[1][1]), fmin(sbox[0][0], sbox[1][0]));
    const double side_y = sub_rn(fmax(sbox[0][3], sbox[1][3]), fmin(sbox[0][2], sbox[1][2]));
    const double s = fmax(side_x, side_y);
#pragma unroll
    for (int a = 0; a < kMaxAlphas; ++a) {
        const double thr = mul_rn(al.a[a], s);
        const bool hit = on && a < A && d2 <= mul_rn(thr, thr);  // on squares: no sqrt enters a count; a NaN on either side is no hit
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int n = __popcll(__ballot(hit && in_part(p, part)));
            if (lane == 0) scount[wave][a * 4 + p] = n;
        }
    }
    __syncthreads();
    int64_t* w = work + (size_t)rt * kFrameWords;
    if (k < 16) w[k] = bits_of(add_rn(sred[0][k], sred[1][k]));
    else if (k < 32) w[k] = (int64_t)(scount[0][k - 16] + scount[1][k - 16]);
}

// one wave per row: word c of the row's record from the per-frame partials, frames in order
__global__ __launch_bounds__(64) void clip_rows_reduce_kernel(const int64_t* __restrict__ work, int T, int64_t* __restrict__ rows) {
    const int c = threadIdx.x;
    const int64_t* w = work + (size_t)blockIdx.x * T * kFrameWords;
    double s = 0.0;
    int64_t h = 0;
    if (c < 16) {
        for (int t = 0; t < T; ++t) s = add_rn(s, double_of(w[(size_t)t * kFrameWords + c]));
    } else if (c >= 20 && c < 36) {
        for (int t = 0; t < T; ++t) h += w[(size_t)t * kFrameWords + c - 4];
    }
    const bool nonfinite = __ballot(c < 16 && !finite_d(s)) != 0;
    int64_t* out = rows + (size_t)blockIdx.x * kCols;
    if (c < 20) out[c] = bits_of(s);  // (div_sum: +0.0)
    else if (c < 36) out[c] = h;
    else if (c == kSeen || c == kCopies) out[c] = 1;
    else if (c == kNonfinite) out[c] = nonfinite ? 1 : 0;
    else if (c == kFrames) out[c] = T;
}

// one workgroup of 128 threads per (clip, frame): the m copies' keypoint k in lane k's own LDS column
__global__ __launch_bounds__(128) void clip_diversity_kernel(const double* __restrict__ pred, const uint8_t* __restrict__ parts, int B, int m,
                                                             int T, int K, double* __restrict__ divwork) {
    __shared__ double sx[kMaxCopies][kMaxK];
    __shared__ double sy[kMaxCopies][kMaxK];
    __shared__ double sred[2][4];
    const int bt = blockIdx.x, b = bt / T, t = bt % T, k = threadIdx.x, wave = k >> 6, lane = k & 63;
    const bool on = k < K;
    double acc = 0.0;
    int part = -1;
    if (on) {
        part = parts[k];
        for (int j = 0; j < m; ++j) {
            const size_t base = (((size_t)j * B + b) * T + t) * 2 * K;
            sx[j][k] = pred[base + k];
            sy[j][k] = pred[base + K + k];
        }
        for (int i = 0; i < m; ++i)
            for (int j = i + 1; j < m; ++j) acc = add_rn(acc, sqrt(norm2(sub_rn(sx[i][k], sx[j][k]), sub_rn(sy[i][k], sy[j][k]))));
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const double v = butterfly_sum(on && in_part(p, part) ? acc : 0.0);
        if (lane == 0) sred[wave][p] = v;
    }
    __syncthreads();
    if (k < 4) divwork[(size_t)bt * 4 + k] = add_rn(sred[0][k], sred[1][k]);
}

// one wave per clip of the call: word c of the clip's record, into row clip_index[b] of the table
__global__ __launch_bounds__(64) void clip_commit_kernel(const int64_t* __restrict__ rows, const double* __restrict__ divwork,
                                                         const int64_t* __restrict__ clip_index, int B, int m, int T,
                                                         int64_t* __restrict__ table, int64_t N) {
    const int b = blockIdx.x, c = threadIdx.x;
    double s = 0.0;
    int64_t h = 0;
    if (c < 16) {
        for (int j = 0; j < m; ++j) s = add_rn(s, double_of(rows[((size_t)j * B + b) * kCols + c]));
    } else if (c < 20) {
        if (divwork)
            for (int t = 0; t < T; ++t) s = add_rn(s, divwork[((size_t)b * T + t) * 4 + c - 16]);
    } else if (c < 36 || c == kNonfinite) {  // hit counts; the number of rows flagged nonfinite
        for (int j = 0; j < m; ++j) h += rows[((size_t)j * B + b) * kCols + c];
    }
    const bool nonfinite = __ballot((c < 20 && !finite_d(s)) || (c == kNonfinite && h != 0)) != 0;
    const int64_t idx = clip_index[b];
    if (idx < 0 || idx >= N) {  // writes nothing but the header's count
        if (c == 0) count_index_error(table, N, kCols);
        return;
    }
    int64_t* out = table + (size_t)idx * kCols;
    if (c < 20) out[c] = bits_of(s);
    else if (c < 36) out[c] = h;
    else if (c == kSeen) out[c] = 1;
    else if (c == kCopies) out[c] = m;
    else if (c == kNonfinite) out[c] = nonfinite ? 1 : 0;
    else if (c == kFrames) out[c] = T;
}

// one wave per chunk of 64 clips: word c of the chunk's partial, clips in index order, each from the lowest rank that has seen it
__global__ __launch_bounds__(64) void clip_epoch_chunk_kernel(Tables tb, int ranks, int64_t N, int64_t* __restrict__ work) {
    const int c = threadIdx.x;
    const int64_t n0 = (int64_t)blockIdx.x * kChunk, n1 = n0 + kChunk < N ? n0 + kChunk : N;
    double s = 0.0;
    int64_t h = 0;
    for (int64_t n = n0; n < n1; ++n) {
        const int64_t* rec = first_seen(tb, ranks, n, kCols, kSeen);
        if (!rec) continue;
        const bool bad = rec[kNonfinite] != 0;
        const int64_t copies = rec[kCopies], frames = rec[kFrames];
        if (c == kSeen) h += 1;
        else if (c == kNonfinite) h += bad ? 1 : 0;
        else if (!bad) {
            if (c < 20) s = add_rn(s, double_of(rec[c]));
            else if (c < 36) h += rec[c];
            else if (c == kCopies) h += copies * frames;
            else if (c == kFrames) h += copies * (frames - 1);
            else if (c == kPairFrames) h += copies * (copies - 1) / 2 * frames;
        }
    }
    if (c < kChunkWords) work[(size_t)blockIdx.x * kChunkWords + c] = c < 20 ? bits_of(s) : h;
}

// one wave: the chunk partials in order, then the divisions
__global__ __launch_bounds__(64) void clip_epoch_final_kernel(Tables tb, int ranks, int64_t N, const int64_t* __restrict__ work, int64_t chunks,
                                                              PartSizes ps, int A, int64_t* __restrict__ out) {
    __shared__ int64_t tot[kChunkWords];
    __shared__ int64_t errors;
    const int c = threadIdx.x;
    if (c < 20) tot[c] = bits_of(chunk_sum_f64(work, chunks, kChunkWords, c));
    else if (c < kChunkWords) tot[c] = chunk_sum_i64(work, chunks, kChunkWords, c);
    else if (c == kChunkWords) errors = index_errors(tb, ranks, N, kCols);
    __syncthreads();
    const int p = c & 3;
    const int64_t n_pos = tot[kCopies] * ps.n[p], n_vel = tot[kFrames] * ps.n[p], n_div = tot[kPairFrames] * ps.n[p];
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
    } else if (c < 36) {
        out[c] = bits_of(quotient(double_of(tot[16 + p]), n_div));
    } else if (c == 36) {
        out[c] = tot[kSeen];
    } else if (c == 37) {
        out[c] = tot[kNonfinite];
    } else if (c == 38) {
        out[c] = errors;
    } else if (c == 39) {
        out[c] = tot[kPairFrames];
    }
}

__global__ __launch_bounds__(256) void clip_sqrt_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = sqrt(x[i]);
}

}  // namespace

extern "C" int sdt_clip_metrics_rows_f64(const double* pred, const double* gt, const uint8_t* parts, const double* alphas, int num_alphas,
                                         int R, int T, int K, void* work, void* rows, void* stream) {
    SDT_CHECK_ARG(pred && gt && parts && alphas && work && rows, "null pointer");
    SDT_CHECK_ARG(K >= 1 && K <= kMaxK, "K outside [1, 128]");
    SDT_CHECK_ARG(R >= 1 && T >= 1 && (int64_t)R * T <= 0x7fffffff, "bad dims (R >= 1, T >= 1, R * T < 2^31)");
    SDT_CHECK_ARG(num_alphas >= 1 && num_alphas <= kMaxAlphas, "number of alphas outside [1, 4]");
    Alphas al;
    for (int a = 0; a < kMaxAlphas; ++a) al.a[a] = a < num_alphas ? alphas[a] : 0.0;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(clip_rows_frame_kernel, dim3(R * T), dim3(128), 0, s, pred, gt, parts, al, num_alphas, T, K, (int64_t*)work);
    hipLaunchKernelGGL(clip_rows_reduce_kernel, dim3(R), dim3(64), 0, s, (const int64_t*)work, T, (int64_t*)rows);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_clip_metrics_diversity_f64(const double* pred, const uint8_t* parts, int B, int m, int T, int K, double* divwork,
                                              void* stream) {
    SDT_CHECK_ARG(pred && parts && divwork, "null pointer");
    SDT_CHECK_ARG(K >= 1 && K <= kMaxK, "K outside [1, 128]");
    SDT_CHECK_ARG(m >= 2 && m <= kMaxCopies, "copies outside [2, 16]");
    SDT_CHECK_ARG(B >= 1 && T >= 1 && (int64_t)B * m * T <= 0x7fffffff, "bad dims (B >= 1, T >= 1, B * m * T < 2^31)");
    hipLaunchKernelGGL(clip_diversity_kernel, dim3(B * T), dim3(128), 0, (hipStream_t)stream, pred, parts, B, m, T, K, divwork);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_clip_metrics_commit(const void* rows, const double* divwork, const int64_t* clip_index, int B, int m, int T, void* table,
                                       int64_t N, void* stream) {
    SDT_CHECK_ARG(rows && clip_index && table, "null pointer");
    SDT_CHECK_ARG(m >= 1 && m <= kMaxCopies, "copies outside [1, 16]");
    SDT_CHECK_ARG((m == 1) == (divwork == nullptr), "the diversity partials come with two or more copies, and only then");
    SDT_CHECK_ARG(B >= 1 && T >= 1 && N >= 1 && (int64_t)B * m * T <= 0x7fffffff, "bad dims");
    hipLaunchKernelGGL(clip_commit_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const int64_t*)rows, divwork, clip_index, B, m, T,
                       (int64_t*)table, N);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_clip_metrics_epoch(const void* const* tables, int ranks, int64_t N, const int64_t* part_sizes, int num_alphas, void* work,
                                      void* out, void* stream) {
    SDT_CHECK_ARG(tables && part_sizes && work && out, "null pointer");
    SDT_CHECK_ARG(ranks >= 1 && ranks <= kMaxRanks, "tables outside [1, 64]");
    SDT_CHECK_ARG(N >= 1 && cdiv64(N, kChunk) <= 0x7fffffff, "bad number of clips");
    SDT_CHECK_ARG(num_alphas >= 1 && num_alphas <= kMaxAlphas, "number of alphas outside [1, 4]");
    Tables tb;
    PartSizes ps;
    SDT_CHECK_ARG(fill_tables(tb, tables, ranks), "null table");
    for (int p = 0; p < 4; ++p) {
        SDT_CHECK_ARG(part_sizes[p] >= 0 && part_sizes[p] <= kMaxK, "part size outside [0, 128]");
        ps.n[p] = part_sizes[p];
    }
    const int64_t chunks = cdiv64(N, kChunk);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(clip_epoch_chunk_kernel, dim3((unsigned)chunks), dim3(64), 0, s, tb, ranks, N, (int64_t*)work);
    hipLaunchKernelGGL(clip_epoch_final_kernel, dim3(1), dim3(64), 0, s, tb, ranks, N, (const int64_t*)work, chunks, ps, num_alphas,
                       (int64_t*)out);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_clip_metrics_sqrt_f64(const double* x, int64_t n, double* y, void* stream) {
    SDT_CHECK_ARG(x && y && n >= 1 && cdiv64(n, 256) <= 0x7fffffff, "bad argument");
    hipLaunchKernelGGL(clip_sqrt_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, (hipStream_t)stream, x, n, y);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
