// Speech-gesture synchrony: audio onsets, motion beats and their matching (TEST.SYNC_METRICS; include/sdt_hip.h states the record layouts,
// DESIGN.md section 24 the contract; sync_metrics.onsets_model / beats_model / match_model / sync_model / epoch_model in Python are the same
// operations in the same order).  All times are integers in ticks of 1/300 s: an audio hop of 160 samples is 3 ticks, a pose frame 20.
//
// Orders of summation, all fixed:
//   envelope         one wave per audio frame of 320 samples; lane l adds the squares of samples l, l + 64, .., l + 256 in ascending order (the
//                    first product starts the sum), then the xor butterfly v += shfl_xor(v, o) for o = 32, 16, 8, 4, 2, 1;
//   onset mean       o[n - 15 .. n + 15] clipped to the clip, ascending, from +0.0;
//   speed            lane k holds keypoint k's term (+0.0 outside the part and for k >= K); butterfly per wave, then wave 0 + wave 1
//                    (as csrc/clip_metrics.hip forms speed_pred);
//   beat mean, align frames in ascending order from +0.0.  The lanes of a wave hold 64 consecutive frames and every lane adds the 64 values in
//                    lane order; a lane without a term holds +0.0, which leaves a sum that started at +0.0 and has only terms >= 0 unchanged;
//   over the copies  j = 0 .. m-1; over the clips: chunks of 64 clips in index order, then the chunk partials in order.
// Every multiply, add, subtract and divide goes through sdt_exact (no FMA); counts and distances are integers.  No floating-point atomics: the
// only atomic is the integer count of clip indices outside the table.
#include "record_table.h"

using namespace sdt_exact;
using namespace sdt_table;

namespace {

constexpr int kHop = 160;                     // samples between audio frames (3 ticks); a frame is two hops long
constexpr int kHalf = 15;                     // the onset mean runs over n - 15 .. n + 15
constexpr int kGap = 8;                       // accepted onsets are at least this many frames apart
constexpr int kDmax = 150;                    // distances are capped at 150 ticks (0.5 s); the Gaussian table has kDmax + 1 entries
constexpr int kTile = 4096;                   // frames per tile of the refractory pass: 64 candidate masks in LDS
constexpr int kRowCols = SDT_SYNC_ROW_COLS;   // words of a row record
constexpr int kCols = SDT_SYNC_COLS;          // words of a clip record
constexpr int kOutCols = SDT_SYNC_OUT_COLS;   // words of the epoch vector
constexpr int kMaxK = 128;
constexpr int kMaxCopies = 16;
constexpr int kMaxHops = 1 << 28;             // 3 n + 3 stays an int32
constexpr int kMaxFrames = 1 << 24;
// words of a clip record (and of a chunk partial): float64 [0,4) align of the prediction, [4,8) of the ground truth; int64 [8,24) beats, hits,
// dsum, covered of the prediction per part, [24,40) of the ground truth
constexpr int kOnsets = 40, kSeen = 41, kCopies = 42, kNonfinite = 43, kFrames = 44, kHops = 45;
// words of a row record: float64 [0,4) align; int64 [4,20) beats, hits, dsum, covered per part
constexpr int kRowOnsets = 20, kRowNonfinite = 21, kRowFrames = 22;

// the value lane i holds (i is the same in every lane)
__device__ __forceinline__ double lane_value(double v, int i) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), i), hi = __builtin_amdgcn_readlane(__double2hiint(v), i);
    return __hiloint2double(hi, lo);
}
// s + the 64 lanes' values in lane order
__device__ __forceinline__ double add_lanes_in_order(double s, double v) {
#pragma unroll
    for (int i = 0; i < 64; ++i) s = add_rn(s, lane_value(v, i));
    return s;
}

// four waves per workgroup, one wave per audio frame; blockIdx.y is the clip
__global__ __launch_bounds__(256) void sync_envelope_kernel(const float* __restrict__ audio, int64_t L, int Nf, double* __restrict__ env) {
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + wave;
    if (n >= Nf) return;  // (the whole wave; nothing below waits for another wave)
    const float* x = audio + (size_t)b * L;
    const int64_t first = (int64_t)n * kHop + lane;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int64_t i = first + 64 * j;
        const double v = i < L ? (double)x[i] : 0.0;  // a sample at or past L reads as 0.0
        const double sq = mul_rn(v, v);
        acc = j == 0 ? sq : add_rn(acc, sq);
    }
    acc = butterfly_sum(acc);
    if (lane == 0) env[(size_t)b * Nf + n] = sqrt(acc);
}

// one workgroup per clip: onset strength and the largest envelope, then tile by tile the candidate masks (all threads) and the refractory pass
// over the masks (thread 0, which visits set bits only)
__global__ __launch_bounds__(256) void sync_onsets_kernel(const double* __restrict__ env, int Nf, double delta, double floor_frac,
                                                          double* __restrict__ strength, int32_t* __restrict__ ticks, int64_t cap,
                                                          int64_t* __restrict__ info) {
    __shared__ double smax[4];
    __shared__ unsigned long long smask[kTile / 64];
    __shared__ int scarry[2];  // the last accepted frame, the number of accepted onsets
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const double* e = env + (size_t)b * Nf;
    double* o = strength + (size_t)b * Nf;
    double mx = 0.0;
    bool bad = false;
    for (int n = tid; n < Nf; n += 256) {
        const double en = e[n];
        bad |= !finite_d(en);
        mx = fmax(mx, en);
        double on = 0.0;
        if (n > 0) {
            const double d = sub_rn(en, e[n - 1]);
            on = d > 0.0 ? d : 0.0;  // (a NaN difference is no rise)
        }
        o[n] = on;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) mx = fmax(mx, __shfl_xor(mx, s, 64));
    if (lane == 0) smax[wave] = mx;
    if (tid == 0) {
        scarry[0] = -kGap;
        scarry[1] = 0;
    }
    const int anybad = __syncthreads_or(bad ? 1 : 0);  // (also makes o[] and smax[] visible to the workgroup)
    const double emax = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
    const double floor_thr = mul_rn(floor_frac, emax);
    int32_t* out = ticks + (size_t)b * cap;
    for (int t0 = 0; t0 < Nf; t0 += kTile) {
        for (int g = wave; g < kTile / 64; g += 4) {
            const int n = t0 + g * 64 + lane;
            bool cand = false;
            if (n >= 1 && n <= Nf - 2) {
                const double v = o[n];
                if (v > o[n - 1] && v >= o[n + 1] && v > floor_thr) {
                    const int lo = n - kHalf < 0 ? 0 : n - kHalf, hi = n + kHalf > Nf - 1 ? Nf - 1 : n + kHalf;
                    double s = 0.0;
                    for (int i = lo; i <= hi; ++i) s = add_rn(s, o[i]);
                    cand = v > mul_rn(delta, div_rn(s, (double)(hi - lo + 1)));
                }
            }
            const unsigned long long m = __ballot(cand);
            if (lane == 0) smask[g] = m;
        }
        __syncthreads();
        if (tid == 0) {
            int last = scarry[0], cnt = scarry[1];
            for (int g = 0; g < kTile / 64; ++g) {
                unsigned long long m = smask[g];
                while (m) {
                    const int n = t0 + g * 64 + __ffsll((long long)m) - 1;
                    m &= m - 1;
                    if (n - last >= kGap) {
                        if (cnt < cap) out[cnt] = 3 * n + 3;
                        ++cnt;
                        last = n;
                    }
                }
            }
            scarry[0] = last;
            scarry[1] = cnt;
        }
        __syncthreads();
    }
    if (tid == 0) {
        info[(size_t)b * 2] = scarry[1];
        info[(size_t)b * 2 + 1] = anybad ? 1 : 0;
    }
}

// one workgroup of 128 threads per (row, t < T - 1); thread k handles keypoint k
__global__ __launch_bounds__(128) void sync_speed_kernel(const double* __restrict__ poses, const uint8_t* __restrict__ parts, int T, int K,
                                                         double* __restrict__ speed) {
    __shared__ double sred[2][4];
    const int rt = blockIdx.x, r = rt / (T - 1), t = rt % (T - 1), k = threadIdx.x, wave = k >> 6, lane = k & 63;
    const bool on = k < K;
    const size_t base = ((size_t)r * T + t) * 2 * K, next = base + (size_t)2 * K;
    double term = 0.0;
    int part = -1;
    if (on) {
        term = sqrt(norm2(sub_rn(poses[next + k], poses[base + k]), sub_rn(poses[next + K + k], poses[base + K + k])));
        part = parts[k];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const double v = butterfly_sum(on && in_part(p, part) ? term : 0.0);
        if (lane == 0) sred[wave][p] = v;
    }
    __syncthreads();
    if (k < 4) speed[(size_t)rt * 4 + k] = add_rn(sred[0][k], sred[1][k]);
}

// the distance of ``tick`` to the nearest of the na ascending onset ticks, capped at kDmax (kDmax without an onset)
__device__ __forceinline__ int nearest(const int32_t* __restrict__ a, int na, int tick) {
    int lo = 0, hi = na;  // the first index with a[i] >= tick
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < tick) lo = mid + 1;
        else hi = mid;
    }
    int d = kDmax;
    if (lo < na && a[lo] - tick < d) d = a[lo] - tick;
    if (lo > 0 && tick - a[lo - 1] < d) d = tick - a[lo - 1];
    return d;
}

// one workgroup per row, wave p handles part p: the mean speed, the beats, their nearest onsets, and which onsets a beat covers
__global__ __launch_bounds__(256) void sync_match_kernel(const double* __restrict__ speed, int T, int B, const int32_t* __restrict__ ticks,
                                                         int64_t cap, const int64_t* __restrict__ info, const double* __restrict__ gauss, int tol,
                                                         double gamma, uint8_t* __restrict__ beat, int64_t* __restrict__ rows) {
    __shared__ int64_t srec[4][5];
    __shared__ int sbad[4];
    const int r = blockIdx.x, p = threadIdx.x >> 6, lane = threadIdx.x & 63, b = r % B;
    const int32_t* a = ticks + (size_t)b * cap;
    const int64_t onsets = info[(size_t)b * 2];
    const int na = (int)(onsets < cap ? onsets : cap);
    const int Tm1 = T - 1;
    const double* s = speed + (size_t)r * Tm1 * 4 + p;  // s[4 t]: the speed of part p between frames t and t + 1
    uint8_t* flag = beat + ((size_t)r * 4 + p) * T;
    double sum = 0.0;
    for (int t0 = 0; t0 < Tm1; t0 += 64) {
        const int t = t0 + lane;
        sum = add_lanes_in_order(sum, t < Tm1 ? s[(size_t)t * 4] : 0.0);
    }
    const double thr = Tm1 > 0 ? mul_rn(gamma, div_rn(sum, (double)Tm1)) : 0.0;
    int64_t beats = 0, hits = 0, dsum = 0;
    double align = 0.0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        bool is_beat = false;
        if (t >= 1 && t <= T - 3) {
            const double v = s[(size_t)t * 4];
            is_beat = v > s[(size_t)(t - 1) * 4] && v >= s[(size_t)(t + 1) * 4] && v > thr;
        }
        if (t < T) flag[t] = is_beat ? 1 : 0;
        double g = 0.0;
        if (is_beat) {
            const int d = nearest(a, na, 20 * t + 10);
            g = gauss[d];
            beats += 1;
            hits += d <= tol ? 1 : 0;
            dsum += d;
        }
        align = add_lanes_in_order(align, g);
    }
    beats = butterfly_count(beats);
    hits = butterfly_count(hits);
    dsum = butterfly_count(dsum);
    __syncthreads();  // (the flags of this wave are read back below)
    int64_t covered = 0;
    for (int i = lane; i < na; i += 64) {
        const int lo = a[i] - tol - 10, hi = a[i] + tol - 10;  // beats t with lo <= 20 t <= hi
        int t_lo = lo <= 0 ? 0 : (lo + 19) / 20, t_hi = hi < 0 ? -1 : hi / 20;
        if (t_lo < 1) t_lo = 1;
        if (t_hi > T - 3) t_hi = T - 3;
        bool any = false;
        for (int t = t_lo; t <= t_hi; ++t) any |= flag[t] != 0;
        covered += any ? 1 : 0;
    }
    covered = butterfly_count(covered);
    if (lane == 0) {
        srec[p][0] = bits_of(align);
        srec[p][1] = beats;
        srec[p][2] = hits;
        srec[p][3] = dsum;
        srec[p][4] = covered;
        sbad[p] = finite_d(sum) ? 0 : 1;
    }
    __syncthreads();
    const int c = threadIdx.x;
    int64_t* out = rows + (size_t)r * kRowCols;
    if (c < 4) out[c] = srec[c][0];
    else if (c < 20) out[c] = srec[c & 3][(c >> 2)];
    else if (c == kRowOnsets) out[c] = onsets;
    else if (c == kRowNonfinite) out[c] = (sbad[0] | sbad[1] | sbad[2] | sbad[3] | (info[(size_t)b * 2 + 1] != 0 ? 1 : 0));
    else if (c == kRowFrames) out[c] = T;
    else if (c < kRowCols) out[c] = 0;
}

// one wave per clip of the call: word c of the clip's record, into row clip_index[b] of the table
__global__ __launch_bounds__(64) void sync_commit_kernel(const int64_t* __restrict__ rows_pred, const int64_t* __restrict__ rows_gt,
                                                         const int64_t* __restrict__ clip_index, int B, int m, int T, int64_t hops,
                                                         int64_t* __restrict__ table, int64_t N) {
    const int b = blockIdx.x, c = threadIdx.x;
    double s = 0.0;
    int64_t h = 0;
    const int64_t* src = c < 4 || (c >= 8 && c < 24) ? rows_pred : rows_gt;       // (words [4,8) and [24,40) are the ground truth's)
    const int w = c < 4 ? c : c < 8 ? c - 4 : c < 24 ? c - 4 : c - 20;             // the word of the row record behind word c < 40
    if (c < 8) {
        if (src)
            for (int j = 0; j < m; ++j) s = add_rn(s, double_of(src[((size_t)j * B + b) * kRowCols + w]));
    } else if (c < 40) {
        if (src)
            for (int j = 0; j < m; ++j) h += src[((size_t)j * B + b) * kRowCols + w];
    } else if (c == kOnsets) {
        for (int j = 0; j < m; ++j) h += rows_pred[((size_t)j * B + b) * kRowCols + kRowOnsets];
    } else if (c == kNonfinite) {
        for (int j = 0; j < m; ++j) {
            h += rows_pred[((size_t)j * B + b) * kRowCols + kRowNonfinite];
            if (rows_gt) h += rows_gt[((size_t)j * B + b) * kRowCols + kRowNonfinite];
        }
    }
    const bool nonfinite = __ballot((c < 8 && !finite_d(s)) || (c == kNonfinite && h != 0)) != 0;
    const int64_t idx = clip_index[b];
    if (idx < 0 || idx >= N) {  // writes nothing but the header's count
        if (c == 0) count_index_error(table, N, kCols);
        return;
    }
    if (c >= kCols) return;
    int64_t* out = table + (size_t)idx * kCols;
    if (c < 8) out[c] = bits_of(s);
    else if (c <= kOnsets) out[c] = h;
    else if (c == kSeen) out[c] = 1;
    else if (c == kCopies) out[c] = m;
    else if (c == kNonfinite) out[c] = nonfinite ? 1 : 0;
    else if (c == kFrames) out[c] = T;
    else if (c == kHops) out[c] = hops;
    else out[c] = 0;
}

// one wave per chunk of 64 clips: word c of the chunk's partial, clips in index order, each from the lowest rank that has seen it
__global__ __launch_bounds__(64) void sync_epoch_chunk_kernel(Tables tb, int ranks, int64_t N, int64_t* __restrict__ work) {
    const int c = threadIdx.x;
    const int64_t n0 = (int64_t)blockIdx.x * kChunk, n1 = n0 + kChunk < N ? n0 + kChunk : N;
    double s = 0.0;
    int64_t h = 0;
    for (int64_t n = n0; n < n1; ++n) {
        const int64_t* rec = first_seen(tb, ranks, n, kCols, kSeen);
        if (!rec) continue;
        const bool bad = rec[kNonfinite] != 0;
        if (c == kSeen) h += 1;
        else if (c == kNonfinite) h += bad ? 1 : 0;
        else if (!bad) {
            if (c < 8) s = add_rn(s, double_of(rec[c]));
            else if (c <= kOnsets) h += rec[c];
            else if (c == kCopies) h += rec[kCopies] * rec[kFrames];
            else if (c == kHops) h += rec[kCopies] * rec[kHops];
        }
    }
    if (c < kCols) work[(size_t)blockIdx.x * kCols + c] = c < 8 ? bits_of(s) : h;
}

// one wave: the chunk partials in order, then the divisions
__global__ __launch_bounds__(64) void sync_epoch_final_kernel(Tables tb, int ranks, int64_t N, const int64_t* __restrict__ work, int64_t chunks,
                                                              int64_t* __restrict__ out) {
    __shared__ int64_t tot[kCols];
    __shared__ int64_t errors;
    const int c = threadIdx.x;
    if (c < 8) tot[c] = bits_of(chunk_sum_f64(work, chunks, kCols, c));
    else if (c < kCols) tot[c] = chunk_sum_i64(work, chunks, kCols, c);
    else if (c == kCols) errors = index_errors(tb, ranks, N, kCols);
    __syncthreads();
    if (c >= kOutCols) return;
    const int p = (c & 1) ? 3 : 0, q = c >> 1;  // value q for all (even words) and for hands (odd words)
    const int64_t beats_pred = tot[8 + p], beats_gt = tot[24 + p];
    double v = 0.0;
    if (q == 0) v = quotient((double)tot[12 + p], beats_pred);                            // sync_precision
    else if (q == 1) v = quotient((double)tot[28 + p], beats_gt);                         // sync_precision_gt
    else if (q == 2) v = quotient((double)tot[20 + p], tot[kOnsets]);                     // sync_recall
    else if (q == 3) v = quotient((double)tot[36 + p], tot[kOnsets]);                     // sync_recall_gt
    else if (q == 4) v = quotient(mul_rn((double)tot[16 + p], 1000.0 / 300.0), beats_pred);  // sync_offset_ms
    else if (q == 5) v = quotient(double_of(tot[p]), beats_pred);                         // beat_align
    else if (q == 6) v = quotient(double_of(tot[4 + p]), beats_gt);                       // beat_align_gt
    else if (q == 7) v = quotient(mul_rn((double)beats_pred, 15.0), tot[kCopies]);        // beats_per_s
    else if (q == 8) v = quotient(mul_rn((double)beats_gt, 15.0), tot[kCopies]);          // beats_per_s_gt
    else if (c == 18) v = quotient(mul_rn((double)tot[kOnsets], 100.0), tot[kHops]);      // onsets_per_s
    if (c < 20) out[c] = bits_of(v);
    else if (c == 20) out[c] = tot[kSeen];
    else if (c == 21) out[c] = tot[kNonfinite];
    else if (c == 22) out[c] = errors;
    else out[c] = 0;
}

int64_t hops_of(int64_t L) { return L / kHop; }
int64_t align8(int64_t n) { return (n + 7) / 8 * 8; }

}  // namespace

extern "C" int64_t sdt_sync_onset_capacity(int64_t L) { return L < 0 || hops_of(L) > kMaxHops ? -1 : hops_of(L) / kGap + 1; }

extern "C" int64_t sdt_sync_workspace_bytes(int B, int64_t L, int R, int T) {
    if (B < 0 || R < 0 || L < 0 || T < 0 || hops_of(L) > kMaxHops || T > kMaxFrames) return -1;
    const int64_t onsets = (int64_t)B * hops_of(L) * 2 * 8;                                             // envelope, strength
    const int64_t rows = (int64_t)R * (T > 0 ? T - 1 : 0) * 4 * 8 + align8((int64_t)R * 4 * T);         // speeds, beat flags
    const int64_t n = onsets > rows ? onsets : rows;
    return n > 8 ? n : 8;
}

extern "C" int sdt_sync_onsets_f64(const float* audio, int B, int64_t L, double delta, double floor_frac, void* work, int32_t* ticks, int64_t cap,
                                   int64_t* info, void* stream) {
    SDT_CHECK_ARG(L >= 0 && hops_of(L) <= kMaxHops, "L outside [0, 160 * 2^28]");
    SDT_CHECK_ARG(audio && work && ticks && info, "null pointer");
    SDT_CHECK_ARG(B >= 1 && B <= 65535, "clips outside [1, 65535]");
    SDT_CHECK_ARG(cap >= sdt_sync_onset_capacity(L), "the tick list is shorter than sdt_sync_onset_capacity(L)");
    const int Nf = (int)hops_of(L);
    SDT_CHECK_ARG((int64_t)B * Nf <= 0x7fffffff, "B * (L / 160) >= 2^31");
    double* env = (double*)work;
    double* strength = env + (size_t)B * Nf;
    hipStream_t s = (hipStream_t)stream;
    if (Nf > 0) hipLaunchKernelGGL(sync_envelope_kernel, dim3(cdiv(Nf, 4), B), dim3(256), 0, s, audio, L, Nf, env);
    hipLaunchKernelGGL(sync_onsets_kernel, dim3(B), dim3(256), 0, s, (const double*)env, Nf, delta, floor_frac, strength, ticks, cap, info);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_sync_rows_f64(const double* poses, const uint8_t* parts, int R, int T, int K, int B, const int32_t* ticks, int64_t cap,
                                 const int64_t* info, const double* gauss, int tol, double gamma, void* work, void* rows, void* stream) {
    SDT_CHECK_ARG(K >= 1 && K <= kMaxK, "K outside [1, 128]");
    SDT_CHECK_ARG(tol >= 1 && tol <= kDmax, "tolerance outside [1, 150] ticks");
    SDT_CHECK_ARG(T >= 1 && T <= kMaxFrames, "T outside [1, 2^24]");
    SDT_CHECK_ARG(poses && parts && ticks && info && gauss && work && rows, "null pointer");
    SDT_CHECK_ARG(R >= 1 && B >= 1 && R % B == 0 && (int64_t)R * T <= 0x7fffffff, "bad dims (R a multiple of B >= 1, R * T < 2^31)");
    SDT_CHECK_ARG(cap >= 1, "empty tick list");
    double* speed = (double*)work;
    uint8_t* beat = (uint8_t*)(speed + (size_t)R * (T - 1) * 4);
    hipStream_t s = (hipStream_t)stream;
    if (T > 1) hipLaunchKernelGGL(sync_speed_kernel, dim3(R * (T - 1)), dim3(128), 0, s, poses, parts, T, K, speed);
    hipLaunchKernelGGL(sync_match_kernel, dim3(R), dim3(256), 0, s, (const double*)speed, T, B, ticks, cap, info, gauss, tol, gamma, beat,
                       (int64_t*)rows);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_sync_commit(const void* rows_pred, const void* rows_gt, const int64_t* clip_index, int B, int m, int T, int64_t L, void* table,
                               int64_t N, void* stream) {
    SDT_CHECK_ARG(rows_pred && clip_index && table, "null pointer");
    SDT_CHECK_ARG(m >= 1 && m <= kMaxCopies, "copies outside [1, 16]");
    SDT_CHECK_ARG(L >= 0 && hops_of(L) <= kMaxHops, "L outside [0, 160 * 2^28]");
    SDT_CHECK_ARG(B >= 1 && T >= 1 && N >= 1 && (int64_t)B * m * T <= 0x7fffffff, "bad dims");
    hipLaunchKernelGGL(sync_commit_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const int64_t*)rows_pred, (const int64_t*)rows_gt,
                       clip_index, B, m, T, hops_of(L), (int64_t*)table, N);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_sync_epoch(const void* const* tables, int ranks, int64_t N, void* work, void* out, void* stream) {
    SDT_CHECK_ARG(tables && work && out, "null pointer");
    SDT_CHECK_ARG(ranks >= 1 && ranks <= kMaxRanks, "tables outside [1, 64]");
    SDT_CHECK_ARG(N >= 1 && cdiv64(N, kChunk) <= 0x7fffffff, "bad number of clips");
    Tables tb;
    SDT_CHECK_ARG(fill_tables(tb, tables, ranks), "null table");
    const int64_t chunks = cdiv64(N, kChunk);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sync_epoch_chunk_kernel, dim3((unsigned)chunks), dim3(64), 0, s, tb, ranks, N, (int64_t*)work);
    hipLaunchKernelGGL(sync_epoch_final_kernel, dim3(1), dim3(64), 0, s, tb, ranks, N, (const int64_t*)work, chunks, (int64_t*)out);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
