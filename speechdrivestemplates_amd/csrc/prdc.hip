// Precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) between the pose-encoder features of the real and of
// the generated clips of a validation epoch (TEST.PRDC; include/sdt_hip.h states the layouts, DESIGN.md section 33 the contract;
// prdc.prdc_model / gather_model in Python are the same operations on whole distance matrices).
//
// d2(x, y) = the sum over c = 0 .. D-1, in that order from +0.0, of (x_c - y_c)^2, every subtract, multiply and add rounded on its own
// (sdt_exact::*_rn, no FMA): symmetric to the bit.  Every comparison is made on d2, so every output is an integer count, a d2 or a quotient of
// two integers: no square root, no transcendental function, no floating-point atomics.  Orders that could show in a result, all fixed:
//   the columns of a d2    serially (above);
//   compaction             a clip's position among the live clips is an exclusive prefix over the live flags in clip-index order;
//   the k smallest         a multiset: the sorted list a thread keeps, and the merge of the slices' lists, give the same k values in any order;
//   the nearest row        strict < along ascending positions inside a slice, then along ascending slices: the lowest position on a tie;
//   counts                 integers.
// The all-pairs kernels: one thread owns one query row in registers (D padded with +0.0 columns to 8, 16, 32 or 64: a padded column adds
// (0 - 0)^2 = +0.0, which leaves every partial sum's bits), the other set streams through LDS in tiles of 32 rows that every lane reads at the
// same address (a broadcast), and the streamed range is split over gridDim.y slices whose partial results a short kernel merges.
#include "record_table.h"

using namespace sdt_exact;
using namespace sdt_table;

namespace {

constexpr int kHdr = SDT_PRDC_HEADER_WORDS;  // words of a record before its features
constexpr int kSeenCopies = 0, kNonfinite = 1;
constexpr int kMaxCopies = 16, kMaxNeighbours = 16;
constexpr int kList = 16;  // the sorted list of a thread: kList - k entries of -inf, then the k smallest values seen
constexpr int64_t kMaxRows = 1 << 20;
constexpr int kMaxSlices = 4096;
constexpr int kTile = 32;  // streamed rows per LDS tile
constexpr int kThreads = 256;
constexpr int kCrossWords = 3;  // a slice's partial per query: ball count, bits of the smallest d2, its position
constexpr int kOutWords = SDT_PRDC_OUT_WORDS;

__device__ __forceinline__ double inf_d() { return __builtin_huge_val(); }

// ---- commit ------------------------------------------------------------------------------------------------------------------------------
// one wave per clip of the step: word w of the clip's features (the ground truth of copy 0, then the prediction of copy 0 .. m-1), widened
__global__ __launch_bounds__(64) void prdc_commit_kernel(const float* __restrict__ mu_p, const float* __restrict__ lv_p,
                                                         const float* __restrict__ mu_g, const float* __restrict__ lv_g,
                                                         const int64_t* __restrict__ clip_index, int B, int m, int Dh, int64_t* __restrict__ table,
                                                         int64_t N) {
    const int b = blockIdx.x, tid = threadIdx.x, D = 2 * Dh, cols = kHdr + D * (1 + m);
    const int64_t idx = clip_index[b];
    const bool inside = idx >= 0 && idx < N;
    int64_t* out = table + (size_t)(inside ? idx : 0) * cols;
    bool bad = false;
    for (int w = tid; w < D * (1 + m); w += 64) {
        const int set = w / D, c = w % D;
        const size_t row = set == 0 ? (size_t)b : (size_t)(set - 1) * B + b;  // copy j of clip b is row j * B + b
        const float* src = set == 0 ? (c < Dh ? mu_g : lv_g) : (c < Dh ? mu_p : lv_p);
        const double v = (double)src[row * Dh + (c < Dh ? c : c - Dh)];
        bad |= !finite_d(v);
        if (inside) out[kHdr + w] = bits_of(v);
    }
    const int nonfinite = __syncthreads_or(bad);
    if (tid != 0) return;
    if (!inside) {  // writes nothing but the header's count
        count_index_error(table, N, cols);
        return;
    }
    out[kSeenCopies] = m;
    out[kNonfinite] = nonfinite ? 1 : 0;
}

// ---- gather ------------------------------------------------------------------------------------------------------------------------------
// state[n]: 0 no rank has seen clip n, 1 live, 2 left out for a non-finite feature
__global__ __launch_bounds__(256) void prdc_state_kernel(Tables tb, int ranks, int64_t N, int cols, int64_t* __restrict__ state) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int64_t* rec = first_seen(tb, ranks, n, cols, kSeenCopies);
    state[n] = !rec ? 0 : rec[kNonfinite] != 0 ? 2 : 1;
}

// one workgroup: thread t counts the live clips of the t-th stretch of the index range, thread 0 turns the 1024 counts into exclusive prefixes
// in stretch order, then every thread numbers its stretch: pos[n] = the number of live clips before n (-1 for a clip that is not live)
__global__ __launch_bounds__(1024) void prdc_scan_kernel(Tables tb, int ranks, int64_t N, int cols, int m, int floor_pass,
                                                         const int64_t* __restrict__ state, int64_t* __restrict__ pos, int64_t* __restrict__ counts) {
    __shared__ int64_t live[1024], bad[1024];
    const int tid = threadIdx.x;
    const int64_t per = (N + 1023) / 1024, n0 = tid * per, n1 = n0 + per < N ? n0 + per : N;
    int64_t l = 0, b = 0;
    for (int64_t n = n0; n < n1; ++n) l += state[n] == 1, b += state[n] == 2;
    live[tid] = l, bad[tid] = b;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0, nb = 0;
        for (int i = 0; i < 1024; ++i) {
            const int64_t t = live[i];
            live[i] = run;
            run += t;
            nb += bad[i];
        }
        counts[0] = floor_pass ? (run + 1) / 2 : run;  // rows of the real set
        counts[1] = floor_pass ? run / 2 : run * m;    // rows of the generated set
        counts[2] = run + nb;                          // clips with a record
        counts[3] = nb;                                // of them left out as non-finite
        counts[4] = index_errors(tb, ranks, N, cols);
        counts[5] = run;
        counts[6] = counts[7] = 0;
    }
    __syncthreads();
    int64_t p = live[tid];
    for (int64_t n = n0; n < n1; ++n) pos[n] = state[n] == 1 ? p++ : -1;
}

// one wave per clip: the leading Du columns of its features into the dense matrices.  The usual pass: live clip p gives real row p and generated
// rows p m + j.  The floor pass: the ground truth of live clip p gives row p / 2 of the "real" set for an even p, of the "generated" set for an odd p.
__global__ __launch_bounds__(64) void prdc_scatter_kernel(Tables tb, int ranks, int D, int m, int Du, int floor_pass,
                                                          const int64_t* __restrict__ pos, double* __restrict__ real, double* __restrict__ gen,
                                                          int64_t* __restrict__ real_clip, int64_t* __restrict__ gen_clip,
                                                          int64_t* __restrict__ gen_copy) {
    const int64_t n = blockIdx.x, p = pos[n];
    if (p < 0) return;
    const int tid = threadIdx.x, cols = kHdr + D * (1 + m);
    const int64_t* rec = first_seen(tb, ranks, n, cols, kSeenCopies);
    if (!rec) return;  // (a live clip has one)
    if (floor_pass) {
        const bool odd = p & 1;
        double* dst = (odd ? gen : real) + (size_t)(p >> 1) * Du;
        for (int c = tid; c < Du; c += 64) dst[c] = double_of(rec[kHdr + c]);
        if (tid == 0) {
            (odd ? gen_clip : real_clip)[p >> 1] = n;
            if (odd) gen_copy[p >> 1] = 0;
        }
        return;
    }
    for (int w = tid; w < Du * (1 + m); w += 64) {
        const int set = w / Du, c = w % Du;
        const double v = double_of(rec[kHdr + set * D + c]);
        if (set == 0) real[(size_t)p * Du + c] = v;
        else gen[((size_t)p * m + set - 1) * Du + c] = v;
    }
    if (tid == 0) real_clip[p] = n;
    if (tid >= 1 && tid <= m) gen_clip[(size_t)p * m + tid - 1] = n, gen_copy[(size_t)p * m + tid - 1] = tid - 1;
}

// ---- the all-pairs kernels ---------------------------------------------------------------------------------------------------------------
template <int DP>
__device__ __forceinline__ double dist2(const double (&q)[DP], const double* __restrict__ t) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < DP; ++c) {
        const double d = sub_rn(q[c], t[c]);
        s = add_rn(s, mul_rn(d, d));
    }
    return s;
}

// v into the ascending list, its largest entry dropped (compile-time indices only: the list stays in registers)
__device__ __forceinline__ void list_insert(double (&kk)[kList], double v) {
    if (!(v < kk[kList - 1])) return;
#pragma unroll
    for (int i = kList - 1; i > 0; --i) kk[i] = v < kk[i - 1] ? kk[i - 1] : (v < kk[i] ? v : kk[i]);
    kk[0] = v < kk[0] ? v : kk[0];
}
__device__ __forceinline__ void list_init(double (&kk)[kList], int k) {
#pragma unroll
    for (int e = 0; e < kList; ++e) kk[e] = e < kList - k ? -inf_d() : inf_d();
}

// rows t0 .. t0 + nt of x (pitch D) into the tile, +0.0 in the padded columns and rows
template <int DP>
__device__ __forceinline__ void load_tile(double (*tile)[DP], const double* __restrict__ x, int64_t t0, int nt, int D) {
    for (int e = threadIdx.x; e < kTile * DP; e += kThreads) {
        const int r = e / DP, c = e % DP;
        tile[r][c] = r < nt && c < D ? x[(size_t)(t0 + r) * D + c] : 0.0;
    }
}
template <int DP>
__device__ __forceinline__ void load_query(double (&q)[DP], const double* __restrict__ x, int64_t i, bool active, int D) {
#pragma unroll
    for (int c = 0; c < DP; ++c) q[c] = active && c < D ? x[(size_t)i * D + c] : 0.0;
}

// slice blockIdx.y of the set against itself: per row its list over the slice's rows, itself left out by position
template <int DP>
__global__ __launch_bounds__(kThreads) void prdc_knn_kernel(const double* __restrict__ x, const int64_t* __restrict__ count, int64_t cap, int D,
                                                            int k, int slices, double* __restrict__ part) {
    __shared__ double tile[kTile][DP];
    const int64_t n = *count < cap ? *count : cap;
    if ((int64_t)blockIdx.x * kThreads >= n) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool active = i < n;
    const int64_t per = (n + slices - 1) / slices, s0 = blockIdx.y * per, s1 = s0 + per < n ? s0 + per : n;
    double q[DP], kk[kList];
    load_query<DP>(q, x, i, active, D);
    list_init(kk, k);
    for (int64_t t0 = s0; t0 < s1; t0 += kTile) {
        const int nt = s1 - t0 < kTile ? (int)(s1 - t0) : kTile;
        load_tile<DP>(tile, x, t0, nt, D);
        __syncthreads();
        if (active)
            for (int r = 0; r < nt; ++r) {
                const double d = dist2<DP>(q, tile[r]);
                if (t0 + r != i) list_insert(kk, d);
            }
        __syncthreads();
    }
    if (active) {
        double* out = part + ((size_t)blockIdx.y * cap + i) * kList;
#pragma unroll
        for (int e = 0; e < kList; ++e) out[e] = kk[e];
    }
}

// the k smallest of the slices' lists: radius[i] = the k-th smallest d2 to another row, +inf for a set of at most k rows
__global__ __launch_bounds__(kThreads) void prdc_knn_merge_kernel(const double* __restrict__ part, const int64_t* __restrict__ count, int64_t cap,
                                                                  int k, int slices, double* __restrict__ radius) {
    const int64_t n = *count < cap ? *count : cap, i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    double kk[kList];
    list_init(kk, k);
    for (int s = 0; s < slices; ++s) {
        const double* in = part + ((size_t)s * cap + i) * kList;
        for (int e = kList - k; e < kList; ++e) list_insert(kk, in[e]);
    }
    radius[i] = kk[kList - 1];
}

// slice blockIdx.y of the streamed set against the query rows: per query the number of streamed rows whose ball holds it (d2 <= their radius),
// the smallest d2 and the lowest position that has it
template <int DP>
__global__ __launch_bounds__(kThreads) void prdc_cross_kernel(const double* __restrict__ qx, const int64_t* __restrict__ qcount, int64_t qcap,
                                                              const double* __restrict__ sx, const int64_t* __restrict__ scount, int64_t scap,
                                                              const double* __restrict__ s_radius, int D, int slices, int64_t* __restrict__ part) {
    __shared__ double tile[kTile][DP];
    __shared__ double rad[kTile];
    const int64_t nq = *qcount < qcap ? *qcount : qcap, ns = *scount < scap ? *scount : scap;
    if ((int64_t)blockIdx.x * kThreads >= nq) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool active = i < nq;
    const int64_t per = (ns + slices - 1) / slices, s0 = blockIdx.y * per, s1 = s0 + per < ns ? s0 + per : ns;
    double q[DP];
    load_query<DP>(q, qx, i, active, D);
    int64_t balls = 0, arg = -1;
    double best = inf_d();
    for (int64_t t0 = s0; t0 < s1; t0 += kTile) {
        const int nt = s1 - t0 < kTile ? (int)(s1 - t0) : kTile;
        load_tile<DP>(tile, sx, t0, nt, D);
        if (threadIdx.x < kTile) rad[threadIdx.x] = (int)threadIdx.x < nt ? s_radius[t0 + threadIdx.x] : 0.0;
        __syncthreads();
        if (active)
            for (int r = 0; r < nt; ++r) {
                const double d = dist2<DP>(q, tile[r]);
                balls += d <= rad[r] ? 1 : 0;
                if (d < best) best = d, arg = t0 + r;
            }
        __syncthreads();
    }
    if (active) {
        int64_t* out = part + ((size_t)blockIdx.y * qcap + i) * kCrossWords;
        out[0] = balls, out[1] = bits_of(best), out[2] = arg;
    }
}

// the slices in ascending order: counts added, the smallest d2 by strict <, so the lowest position keeps a tie
__global__ __launch_bounds__(kThreads) void prdc_cross_merge_kernel(const int64_t* __restrict__ part, const int64_t* __restrict__ qcount,
                                                                    int64_t qcap, int slices, int64_t* __restrict__ ball_count,
                                                                    int64_t* __restrict__ nearest, double* __restrict__ nearest_d2) {
    const int64_t nq = *qcount < qcap ? *qcount : qcap, i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= nq) return;
    int64_t balls = 0, arg = -1;
    double best = inf_d();
    for (int s = 0; s < slices; ++s) {
        const int64_t* in = part + ((size_t)s * qcap + i) * kCrossWords;
        balls += in[0];
        const double d = double_of(in[1]);
        if (d < best) best = d, arg = in[2];
    }
    ball_count[i] = balls, nearest[i] = arg, nearest_d2[i] = best;
}

// ---- reduce ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double quotient_or_nan(int64_t num, int64_t den, bool err) {
    return err ? double_of(0x7ff8000000000000ll) : div_rn((double)num, (double)den);
}

// one workgroup: the flags of the real rows, the four counts (integers: any order gives the same sums) and the four divisions
__global__ __launch_bounds__(1024) void prdc_reduce_kernel(const int64_t* __restrict__ counts, int64_t real_cap, int64_t gen_cap, int k,
                                                           const double* __restrict__ r_real, const int64_t* __restrict__ gen_balls,
                                                           const int64_t* __restrict__ real_balls, const double* __restrict__ real_nearest_d2,
                                                           int64_t* __restrict__ covered, int64_t* __restrict__ recalled,
                                                           int64_t* __restrict__ out) {
    __shared__ int64_t sums[16][4];
    const int tid = threadIdx.x;
    const int64_t nr = counts[0] < real_cap ? counts[0] : real_cap, ng = counts[1] < gen_cap ? counts[1] : gen_cap;
    int64_t v[4] = {0, 0, 0, 0};  // precision, recall, density, coverage
    for (int64_t j = tid; j < ng; j += 1024) v[0] += gen_balls[j] > 0, v[2] += gen_balls[j];
    for (int64_t i = tid; i < nr; i += 1024) {
        const int64_t c = real_nearest_d2[i] <= r_real[i], r = real_balls[i] > 0;
        covered[i] = c, recalled[i] = r;
        v[1] += r, v[3] += c;
    }
    for (int e = 0; e < 4; ++e) {
        const int64_t s = butterfly_count(v[e]);
        if ((tid & 63) == 0) sums[tid >> 6][e] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int e = 0; e < 4; ++e) {
        v[e] = 0;
        for (int w = 0; w < 16; ++w) v[e] += sums[w][e];
    }
    const int64_t err = (nr <= k ? SDT_PRDC_ERR_REAL_ROWS : 0) | (ng <= k ? SDT_PRDC_ERR_GEN_ROWS : 0);
    out[0] = bits_of(quotient_or_nan(v[0], ng, err));
    out[1] = bits_of(quotient_or_nan(v[1], nr, err));
    out[2] = bits_of(quotient_or_nan(v[2], (int64_t)k * ng, err));
    out[3] = bits_of(quotient_or_nan(v[3], nr, err));
    for (int e = 0; e < 4; ++e) out[4 + e] = v[e];
    out[8] = nr, out[9] = ng, out[10] = k, out[11] = err;
    out[12] = counts[2], out[13] = counts[3], out[14] = counts[4], out[15] = 0;
}

bool sizes_ok(int64_t cap, int D) { return cap >= 1 && cap <= kMaxRows && D >= 1 && D <= kMaxD; }

}  // namespace

extern "C" int64_t sdt_prdc_cols(int D, int m) { return D < 1 || D > kMaxD || m < 1 || m > kMaxCopies ? 0 : kHdr + (int64_t)D * (1 + m); }

extern "C" int sdt_prdc_commit(const float* mu_pred, const float* logvar_pred, const float* mu_gt, const float* logvar_gt,
                               const int64_t* clip_index, int B, int m, int Dh, void* table, int64_t N, void* stream) {
    SDT_CHECK_ARG(mu_pred && logvar_pred && mu_gt && logvar_gt && clip_index && table, "null pointer");
    SDT_CHECK_SUPPORTED(m >= 1 && m <= kMaxCopies, "copies outside [1, 16]");
    SDT_CHECK_SUPPORTED(Dh >= 1 && 2 * Dh <= kMaxD, "feature width outside [1, 32] per half");
    SDT_CHECK_SUPPORTED(B >= 1 && B <= kMaxRows && N >= 1 && N <= kMaxRows, "bad dims (B and N in [1, 2^20])");
    hipLaunchKernelGGL(prdc_commit_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, mu_pred, logvar_pred, mu_gt, logvar_gt, clip_index, B, m,
                       Dh, (int64_t*)table, N);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_prdc_gather(const void* const* tables, int ranks, int64_t N, int D, int m, int dim_used, int floor_pass, void* work,
                               double* real, double* gen, int64_t* real_clip, int64_t* gen_clip, int64_t* gen_copy, int64_t* counts,
                               void* stream) {
    SDT_CHECK_ARG(tables && work && real && gen && real_clip && gen_clip && gen_copy && counts, "null pointer");
    SDT_CHECK_ARG(ranks >= 1 && ranks <= kMaxRanks, "tables outside [1, 64]");
    SDT_CHECK_SUPPORTED(m >= 1 && m <= kMaxCopies, "copies outside [1, 16]");
    SDT_CHECK_SUPPORTED(D >= 1 && D <= kMaxD && dim_used >= 1 && dim_used <= D, "D outside [1, 64] or dim_used outside [1, D]");
    SDT_CHECK_SUPPORTED(N >= 1 && N * m <= kMaxRows, "clips x copies outside [1, 2^20]");
    Tables tb;
    SDT_CHECK_ARG(fill_tables(tb, tables, ranks), "null table");
    const int cols = kHdr + D * (1 + m);
    int64_t *state = (int64_t*)work, *pos = state + N;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(prdc_state_kernel, dim3((unsigned)cdiv64(N, 256)), dim3(256), 0, s, tb, ranks, N, cols, state);
    hipLaunchKernelGGL(prdc_scan_kernel, dim3(1), dim3(1024), 0, s, tb, ranks, N, cols, m, floor_pass ? 1 : 0, (const int64_t*)state, pos, counts);
    hipLaunchKernelGGL(prdc_scatter_kernel, dim3((unsigned)N), dim3(64), 0, s, tb, ranks, D, m, dim_used, floor_pass ? 1 : 0,
                       (const int64_t*)pos, real, gen, real_clip, gen_clip, gen_copy);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int64_t sdt_prdc_slices(int64_t queries, int64_t streamed) {
    if (queries < 1 || streamed < 1) return 1;
    const int64_t fill = cdiv64(512, cdiv64(queries, kThreads)), most = cdiv64(streamed, 4 * kTile);  // two workgroups per CU, four tiles a slice
    return std::max<int64_t>(1, std::min<int64_t>(std::min(fill, most), kMaxSlices));
}

#define PRDC_BY_WIDTH(KERNEL, ...)                                                              \
    do {                                                                                        \
        if (D <= 8) hipLaunchKernelGGL(KERNEL<8>, grid, dim3(kThreads), 0, s, __VA_ARGS__);       \
        else if (D <= 16) hipLaunchKernelGGL(KERNEL<16>, grid, dim3(kThreads), 0, s, __VA_ARGS__); \
        else if (D <= 32) hipLaunchKernelGGL(KERNEL<32>, grid, dim3(kThreads), 0, s, __VA_ARGS__); \
        else hipLaunchKernelGGL(KERNEL<64>, grid, dim3(kThreads), 0, s, __VA_ARGS__);             \
    } while (0)

extern "C" int sdt_prdc_knn(const double* x, const int64_t* count, int64_t cap, int D, int k, int slices, void* part, int64_t part_words,
                            double* radius, void* stream) {
    SDT_CHECK_ARG(x && count && part && radius, "null pointer");
    SDT_CHECK_SUPPORTED(sizes_ok(cap, D), "rows outside [1, 2^20] or D outside [1, 64]");
    SDT_CHECK_SUPPORTED(k >= 1 && k <= kMaxNeighbours, "k outside [1, 16]");
    SDT_CHECK_SUPPORTED(slices >= 1 && slices <= kMaxSlices, "slices outside [1, 4096]");
    SDT_CHECK_ARG(part_words >= (int64_t)slices * cap * kList, "the workspace is smaller than slices x rows x 16 words");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv64(cap, kThreads), (unsigned)slices);
    PRDC_BY_WIDTH(prdc_knn_kernel, x, count, cap, D, k, slices, (double*)part);
    hipLaunchKernelGGL(prdc_knn_merge_kernel, dim3(grid.x), dim3(kThreads), 0, s, (const double*)part, count, cap, k, slices, radius);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_prdc_cross(const double* q, const int64_t* qcount, int64_t qcap, const double* sx, const int64_t* scount, int64_t scap,
                              const double* s_radius, int D, int slices, void* part, int64_t part_words, int64_t* ball_count, int64_t* nearest,
                              double* nearest_d2, void* stream) {
    SDT_CHECK_ARG(q && qcount && sx && scount && s_radius && part && ball_count && nearest && nearest_d2, "null pointer");
    SDT_CHECK_SUPPORTED(sizes_ok(qcap, D) && sizes_ok(scap, D), "rows outside [1, 2^20] or D outside [1, 64]");
    SDT_CHECK_SUPPORTED(slices >= 1 && slices <= kMaxSlices, "slices outside [1, 4096]");
    SDT_CHECK_ARG(part_words >= (int64_t)slices * qcap * kCrossWords, "the workspace is smaller than slices x query rows x 3 words");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv64(qcap, kThreads), (unsigned)slices);
    PRDC_BY_WIDTH(prdc_cross_kernel, q, qcount, qcap, sx, scount, scap, s_radius, D, slices, (int64_t*)part);
    hipLaunchKernelGGL(prdc_cross_merge_kernel, dim3(grid.x), dim3(kThreads), 0, s, (const int64_t*)part, qcount, qcap, slices, ball_count,
                       nearest, nearest_d2);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_prdc_reduce(const int64_t* counts, int64_t real_cap, int64_t gen_cap, int k, const double* r_real, const int64_t* gen_balls,
                               const int64_t* real_balls, const double* real_nearest_d2, int64_t* covered, int64_t* recalled, int64_t* out,
                               void* stream) {
    SDT_CHECK_ARG(counts && r_real && gen_balls && real_balls && real_nearest_d2 && covered && recalled && out, "null pointer");
    SDT_CHECK_SUPPORTED(real_cap >= 1 && real_cap <= kMaxRows && gen_cap >= 1 && gen_cap <= kMaxRows, "rows outside [1, 2^20]");
    SDT_CHECK_SUPPORTED(k >= 1 && k <= kMaxNeighbours, "k outside [1, 16]");
    static_assert(kOutWords == 16, "the epoch vector has 16 words");
    hipLaunchKernelGGL(prdc_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, counts, real_cap, gen_cap, k, r_real, gen_balls,
                       real_balls, real_nearest_d2, covered, recalled, out);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
