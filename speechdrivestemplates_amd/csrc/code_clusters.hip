// Clusters of the template-code table and the table row that stands for each (code_clusters.py): k-means on the
// (N, D) fp32 clip-code table, seeded by k-means++ or by farthest-point traversal, iterated by Lloyd's rule, and a final pass that numbers
// the clusters by descending size and names each cluster's medoid row.  The file the tool writes is what the two demo modes of the
// reference consume (pose2pose.py:50-56 DEMO.CODE_PATH / DEMO.MULTIPLE, voice2pose.py:107-117 DEMO.CODE_INDEX / CODE_INDEX_B).
// Rows are grouped in CHUNKS of 1024 consecutive rows; every floating-point sum over rows runs rows ascending inside a chunk from +0.0,
// then chunks ascending, so no result depends on a grid.  Stages:
//   seed_update : m[n] = min(m[n], d2(x[n], x[seed])); one workgroup per chunk, one thread per row of a 128-row tile staged in LDS; the
//                 chunk's ordered sum of m, its (max m, lowest row) pair and its last row with m > 0 go to the workspace.
//   seed_pick   : one workgroup.  k-means++: ordered scan of the chunk sums, the first chunk whose running sum passes r = u T, then an
//                 ordered walk of that chunk.  farthest: the exact (m, row) maximum of the chunk pairs.
//   assign      : label[n] = argmin over c of d2(x[n], centre[c]); a tile of rows in LDS (pitch D | 1 floats), the k centres in LDS as
//                 float64 (every lane reads one address: a broadcast), one thread per row, four centres at a time for four independent
//                 chains; the count of changed labels by integer atomics.
//   update      : one workgroup per chunk, threads own (cluster, d) pairs and walk the chunk's rows ascending; chunk partials to the
//                 workspace; a second kernel adds them chunks ascending and divides by the integer count.
//   final       : assign against the final centres keeping d2, per-chunk (within-SS, count, best (d2, row)) per cluster, one workgroup
//                 that reduces them chunks ascending, ranks the clusters by (count descending, number ascending) and writes everything in
//                 that numbering, and a relabel of the rows.
// Everything is float64 on values converted exactly from fp32, every operation rounded on its own (exact_f64.h); no floating-point atomics.
#include "exact_f64.h"

namespace {

using sdt_exact::add_rn;
using sdt_exact::div_rn;
using sdt_exact::kMaxD;
using sdt_exact::mul_rn;
using sdt_exact::sub_rn;

constexpr int kChunk = 1024;  // rows of one chunk: the unit of every ordered sum
constexpr int64_t kMaxRows = (int64_t)1 << 24;
constexpr int kMaxK = 64;
constexpr int kRowThreads = 128, kTile = 128;  // one thread per row of a tile
constexpr int kAssignMaxGrid = 512;
constexpr int kAssignLdsBudget = 60 * 1024;
constexpr int kUpdThreads = 256, kUpdTile = 64;
constexpr int kPickThreads = 256;

inline bool sizes_ok(int64_t N, int D) { return N >= 2 && N <= kMaxRows && D >= 2 && D <= kMaxD; }
inline bool k_ok(int64_t N, int k) { return k >= 1 && k <= kMaxK && (int64_t)k <= N; }
inline int num_chunks(int64_t N) { return (int)cdiv64(N, kChunk); }
inline int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

// rows [row0, row0 + rows) of x -> s_x with pitch ld = D | 1 floats: the global loads run along the table (coalesced), and the lanes of
// a wave later read their own rows at one d on different banks
__device__ __forceinline__ void stage_rows(const float* __restrict__ x, int64_t row0, int rows, int D, int ld, float* s_x, int t, int threads) {
    const float* src = x + row0 * D;
    for (int e = t; e < rows * D; e += threads) s_x[(e / D) * ld + e % D] = src[e];
}

// ---- seeding ---------------------------------------------------------------------------------------------------------------------------
// workspace of the seeding, in 8-byte words: chunk sums | chunk maxima | rows of the maxima | last rows with m > 0 | running sums P
struct SeedWs {
    double* sum;
    double* max;
    long long* arg;
    long long* last;
    double* P;
};
inline int64_t seed_ws_bytes(int64_t N) { return (int64_t)num_chunks(N) * 40; }
inline SeedWs seed_ws(void* ws, int64_t N) {
    const int64_t c = num_chunks(N);
    SeedWs w;
    w.sum = (double*)ws;
    w.max = w.sum + c;
    w.arg = (long long*)(w.max + c);
    w.last = w.arg + c;
    w.P = (double*)(w.last + c);
    return w;
}

// workgroup = chunk.  d2 of every row to row seeds[j]; first != 0: m is written without being read (m starts at +inf, and d2 is finite)
__global__ void __launch_bounds__(kRowThreads) sdt_code_clusters_seed_update_kernel(const float* __restrict__ x, int64_t N, int D,
                                                                                    const long long* __restrict__ seeds, int j, int first,
                                                                                    double* __restrict__ m, SeedWs w) {
    __shared__ float s_x[kTile * (kMaxD + 1)];
    __shared__ double s_seed[kMaxD];
    __shared__ double s_m[kChunk];
    const int t = threadIdx.x, ld = D | 1;
    long long s = seeds[j];
    s = s < 0 ? 0 : (s >= N ? N - 1 : s);  // (a row number from a device buffer: kept inside the table)
    if (t < D) s_seed[t] = (double)x[s * D + t];
    const int64_t row0 = (int64_t)blockIdx.x * kChunk;
    const int rows = (int)(N - row0 < kChunk ? N - row0 : kChunk);
    for (int r0 = 0; r0 < rows; r0 += kTile) {
        __syncthreads();  // the seed row is staged; the previous tile has been read
        const int tr = rows - r0 < kTile ? rows - r0 : kTile;
        stage_rows(x, row0 + r0, tr, D, ld, s_x, t, kRowThreads);
        __syncthreads();
        if (t < tr) {
            double acc = 0.0;
            for (int d = 0; d < D; ++d) {
                const double diff = sub_rn((double)s_x[t * ld + d], s_seed[d]);
                acc = add_rn(acc, mul_rn(diff, diff));
            }
            const int64_t n = row0 + r0 + t;
            if (!first) {
                const double old = m[n];
                acc = old < acc ? old : acc;
            }
            m[n] = acc;
            s_m[r0 + t] = acc;
        }
    }
    __syncthreads();
    if (t == 0) {  // the ordered sum, rows ascending from +0.0
        double sum = 0.0;
        for (int r = 0; r < rows; ++r) sum = add_rn(sum, s_m[r]);
        w.sum[blockIdx.x] = sum;
    } else if (t == 64) {  // (the other wave) exact comparisons: the largest m, of equals the lowest row; the last row with m > 0
        double best = -1.0;
        int arg = 0, last = -1;
        for (int r = 0; r < rows; ++r) {
            const double v = s_m[r];
            if (v > best) {
                best = v;
                arg = r;
            }
            if (v > 0.0) last = r;
        }
        w.max[blockIdx.x] = best;
        w.arg[blockIdx.x] = row0 + arg;
        w.last[blockIdx.x] = last < 0 ? -1 : row0 + last;
    }
}

// the rule for a table whose remaining rows all coincide with a seed: the lowest row that is not among seeds[0, j)
__device__ long long lowest_free_row(const long long* seeds, int j) {
    for (long long cand = 0; cand <= j; ++cand) {  // j seeds cannot cover j + 1 candidates
        bool taken = false;
        for (int i = 0; i < j; ++i) taken = taken || seeds[i] == cand;
        if (!taken) return cand;
    }
    return j;
}

// one workgroup.  mode 0 (k-means++): P = running sum of the chunk sums, T = P[last], r = u T, the first chunk with P > r, then the walk
// inside it from P[chunk - 1]; mode 1 (farthest): the (m, row) maximum.  info: T (mode 1: the maximum), r, chunk, rule (0 the walk
// passed r, 1 the chunk's last positive row, 2 the table's last positive row, 3 no distance left, 4 farthest).
__global__ void __launch_bounds__(kPickThreads) sdt_code_clusters_seed_pick_kernel(const double* __restrict__ m, int64_t N, int chunks, int mode,
                                                                                   double u, long long* __restrict__ seeds, int j, SeedWs w,
                                                                                   double* __restrict__ info) {
    __shared__ double s_buf[kChunk];
    __shared__ long long s_idx[kPickThreads];
    __shared__ double s_val[kPickThreads];
    __shared__ double s_T;
    const int t = threadIdx.x;
    if (mode == 1) {
        double bd = -1.0;
        long long bn = 0x7fffffffffffffffll;
        for (int c = t; c < chunks; c += kPickThreads) {
            const double v = w.max[c];
            const long long n = w.arg[c];
            if (v > bd || (v == bd && n < bn)) {
                bd = v;
                bn = n;
            }
        }
        s_val[t] = bd;
        s_idx[t] = bn;
        __syncthreads();
        if (t == 0) {
            for (int i = 1; i < kPickThreads; ++i)
                if (s_val[i] > bd || (s_val[i] == bd && s_idx[i] < bn)) {
                    bd = s_val[i];
                    bn = s_idx[i];
                }
            const bool none = !(bd > 0.0);
            long long row = none ? lowest_free_row(seeds, j) : bn;
            row = row < 0 ? 0 : (row >= N ? N - 1 : row);
            seeds[j] = row;
            info[0] = bd;
            info[1] = 0.0;
            info[2] = -1.0;
            info[3] = none ? 3.0 : 4.0;
        }
        return;
    }
    double run = 0.0;  // (thread 0) the running sum over all chunks
    for (int c0 = 0; c0 < chunks; c0 += kChunk) {
        const int cnt = chunks - c0 < kChunk ? chunks - c0 : kChunk;
        __syncthreads();
        for (int i = t; i < cnt; i += kPickThreads) s_buf[i] = w.sum[c0 + i];
        __syncthreads();
        if (t == 0)
            for (int i = 0; i < cnt; ++i) {
                run = add_rn(run, s_buf[i]);
                s_buf[i] = run;
            }
        __syncthreads();
        for (int i = t; i < cnt; i += kPickThreads) w.P[c0 + i] = s_buf[i];
    }
    if (t == 0) s_T = run;
    __syncthreads();  // (also: the P written above is visible to the workgroup)
    const double T = s_T, r = mul_rn(u, T);
    if (!(T > 0.0)) {
        if (t == 0) {
            seeds[j] = lowest_free_row(seeds, j);
            info[0] = T;
            info[1] = r;
            info[2] = -1.0;
            info[3] = 3.0;
        }
        return;
    }
    long long first = chunks;  // P does not decrease: a thread's first hit is its lowest
    for (int c = t; c < chunks; c += kPickThreads)
        if (w.P[c] > r) {
            first = c;
            break;
        }
    s_idx[t] = first;
    __syncthreads();
    for (int o = kPickThreads / 2; o > 0; o >>= 1) {
        if (t < o && s_idx[t + o] < s_idx[t]) s_idx[t] = s_idx[t + o];
        __syncthreads();
    }
    const int chosen = (int)s_idx[0];
    if (chosen >= chunks) {  // r == T (only u == 1 gets there): the last row of the table that still has a distance
        if (t == 0) {
            long long row = 0;
            for (int c = chunks - 1; c >= 0; --c)
                if (w.last[c] >= 0) {
                    row = w.last[c];
                    break;
                }
            seeds[j] = row < 0 ? 0 : (row >= N ? N - 1 : row);
            info[0] = T;
            info[1] = r;
            info[2] = -1.0;
            info[3] = 2.0;
        }
        return;
    }
    const int64_t row0 = (int64_t)chosen * kChunk;
    const int rows = (int)(N - row0 < kChunk ? N - row0 : kChunk);
    __syncthreads();
    for (int i = t; i < rows; i += kPickThreads) s_buf[i] = m[row0 + i];
    __syncthreads();
    if (t == 0) {
        double walk = chosen > 0 ? w.P[chosen - 1] : 0.0;
        int pick = -1, last = -1;
        for (int i = 0; i < rows; ++i) {
            const double v = s_buf[i];
            walk = add_rn(walk, v);
            if (v > 0.0) last = i;
            if (walk > r) {
                pick = i;
                break;
            }
        }
        const int at = pick >= 0 ? pick : (last >= 0 ? last : 0);
        seeds[j] = row0 + at;
        info[0] = T;
        info[1] = r;
        info[2] = (double)chosen;
        info[3] = pick >= 0 ? 0.0 : 1.0;
    }
}

// ---- assignment ------------------------------------------------------------------------------------------------------------------------
// rows of a tile: 128, or 64 where 128 rows and the k centres together would pass 60 KiB of LDS (k D > 3520 at D = 64)
inline int assign_tile_rows(int D, int k) {
    return align16((int64_t)k * D * 8) + (int64_t)kTile * (D | 1) * 4 <= kAssignLdsBudget ? kTile : kTile / 2;
}
inline int assign_lds_bytes(int D, int k) { return (int)(align16((int64_t)k * D * 8) + (int64_t)assign_tile_rows(D, k) * (D | 1) * 4); }

__global__ void __launch_bounds__(kRowThreads) sdt_code_clusters_zero_kernel(unsigned long long* word) {
    if (threadIdx.x == 0 && blockIdx.x == 0) word[0] = 0ull;
}

// workgroup b takes the tiles b, b + G, ...  labels: read (unless first) and written by the thread that owns the row.  dist: d2 to the
// chosen centre, or null.  changed: null, or a word zeroed earlier in the stream.  All LDS is dynamic: centres (k D float64) | tile.
__global__ void __launch_bounds__(kRowThreads) sdt_code_clusters_assign_kernel(const float* __restrict__ x, int64_t N, int D,
                                                                               const double* __restrict__ centers, int k, int tile_rows,
                                                                               int32_t* __restrict__ labels, int first,
                                                                               unsigned long long* __restrict__ changed,
                                                                               double* __restrict__ dist) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* s_c = (double*)smem;
    float* s_x = (float*)(smem + (((size_t)k * D * 8 + 15) & ~(size_t)15));
    const int t = threadIdx.x, ld = D | 1;
    for (int e = t; e < k * D; e += kRowThreads) s_c[e] = centers[e];
    const int64_t tiles = (N + tile_rows - 1) / tile_rows;
    const double inf = __builtin_huge_val();
    unsigned int diff_count = 0u;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        __syncthreads();  // the centres are staged; the previous tile has been read
        const int64_t row0 = tile * tile_rows;
        const int tr = (int)(N - row0 < tile_rows ? N - row0 : tile_rows);
        stage_rows(x, row0, tr, D, ld, s_x, t, kRowThreads);
        __syncthreads();
        if (t < tr) {
            const float* xr = s_x + t * ld;
            double bd = inf;
            int bc = 0;
            for (int c0 = 0; c0 < k; c0 += 4) {  // four centres at a time: four independent chains of rounded operations
                const double* p0 = s_c + c0 * D;
                const double* p1 = s_c + (c0 + 1 < k ? c0 + 1 : c0) * D;
                const double* p2 = s_c + (c0 + 2 < k ? c0 + 2 : c0) * D;
                const double* p3 = s_c + (c0 + 3 < k ? c0 + 3 : c0) * D;
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
                for (int d = 0; d < D; ++d) {
                    const double xv = (double)xr[d];
                    const double e0 = sub_rn(xv, p0[d]), e1 = sub_rn(xv, p1[d]), e2 = sub_rn(xv, p2[d]), e3 = sub_rn(xv, p3[d]);
                    a0 = add_rn(a0, mul_rn(e0, e0));
                    a1 = add_rn(a1, mul_rn(e1, e1));
                    a2 = add_rn(a2, mul_rn(e2, e2));
                    a3 = add_rn(a3, mul_rn(e3, e3));
                }
                // ascending c with a strict comparison: of equal distances the lower cluster (a repeated centre never beats itself)
                if (a0 < bd) {
                    bd = a0;
                    bc = c0;
                }
                if (c0 + 1 < k && a1 < bd) {
                    bd = a1;
                    bc = c0 + 1;
                }
                if (c0 + 2 < k && a2 < bd) {
                    bd = a2;
                    bc = c0 + 2;
                }
                if (c0 + 3 < k && a3 < bd) {
                    bd = a3;
                    bc = c0 + 3;
                }
            }
            const int64_t n = row0 + t;
            if (first || labels[n] != bc) ++diff_count;
            labels[n] = bc;
            if (dist != nullptr) dist[n] = bd;
        }
    }
    if (changed != nullptr) {  // an integer count: the order of the additions does not matter
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) diff_count += __shfl_xor(diff_count, o, 64);
        if (t % 64 == 0 && diff_count != 0u) atomicAdd(changed, (unsigned long long)diff_count);
    }
}

// ---- centre update ---------------------------------------------------------------------------------------------------------------------
inline int64_t update_ws_bytes(int64_t N, int D, int k) {
    const int64_t c = num_chunks(N);
    return c * k * D * 8 + align16(c * k * 4);
}
inline int update_lds_bytes(int D, int k) { return (int)(align16((int64_t)k * D * 8) + align16((int64_t)kUpdTile * (D | 1) * 4) + kUpdTile * 4 + kMaxK * 4); }

// workgroup = chunk; thread t owns the (cluster, d) pairs t, t + 256, ... and walks the rows of the chunk in ascending order, 64 staged
// rows at a time, its sums resting in LDS between tiles.  A row of another cluster adds +0.0 instead of being skipped: the sums start
// at +0.0 and the rows are finite, so no partial sum is ever -0.0 and adding +0.0 changes no bit of it; the lanes do not diverge.
// All LDS is dynamic: sums (k D float64) | tile (64 rows, pitch D | 1 floats) | labels of the tile | counts (64).
__global__ void __launch_bounds__(kUpdThreads) sdt_code_clusters_update_kernel(const float* __restrict__ x, int64_t N, int D,
                                                                               const int32_t* __restrict__ labels, int k,
                                                                               double* __restrict__ part_total, int32_t* __restrict__ part_count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ld = D | 1, kd = k * D, t = threadIdx.x;
    double* s_acc = (double*)smem;
    float* s_x = (float*)(smem + (((size_t)kd * 8 + 15) & ~(size_t)15));
    int* s_lab = (int*)((char*)s_x + (((size_t)kUpdTile * ld * 4 + 15) & ~(size_t)15));
    int* s_cnt = s_lab + kUpdTile;
    for (int p = t; p < kd; p += kUpdThreads) s_acc[p] = 0.0;
    if (t < kMaxK) s_cnt[t] = 0;
    const int64_t row0 = (int64_t)blockIdx.x * kChunk;
    const int rows = (int)(N - row0 < kChunk ? N - row0 : kChunk);
    for (int r0 = 0; r0 < rows; r0 += kUpdTile) {
        __syncthreads();
        const int tr = rows - r0 < kUpdTile ? rows - r0 : kUpdTile;
        stage_rows(x, row0 + r0, tr, D, ld, s_x, t, kUpdThreads);
        if (t < tr) {
            const int lab = labels[row0 + r0 + t];
            s_lab[t] = lab;
            if ((unsigned)lab < (unsigned)k) atomicAdd(&s_cnt[lab], 1);  // (a label outside [0, k) belongs to no cluster)
        }
        __syncthreads();
        for (int p = t; p < kd; p += kUpdThreads) {
            const int c = p / D, d = p % D;
            double acc = s_acc[p];
            for (int r = 0; r < tr; ++r) acc = add_rn(acc, s_lab[r] == c ? (double)s_x[r * ld + d] : 0.0);
            s_acc[p] = acc;
        }
    }
    __syncthreads();
    for (int p = t; p < kd; p += kUpdThreads) part_total[(int64_t)blockIdx.x * kd + p] = s_acc[p];
    if (t < k) part_count[(int64_t)blockIdx.x * k + t] = s_cnt[t];
}

// thread p = (cluster, d): the chunk partials in ascending chunk order, the integer count, the division; an empty cluster keeps its centre
__global__ void __launch_bounds__(kUpdThreads) sdt_code_clusters_update_reduce_kernel(int chunks, int D, int k, const double* __restrict__ part_total,
                                                                                      const int32_t* __restrict__ part_count,
                                                                                      double* __restrict__ centers, int32_t* __restrict__ counts) {
    const int p = blockIdx.x * kUpdThreads + threadIdx.x, kd = k * D;
    if (p >= kd) return;
    const int c = p / D;
    double total = 0.0;
    long long count = 0;
    for (int ch = 0; ch < chunks; ++ch) {
        total = add_rn(total, part_total[(int64_t)ch * kd + p]);
        count += part_count[(int64_t)ch * k + c];
    }
    if (count > 0) centers[p] = div_rn(total, (double)count);
    if (p % D == 0) counts[c] = (int32_t)count;
}

// ---- final pass ------------------------------------------------------------------------------------------------------------------------
// workspace: d2 of every row (N) | per (chunk, cluster): within-SS | best d2 | best row | count (int32) || rank of every cluster (int32)
struct FinalWs {
    double* dist;
    double* ss;
    double* bd;
    long long* bn;
    int32_t* cnt;
    int32_t* rank;
};
inline int64_t final_ws_bytes(int64_t N, int k) {
    const int64_t ck = (int64_t)num_chunks(N) * k;
    return N * 8 + ck * 24 + align16(ck * 4) + kMaxK * 4;
}
inline FinalWs final_ws(void* ws, int64_t N, int k) {
    const int64_t ck = (int64_t)num_chunks(N) * k;
    FinalWs w;
    w.dist = (double*)ws;
    w.ss = w.dist + N;
    w.bd = w.ss + ck;
    w.bn = (long long*)(w.bd + ck);
    w.cnt = (int32_t*)(w.bn + ck);
    w.rank = (int32_t*)((char*)w.cnt + align16(ck * 4));
    return w;
}

// workgroup = chunk; thread c < k walks the chunk's rows ascending: the ordered sum of its members' d2 (+0.0 for the others, as in the
// update), their number, and the member with the smallest (d2, row): a strict comparison keeps the lowest row of equal distances
__global__ void __launch_bounds__(kUpdThreads) sdt_code_clusters_final_chunk_kernel(int64_t N, int k, const int32_t* __restrict__ labels, FinalWs w) {
    __shared__ double s_d[kChunk];
    __shared__ int s_l[kChunk];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kChunk;
    const int rows = (int)(N - row0 < kChunk ? N - row0 : kChunk);
    for (int r = t; r < rows; r += kUpdThreads) {
        s_d[r] = w.dist[row0 + r];
        s_l[r] = labels[row0 + r];
    }
    __syncthreads();
    if (t >= k) return;
    double ss = 0.0, bd = __builtin_huge_val();
    long long bn = -1;
    int cnt = 0;
    for (int r = 0; r < rows; ++r) {
        const bool member = s_l[r] == t;
        const double v = s_d[r];
        ss = add_rn(ss, member ? v : 0.0);
        cnt += member ? 1 : 0;
        if (member && v < bd) {
            bd = v;
            bn = row0 + r;
        }
    }
    const int64_t slot = (int64_t)blockIdx.x * k + t;
    w.ss[slot] = ss;
    w.bd[slot] = bd;
    w.bn[slot] = bn;
    w.cnt[slot] = cnt;
}

// one workgroup, thread c < k: the chunk partials in ascending chunk order; the rank of cluster c = the number of clusters with more
// members, or as many and a lower number; every output in the ranked numbering; inertia = the ascending sum of the ranked within-SS
__global__ void __launch_bounds__(kMaxK) sdt_code_clusters_final_reduce_kernel(int chunks, int D, int k, FinalWs w, const double* __restrict__ centers,
                                                                               double* __restrict__ centers_out, int32_t* __restrict__ counts,
                                                                               double* __restrict__ within_ss, double* __restrict__ inertia,
                                                                               long long* __restrict__ code_index, double* __restrict__ code_dist2,
                                                                               int32_t* __restrict__ order) {
    __shared__ long long s_cnt[kMaxK];
    __shared__ double s_ss[kMaxK];
    const int c = threadIdx.x;
    double ss = 0.0, bd = __builtin_huge_val();
    long long bn = -1, cnt = 0;
    if (c < k) {
        for (int ch = 0; ch < chunks; ++ch) {
            const int64_t slot = (int64_t)ch * k + c;
            ss = add_rn(ss, w.ss[slot]);
            cnt += w.cnt[slot];
            if (w.bn[slot] >= 0 && w.bd[slot] < bd) {
                bd = w.bd[slot];
                bn = w.bn[slot];
            }
        }
        s_cnt[c] = cnt;
    }
    __syncthreads();
    int rank = 0;
    if (c < k) {
        for (int o = 0; o < k; ++o) rank += (s_cnt[o] > cnt || (s_cnt[o] == cnt && o < c)) ? 1 : 0;
        s_ss[rank] = ss;
        counts[rank] = (int32_t)cnt;
        within_ss[rank] = ss;
        code_index[rank] = bn;
        code_dist2[rank] = bd;
        order[rank] = c;
        w.rank[c] = rank;
        for (int d = 0; d < D; ++d) centers_out[rank * D + d] = centers[c * D + d];
    }
    __syncthreads();
    if (c == 0) inertia[0] = sdt_exact::ordered_sum(s_ss, k);
}

__global__ void __launch_bounds__(kUpdThreads) sdt_code_clusters_relabel_kernel(int64_t N, int k, const int32_t* __restrict__ rank,
                                                                                int32_t* __restrict__ labels) {
    const int64_t n = (int64_t)blockIdx.x * kUpdThreads + threadIdx.x;
    if (n >= N) return;
    const int lab = labels[n];
    if ((unsigned)lab < (unsigned)k) labels[n] = rank[lab];
}

void launch_assign(const float* x, int64_t N, int D, const double* centers, int k, int32_t* labels, int first, unsigned long long* changed,
                   double* dist, hipStream_t st) {
    const int tile_rows = assign_tile_rows(D, k);
    const int G = (int)std::min<int64_t>(kAssignMaxGrid, cdiv64(N, tile_rows));
    hipLaunchKernelGGL(sdt_code_clusters_assign_kernel, dim3(G), dim3(kRowThreads), assign_lds_bytes(D, k), st, x, N, D, centers, k, tile_rows,
                       labels, first, changed, dist);
}

}  // namespace

#define SDT_CLUSTER_SIZES(n_rows, dim) SDT_CHECK_SUPPORTED(sizes_ok(n_rows, dim), "n_rows must lie in [2, 2^24] and dim in [2, 64]")
#define SDT_CLUSTER_K(n_rows, k) SDT_CHECK_SUPPORTED(k_ok(n_rows, k), "k must lie in [1, 64] and not exceed n_rows")

extern "C" int64_t sdt_code_clusters_seed_workspace_bytes(int64_t n_rows, int dim) {
    if (!sizes_ok(n_rows, dim)) return 0;
    return seed_ws_bytes(n_rows);
}

extern "C" int sdt_code_clusters_seed_update(const float* x, int64_t n_rows, int dim, const int64_t* seeds, int j, int first, double* m,
                                             void* workspace, int64_t workspace_bytes, void* stream) {
    SDT_CHECK_ARG(x != nullptr && seeds != nullptr && m != nullptr && workspace != nullptr, "null pointer");
    SDT_CLUSTER_SIZES(n_rows, dim);
    SDT_CHECK_SUPPORTED(j >= 0 && j < kMaxK, "the seed number must lie in [0, 64)");
    SDT_CHECK_ARG(workspace_bytes >= seed_ws_bytes(n_rows), "workspace too small");
    hipLaunchKernelGGL(sdt_code_clusters_seed_update_kernel, dim3(num_chunks(n_rows)), dim3(kRowThreads), 0, (hipStream_t)stream, x, n_rows, dim,
                       (const long long*)seeds, j, first, m, seed_ws(workspace, n_rows));
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_code_clusters_seed_pick(const double* m, int64_t n_rows, int mode, double u, int64_t* seeds, int j, double* info,
                                           void* workspace, int64_t workspace_bytes, void* stream) {
    SDT_CHECK_ARG(m != nullptr && seeds != nullptr && info != nullptr && workspace != nullptr, "null pointer");
    SDT_CHECK_SUPPORTED(n_rows >= 2 && n_rows <= kMaxRows, "n_rows must lie in [2, 2^24]");
    SDT_CHECK_SUPPORTED(j >= 1 && j < kMaxK && (int64_t)j < n_rows, "the seed number must lie in [1, 64) and below n_rows");
    SDT_CHECK_ARG(mode == 0 || mode == 1, "mode must be 0 (k-means++) or 1 (farthest)");
    SDT_CHECK_ARG(u >= 0.0 && u <= 1.0, "u must lie in [0, 1]");
    SDT_CHECK_ARG(workspace_bytes >= seed_ws_bytes(n_rows), "workspace too small");
    hipLaunchKernelGGL(sdt_code_clusters_seed_pick_kernel, dim3(1), dim3(kPickThreads), 0, (hipStream_t)stream, m, n_rows, num_chunks(n_rows), mode,
                       u, (long long*)seeds, j, seed_ws(workspace, n_rows), info);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_code_clusters_assign(const float* x, int64_t n_rows, int dim, const double* centers, int k, int32_t* labels, int first,
                                        int64_t* changed, void* stream) {
    SDT_CHECK_ARG(x != nullptr && centers != nullptr && labels != nullptr && changed != nullptr, "null pointer");
    SDT_CLUSTER_SIZES(n_rows, dim);
    SDT_CLUSTER_K(n_rows, k);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sdt_code_clusters_zero_kernel, dim3(1), dim3(kRowThreads), 0, st, (unsigned long long*)changed);
    launch_assign(x, n_rows, dim, centers, k, labels, first, (unsigned long long*)changed, nullptr, st);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int64_t sdt_code_clusters_update_workspace_bytes(int64_t n_rows, int dim, int k) {
    if (!sizes_ok(n_rows, dim) || !k_ok(n_rows, k)) return 0;
    return update_ws_bytes(n_rows, dim, k);
}

extern "C" int sdt_code_clusters_update(const float* x, int64_t n_rows, int dim, const int32_t* labels, int k, double* centers, int32_t* counts,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
    SDT_CHECK_ARG(x != nullptr && labels != nullptr && centers != nullptr && counts != nullptr && workspace != nullptr, "null pointer");
    SDT_CLUSTER_SIZES(n_rows, dim);
    SDT_CLUSTER_K(n_rows, k);
    SDT_CHECK_ARG(workspace_bytes >= update_ws_bytes(n_rows, dim, k), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int chunks = num_chunks(n_rows);
    double* part_total = (double*)workspace;
    int32_t* part_count = (int32_t*)(part_total + (int64_t)chunks * k * dim);
    hipLaunchKernelGGL(sdt_code_clusters_update_kernel, dim3(chunks), dim3(kUpdThreads), update_lds_bytes(dim, k), st, x, n_rows, dim, labels, k,
                       part_total, part_count);
    hipLaunchKernelGGL(sdt_code_clusters_update_reduce_kernel, dim3(cdiv(k * dim, kUpdThreads)), dim3(kUpdThreads), 0, st, chunks, dim, k, part_total,
                       part_count, centers, counts);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int64_t sdt_code_clusters_final_workspace_bytes(int64_t n_rows, int dim, int k) {
    if (!sizes_ok(n_rows, dim) || !k_ok(n_rows, k)) return 0;
    return final_ws_bytes(n_rows, k);
}

extern "C" int sdt_code_clusters_final(const float* x, int64_t n_rows, int dim, const double* centers, int k, int32_t* labels, double* centers_out,
                                       int32_t* counts, double* within_ss, double* inertia, int64_t* code_index, double* code_dist2,
                                       int32_t* order, void* workspace, int64_t workspace_bytes, void* stream) {
    SDT_CHECK_ARG(x != nullptr && centers != nullptr && labels != nullptr && centers_out != nullptr && counts != nullptr && within_ss != nullptr &&
                      inertia != nullptr && code_index != nullptr && code_dist2 != nullptr && order != nullptr && workspace != nullptr,
                  "null pointer");
    SDT_CLUSTER_SIZES(n_rows, dim);
    SDT_CLUSTER_K(n_rows, k);
    SDT_CHECK_ARG(centers != centers_out, "centers_out must not be centers");
    SDT_CHECK_ARG(workspace_bytes >= final_ws_bytes(n_rows, k), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int chunks = num_chunks(n_rows);
    const FinalWs w = final_ws(workspace, n_rows, k);
    launch_assign(x, n_rows, dim, centers, k, labels, 1, nullptr, w.dist, st);
    hipLaunchKernelGGL(sdt_code_clusters_final_chunk_kernel, dim3(chunks), dim3(kUpdThreads), 0, st, n_rows, k, labels, w);
    hipLaunchKernelGGL(sdt_code_clusters_final_reduce_kernel, dim3(1), dim3(kMaxK), 0, st, chunks, dim, k, w, centers, centers_out, counts, within_ss,
                       inertia, (long long*)code_index, code_dist2, order);
    hipLaunchKernelGGL(sdt_code_clusters_relabel_kernel, dim3((unsigned)cdiv64(n_rows, kUpdThreads)), dim3(kUpdThreads), 0, st, n_rows, k, w.rank,
                       labels);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
