// Principal template axes and nearest template codes (code_axes.py): the (N, D) fp32 clip-code table is decomposed
// along ALL of its principal axes, the populated range of every axis is measured by exact order statistics, and any point of that
// space is mapped to the nearest row of the table.  The output file is what the two demo modes of the reference consume
// (pose2pose.py:50-56 DEMO.CODE_PATH, voice2pose.py:107-117 DEMO.CODE_INDEX / CODE_INDEX_B).  Four stages:
//   eigh      : the eigen kernel of code_pca.hip (the one-wave cyclic Jacobi of jacobi.h), asked for every component.
//   project   : P (N, D) = (x - mean) . comps^T.  A tile of 32 rows is staged in LDS by coalesced fp32 loads and centred there;
//               thread per (row, axis) pair, the pairs of a tile in the order of P, so the float64 stores are contiguous.
//   quantiles : radix select on the order-preserving uint64 image of the float64 bits, 8 passes of 8 bits; 256-bin histograms per
//               (axis, rank) with integer atomics, in LDS first; the surviving prefix and the remaining rank stay on the device.
//   nearest   : tiles of 128 table rows staged in LDS, 8 queries per workgroup, a (d2, n) pair per thread and query, reduced by
//               comparing d2 first and n second; one partial per (query tile, row chunk), then a final kernel over the partials.
// Everything is float64 on values converted exactly from fp32, every operation rounded on its own (exact_f64.h); no floating-point atomics.
#include "jacobi.h"
#include "radix_select.h"

namespace {

using sdt_exact::add_rn;
using sdt_exact::kMaxD;
using sdt_exact::mul_rn;
using sdt_exact::sub_rn;

constexpr int kThreads = 256;
constexpr int64_t kMaxRows = (int64_t)1 << 30;
constexpr int kMaxQueries = 65536, kMaxRanks = 16;

// ---- projection --------------------------------------------------------------------------------------------------------------------------
constexpr int kProjRows = 32, kProjMaxGrid = 2048;
constexpr int kCompLd = kMaxD + 1;  // pitch of comps in LDS: the 32 lanes of a ds_read_b64 group read 32 axes at one d on 64 different banks

// workgroup b takes the 32-row tiles b, b + G, ...  P[n,k] = sum over d ascending of (x[n,d] - mean[d]) * comps[k,d].
__global__ void __launch_bounds__(kThreads) sdt_code_axes_project_kernel(const float* __restrict__ x, int64_t N, int D,
                                                                         const double* __restrict__ mean, const double* __restrict__ comps,
                                                                         double* __restrict__ P) {
    __shared__ double s_c[kProjRows * kMaxD];  // centred rows, pitch D
    __shared__ double s_comp[kMaxD * kCompLd];
    __shared__ double s_mean[kMaxD];
    const int t = threadIdx.x;
    if (t < D) s_mean[t] = mean[t];
    for (int e = t; e < D * D; e += kThreads) s_comp[(e / D) * kCompLd + e % D] = comps[e];
    __syncthreads();
    const int64_t tiles = (N + kProjRows - 1) / kProjRows, total = N * D;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t base = tile * kProjRows * D;
        for (int e = t; e < kProjRows * D; e += kThreads)
            if (base + e < total) s_c[e] = sub_rn((double)x[base + e], s_mean[e % D]);
        __syncthreads();
        for (int e = t; e < kProjRows * D; e += kThreads) {
            if (base + e >= total) break;
            const int r = e / D, k = e % D;
            const double* c = s_c + r * D;
            const double* v = s_comp + k * kCompLd;
            double acc = 0.0;
            for (int d = 0; d < D; ++d) acc = add_rn(acc, mul_rn(c[d], v[d]));
            P[base + e] = acc;
        }
        __syncthreads();
    }
}

// ---- exact order statistics ------------------------------------------------------------------------------------------------------------
constexpr int kHistPairs = 32;       // (axis, rank) histograms of one workgroup in LDS: 32 x 256 x 4 bytes
constexpr int kSelMaxGridX = 512;

using sdt_select::order_key;  // (radix_select.h: the key, its inverse and the digit choice, shared with speech_gate.hip)
using sdt_select::order_value;

inline int sel_cols_per_group(int R) { return std::max(1, kHistPairs / R); }

// state of the select, in the workspace: prefix (D*R uint64) | remaining rank (D*R int64) | histograms (D*R*256 uint32)
__global__ void __launch_bounds__(kThreads) sdt_code_axes_select_init_kernel(const int64_t* __restrict__ ranks, int D, int R,
                                                                             unsigned long long* __restrict__ prefix,
                                                                             long long* __restrict__ remain, uint32_t* __restrict__ hist) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < D * R * 256) hist[i] = 0u;
    if (i < D * R) {
        prefix[i] = 0ull;
        remain[i] = ranks[i % R];
    }
}

// blockIdx.y = group of cg columns, blockIdx.x = row lane: thread (rr, c) = (t / cg, t % cg) walks rows rr + 256 / cg * (blockIdx.x + i * gridDim.x)
// of column k0 + c.  An element whose bits above the current byte equal the prefix of (column, rank) counts into that pair's histogram.
__global__ void __launch_bounds__(kThreads) sdt_code_axes_select_hist_kernel(const double* __restrict__ P, int64_t N, int D, int R, int cg,
                                                                             int pass, const unsigned long long* __restrict__ prefix,
                                                                             uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_h[kHistPairs * 256];
    __shared__ unsigned long long s_prefix[kHistPairs];
    const int t = threadIdx.x, k0 = blockIdx.y * cg, ncol = min(cg, D - k0), pairs = ncol * R;  // cg = 32 / R and R <= 16: pairs <= 32
    for (int e = t; e < pairs * 256; e += kThreads) s_h[e] = 0u;
    if (t < pairs) s_prefix[t] = prefix[(int64_t)k0 * R + t];
    __syncthreads();
    const int shift = 56 - 8 * pass, rows_par = kThreads / cg, rr = t / cg, c = t % cg;
    if (rr < rows_par && c < ncol) {
        for (int64_t n = (int64_t)blockIdx.x * rows_par + rr; n < N; n += (int64_t)gridDim.x * rows_par) {
            const unsigned long long key = order_key(P[n * D + k0 + c]);
            const uint32_t digit = (uint32_t)(key >> shift) & 255u;
            for (int r = 0; r < R; ++r) {
                const bool match = pass == 0 || ((key ^ s_prefix[c * R + r]) >> (shift + 8)) == 0ull;
                if (match) atomicAdd(&s_h[(c * R + r) * 256 + digit], 1u);
            }
        }
    }
    __syncthreads();
    for (int e = t; e < pairs * 256; e += kThreads) {
        const uint32_t v = s_h[e];
        if (v != 0u) atomicAdd(&hist[(int64_t)k0 * R * 256 + e], v);
    }
}

// one workgroup per (column, rank): the byte whose cumulative count passes the remaining rank joins the prefix; the histogram is zeroed
// for the next pass; the last pass writes the value.
__global__ void __launch_bounds__(kThreads) sdt_code_axes_select_step_kernel(int pass, unsigned long long* __restrict__ prefix,
                                                                             long long* __restrict__ remain, uint32_t* __restrict__ hist,
                                                                             double* __restrict__ out) {
    __shared__ uint32_t s_cnt[256];
    const int pair = blockIdx.x, t = threadIdx.x;
    s_cnt[t] = hist[(int64_t)pair * 256 + t];
    hist[(int64_t)pair * 256 + t] = 0u;
    __syncthreads();
    if (t != 0) return;
    long long rem = remain[pair];
    const int digit = sdt_select::pick_digit(s_cnt, &rem);
    const unsigned long long p = prefix[pair] | ((unsigned long long)digit << (56 - 8 * pass));
    prefix[pair] = p;
    remain[pair] = rem;
    if (pass == 7) out[pair] = order_value(p);
}

inline int64_t quantiles_ws_bytes(int D, int R) { return (int64_t)D * R * (8 + 8 + 256 * 4); }

// ---- nearest row ---------------------------------------------------------------------------------------------------------------------------
constexpr int kNearThreads = 128, kNearRows = 128, kNearQ = 8, kNearTargetGrid = 2048;
constexpr unsigned long long kNoBadQuery = ~0ull;

struct NearPlan {
    int qtiles;       // ceil(Q / 8)
    int chunks;       // row chunks
    int64_t tiles_per_chunk;
};

inline NearPlan near_plan(int64_t N, int64_t Q) {
    NearPlan p;
    p.qtiles = (int)cdiv64(Q, kNearQ);
    const int64_t tiles = cdiv64(N, kNearRows);
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(tiles, kNearTargetGrid / p.qtiles));
    p.tiles_per_chunk = cdiv64(tiles, want);
    p.chunks = (int)cdiv64(tiles, p.tiles_per_chunk);
    return p;
}

// (d2, n) is better than (bd, bn): smaller distance, then the smaller row.  Exact and associative: the result does not depend on the grid.
__device__ __forceinline__ bool near_better(double d2, long long n, double bd, long long bn) { return d2 < bd || (d2 == bd && n < bn); }

// blockIdx.x = query tile, blockIdx.y = row chunk.  Thread t owns row t of every 128-row tile of the chunk (rows ascending: a strict
// comparison keeps the first of equal distances).  part_d / part_n [(qtile*8 + j) * chunks + chunk].
__global__ void __launch_bounds__(kNearThreads) sdt_code_axes_nearest_kernel(const float* __restrict__ x, int64_t N, int D,
                                                                             const double* __restrict__ queries, int64_t Q,
                                                                             int64_t tiles_per_chunk, double* __restrict__ part_d,
                                                                             long long* __restrict__ part_n,
                                                                             unsigned long long* __restrict__ bad) {
    __shared__ float s_x[kNearRows * (kMaxD + 1)];  // pitch D | 1 floats: the lanes of a wave read their rows at one d on different banks
    __shared__ double s_q[kNearQ * kMaxD];
    __shared__ double s_rd[kNearThreads / 64][kNearQ];
    __shared__ long long s_rn[kNearThreads / 64][kNearQ];
    const int t = threadIdx.x, ld = D | 1;
    if (blockIdx.x == 0 && blockIdx.y == 0 && t == 0) bad[0] = kNoBadQuery;  // (the final kernel, later in the stream, lowers it)
    const int64_t q0 = (int64_t)blockIdx.x * kNearQ;
    for (int e = t; e < kNearQ * D; e += kNearThreads) {
        const int64_t q = q0 + e / D;
        s_q[e] = q < Q ? queries[q * D + e % D] : 0.0;
    }
    const double inf = __builtin_huge_val();
    double bd[kNearQ];
    long long bn[kNearQ];
#pragma unroll
    for (int j = 0; j < kNearQ; ++j) {
        bd[j] = inf;
        bn[j] = 0x7fffffffffffffffll;
    }
    const int64_t tiles = (N + kNearRows - 1) / kNearRows, total = N * D;
    const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_chunk, tile1 = tile0 + tiles_per_chunk < tiles ? tile0 + tiles_per_chunk : tiles;
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        __syncthreads();  // the queries are staged; the previous tile has been read
        const int64_t base = tile * kNearRows * D;
        for (int e = t; e < kNearRows * D; e += kNearThreads)
            if (base + e < total) s_x[(e / D) * ld + e % D] = x[base + e];
        __syncthreads();
        const int64_t n = tile * kNearRows + t;
        if (n < N) {
            double acc[kNearQ];
#pragma unroll
            for (int j = 0; j < kNearQ; ++j) acc[j] = 0.0;
            for (int d = 0; d < D; ++d) {
                const double xv = (double)s_x[t * ld + d];
#pragma unroll
                for (int j = 0; j < kNearQ; ++j) {
                    const double diff = sub_rn(s_q[j * D + d], xv);  // the same address in every lane: a broadcast read
                    acc[j] = add_rn(acc[j], mul_rn(diff, diff));
                }
            }
#pragma unroll
            for (int j = 0; j < kNearQ; ++j)
                if (near_better(acc[j], n, bd[j], bn[j])) {
                    bd[j] = acc[j];
                    bn[j] = n;
                }
        }
    }
    // the workgroup's best pair of every query: within the wave by shuffles, then the two waves through LDS
#pragma unroll
    for (int j = 0; j < kNearQ; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(bd[j], o, 64);
            const long long on = __shfl_xor(bn[j], o, 64);
            if (near_better(od, on, bd[j], bn[j])) {
                bd[j] = od;
                bn[j] = on;
            }
        }
        if (t % 64 == 0) {
            s_rd[t / 64][j] = bd[j];
            s_rn[t / 64][j] = bn[j];
        }
    }
    __syncthreads();
    if (t < kNearQ) {
        double d = s_rd[0][t];
        long long n = s_rn[0][t];
        for (int w = 1; w < kNearThreads / 64; ++w)
            if (near_better(s_rd[w][t], s_rn[w][t], d, n)) {
                d = s_rd[w][t];
                n = s_rn[w][t];
            }
        const int64_t slot = (q0 + t) * gridDim.y + blockIdx.y;  // (the partial arrays hold qtiles * 8 queries)
        part_d[slot] = d;
        part_n[slot] = n;
    }
}

// thread q: the best of the partials of query q; a query with a non-finite entry gets index -1 and lowers bad[0] to its number
__global__ void __launch_bounds__(kThreads) sdt_code_axes_nearest_final_kernel(const double* __restrict__ queries, int64_t Q, int D, int chunks,
                                                                               const double* __restrict__ part_d,
                                                                               const long long* __restrict__ part_n,
                                                                               long long* __restrict__ index, double* __restrict__ dist2,
                                                                               unsigned long long* __restrict__ bad) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= Q) return;
    bool finite = true;
    for (int d = 0; d < D; ++d) finite = finite && isfinite(queries[q * D + d]);
    if (!finite) {
        index[q] = -1;
        dist2[q] = __builtin_nan("");
        atomicMin(bad, (unsigned long long)q);
        return;
    }
    double bd = part_d[q * chunks];
    long long bn = part_n[q * chunks];
    for (int c = 1; c < chunks; ++c)
        if (near_better(part_d[q * chunks + c], part_n[q * chunks + c], bd, bn)) {
            bd = part_d[q * chunks + c];
            bn = part_n[q * chunks + c];
        }
    index[q] = bn;
    dist2[q] = bd;
}

inline int64_t nearest_ws_bytes(int64_t N, int64_t Q) {
    const NearPlan p = near_plan(N, Q);
    return (int64_t)p.qtiles * kNearQ * p.chunks * 16;
}

inline bool sizes_ok(int64_t N, int D) { return N >= 2 && N <= kMaxRows && D >= 2 && D <= kMaxD; }

}  // namespace

extern "C" int sdt_code_axes_eigh(const double* cov, int dim, int max_sweeps, double rel_tol, double* evals, double* comps, double* info,
                                  int32_t* err, void* stream) {
    SDT_CHECK_ARG(cov != nullptr && evals != nullptr && comps != nullptr && info != nullptr && err != nullptr, "null pointer");
    SDT_CHECK_SUPPORTED(dim >= 2 && dim <= kMaxD, "dim must lie in [2, 64]");
    SDT_CHECK_ARG(max_sweeps >= 0 && max_sweeps <= 1000, "max_sweeps must lie in [0, 1000]");
    SDT_CHECK_ARG(rel_tol >= 0.0, "rel_tol must not be negative");
    sdt_jacobi::launch_eigh(cov, dim, max_sweeps, rel_tol, dim, evals, comps, info, err, stream);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_code_axes_project(const float* x, int64_t n_rows, int dim, const double* mean, const double* comps, double* P,
                                     void* stream) {
    SDT_CHECK_ARG(x != nullptr && mean != nullptr && comps != nullptr && P != nullptr, "null pointer");
    SDT_CHECK_SUPPORTED(sizes_ok(n_rows, dim), "n_rows must lie in [2, 2^30] and dim in [2, 64]");
    const int G = (int)std::min<int64_t>(kProjMaxGrid, cdiv64(n_rows, kProjRows));
    hipLaunchKernelGGL(sdt_code_axes_project_kernel, dim3(G), dim3(kThreads), 0, (hipStream_t)stream, x, n_rows, dim, mean, comps, P);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int64_t sdt_code_axes_quantiles_workspace_bytes(int64_t n_rows, int dim, int n_ranks) {
    if (!sizes_ok(n_rows, dim) || n_ranks < 1 || n_ranks > kMaxRanks) return 0;
    return quantiles_ws_bytes(dim, n_ranks);
}

extern "C" int sdt_code_axes_quantiles(const double* P, int64_t n_rows, int dim, const int64_t* ranks, int n_ranks, double* out,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
    SDT_CHECK_ARG(P != nullptr && ranks != nullptr && out != nullptr && workspace != nullptr, "null pointer");
    SDT_CHECK_SUPPORTED(sizes_ok(n_rows, dim), "n_rows must lie in [2, 2^30] and dim in [2, 64]");
    SDT_CHECK_SUPPORTED(n_ranks >= 1 && n_ranks <= kMaxRanks, "n_ranks must lie in [1, 16]");
    SDT_CHECK_ARG(workspace_bytes >= quantiles_ws_bytes(dim, n_ranks), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int pairs = dim * n_ranks;
    unsigned long long* prefix = (unsigned long long*)workspace;
    long long* remain = (long long*)(prefix + pairs);
    uint32_t* hist = (uint32_t*)(remain + pairs);
    const int cg = sel_cols_per_group(n_ranks), rows_par = kThreads / cg;
    const dim3 grid((unsigned)std::min<int64_t>(kSelMaxGridX, cdiv64(n_rows, (int64_t)rows_par * 8)), (unsigned)cdiv(dim, cg));
    hipLaunchKernelGGL(sdt_code_axes_select_init_kernel, dim3(cdiv(pairs * 256, kThreads)), dim3(kThreads), 0, st, ranks, dim, n_ranks, prefix,
                       remain, hist);
    for (int pass = 0; pass < 8; ++pass) {
        hipLaunchKernelGGL(sdt_code_axes_select_hist_kernel, grid, dim3(kThreads), 0, st, P, n_rows, dim, n_ranks, cg, pass, prefix, hist);
        hipLaunchKernelGGL(sdt_code_axes_select_step_kernel, dim3(pairs), dim3(kThreads), 0, st, pass, prefix, remain, hist, out);
    }
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int64_t sdt_code_axes_nearest_workspace_bytes(int64_t n_rows, int dim, int64_t n_queries) {
    if (!sizes_ok(n_rows, dim) || n_queries < 1 || n_queries > kMaxQueries) return 0;
    return nearest_ws_bytes(n_rows, n_queries);
}

extern "C" int sdt_code_axes_nearest(const float* x, int64_t n_rows, int dim, const double* queries, int64_t n_queries, int64_t* index,
                                     double* dist2, int64_t* first_bad_query, void* workspace, int64_t workspace_bytes, void* stream) {
    SDT_CHECK_ARG(x != nullptr && queries != nullptr && index != nullptr && dist2 != nullptr && first_bad_query != nullptr &&
                      workspace != nullptr,
                  "null pointer");
    SDT_CHECK_SUPPORTED(sizes_ok(n_rows, dim), "n_rows must lie in [2, 2^30] and dim in [2, 64]");
    SDT_CHECK_SUPPORTED(n_queries >= 1 && n_queries <= kMaxQueries, "n_queries must lie in [1, 65536]");
    SDT_CHECK_ARG(workspace_bytes >= nearest_ws_bytes(n_rows, n_queries), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const NearPlan p = near_plan(n_rows, n_queries);
    double* part_d = (double*)workspace;
    long long* part_n = (long long*)(part_d + (int64_t)p.qtiles * kNearQ * p.chunks);
    hipLaunchKernelGGL(sdt_code_axes_nearest_kernel, dim3(p.qtiles, p.chunks), dim3(kNearThreads), 0, st, x, n_rows, dim, queries, n_queries,
                       p.tiles_per_chunk, part_d, part_n, (unsigned long long*)first_bad_query);
    hipLaunchKernelGGL(sdt_code_axes_nearest_final_kernel, dim3((unsigned)cdiv64(n_queries, kThreads)), dim3(kThreads), 0, st, queries,
                       n_queries, dim, p.chunks, part_d, part_n, (long long*)index, dist2, (unsigned long long*)first_bad_query);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
