// Per-tensor histograms and moments of a flat fp32 buffer in one segmented pass (tensor_hist.py holds the numpy
// contract model).  The buffer is FlatAdam's: every tensor is one segment (offset, numel), offsets are multiples of 4 elements and the
// padding between segments is never read into a result.
//
// Every element is taken as v = (float)(x * scale) (one fp32 multiply) and widened to float64.  Per segment:
//   counts[1548]  bucket i is [E[i], E[i + 1]) of the 1549 float64 edges the caller passes (TensorBoard's default table, built on the
//                 host); a finite v beyond the outermost edges goes to the outermost bucket of its sign.  The bucket is found by float64
//                 compares against the table, starting from a guess taken from log2 of the fp32 magnitude; the guess only saves compares.
//   tallies[3]    finite, NaN and +-inf elements.
//   stats[4]      min, max, sum and sum of squares (float64) over the finite elements.
// Counts and tallies are integer sums (LDS and global integer atomics): exact whatever the arrival order.  The float64 sums have ONE
// order (the CONTRACT tensor_hist.model_histograms states in numpy):
//   chunk    a segment is cut into chunks of HIST_CHUNK elements, one workgroup of 256 threads per chunk;
//   thread   t walks the float4s t, t + 256, t + 512, ... of its chunk, element 0 first, and adds every finite v (v * v for the squares) to
//            accumulators that start at +0; elements past the end of the segment, NaN and +-inf add nothing;
//   wave     six butterfly steps v += v[lane ^ o], o = 32, 16, 8, 4, 2, 1;
//   block    (w0 + w1) + (w2 + w3) over its four waves -> one partial per chunk;
//   final    second launch, one workgroup per segment: thread t adds the partials t, t + 256, ... of the segment in chunk order, then the
//            same wave and block steps.
// This is the tree of sdt_grad_sumsq_f64 (optim_guard.hip).  min and max do not depend on the order.
#include "common.h"

#define HIST_THREADS 256
#define HIST_CHUNK 16384  // elements per workgroup: 16 float4s per thread
#define HIST_BUCKETS 1548
#define HIST_EDGES (HIST_BUCKETS + 1)
#define HIST_ZERO_EDGE 774       // E[774] == 0.0
#define HIST_MAX_SEGMENTS 65536  // tensors per call
#define HIST_MAX_CHUNKS (1 << 24)

// last index i with E[i] <= v, clipped to [0, 1547]; E ascending.  Any guess gives the same answer, a good one gives it in two reads.
__device__ __forceinline__ int hist_bucket(double v, float mag, const double* __restrict__ E) {
    int g;
    if (mag < 1e-12f) {
        g = v >= 0.0 ? HIST_ZERO_EDGE : HIST_ZERO_EDGE - 1;
    } else {
        // the positive edges are 1e-12 * 1.1^k: k ~ (log2 |v| - log2 1e-12) / log2 1.1
        int k = (int)(__log2f(mag) * (1.0f / 0.13750352f) + 289.90537f);
        k = k < 0 ? 0 : k > 773 ? 773 : k;
        g = v >= 0.0 ? HIST_ZERO_EDGE + 1 + k : HIST_ZERO_EDGE - 2 - k;
        g = g < 0 ? 0 : g > HIST_BUCKETS - 1 ? HIST_BUCKETS - 1 : g;  // (k = 773 is the bucket beyond the last edge: the clipped one)
    }
    while (g < HIST_BUCKETS - 1 && v >= E[g + 1]) ++g;
    while (g > 0 && v < E[g]) --g;
    return g;
}

struct HistAcc {
    double mn, mx, sum, sq;
    int fin, nan, inf;
};

__device__ __forceinline__ void hist_take(float x, float scale, HistAcc& a, const double* __restrict__ E, unsigned* __restrict__ H) {
    const float v32 = x * scale;
    if (v32 != v32) {
        ++a.nan;
    } else if (fabsf(v32) == INFINITY) {
        ++a.inf;
    } else {
        ++a.fin;
        const double v = (double)v32;
        a.mn = v < a.mn ? v : a.mn;
        a.mx = v > a.mx ? v : a.mx;
        a.sum += v;
        a.sq += v * v;  // (the product of two fp32 values is exact in float64: fused or not, the sum rounds once)
        atomicAdd(&H[hist_bucket(v, fabsf(v32), E)], 1u);
    }
}

__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// seg: S rows {offset, numel, first chunk}; chunks: n_chunks rows {segment, chunk number inside the segment}.  Both tables come from
// sdt_tensor_hist_plan; every entry is checked again here against S, n and the row it points to, and a row that fails adds nothing.
__global__ __launch_bounds__(HIST_THREADS) void tensor_hist_kernel(const float* __restrict__ flat, int64_t n, const int64_t* __restrict__ seg,
                                                                   int S, const int64_t* __restrict__ chunks,
                                                                   const double* __restrict__ edges, float scale,
                                                                   unsigned long long* __restrict__ counts,
                                                                   unsigned long long* __restrict__ tallies, double* __restrict__ partials) {
    __shared__ double E[HIST_EDGES];
    __shared__ unsigned H[4][HIST_BUCKETS];  // one copy per wave: a hot bucket is contended by 64 lanes, not 256
    __shared__ double red[4][4];
    __shared__ int redi[4][3];
    const int t = threadIdx.x, wave = t >> 6;
    const int64_t c = blockIdx.x;
    const int64_t s = chunks[2 * c], k = chunks[2 * c + 1];
    int64_t off = 0, len = 0;
    if (s >= 0 && s < S && k >= 0 && k < HIST_MAX_CHUNKS) {
        off = seg[3 * s];
        const int64_t numel = seg[3 * s + 1], start = k * HIST_CHUNK;
        if (off >= 0 && (off & 3) == 0 && numel >= 0 && off <= n && numel <= n - off && start < numel && seg[3 * s + 2] + k == c) {
            len = std::min<int64_t>(HIST_CHUNK, numel - start);
            off += start;
        }
    }
    HistAcc a = {INFINITY, -INFINITY, 0.0, 0.0, 0, 0, 0};
    if (len > 0) {  // (uniform over the workgroup)
        for (int i = t; i < HIST_EDGES; i += HIST_THREADS) E[i] = edges[i];
        for (int i = t; i < 4 * HIST_BUCKETS; i += HIST_THREADS) (&H[0][0])[i] = 0u;
        __syncthreads();
        const float* __restrict__ x = flat + off;
        const int nv = (int)(len >> 2), rem = (int)(len & 3);
        unsigned* Hw = H[wave];
#pragma unroll 4
        for (int i = t; i < nv; i += HIST_THREADS) {
            const f32x4 xv = *(const f32x4*)(x + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) hist_take(xv[e], scale, a, E, Hw);
        }
        if (rem && (nv & (HIST_THREADS - 1)) == t)  // the thread whose turn float4 nv would be: its 1 to 3 elements, one by one
            for (int e = 0; e < rem; ++e) hist_take(x[4 * nv + e], scale, a, E, Hw);
        __syncthreads();
        unsigned long long* out = counts + s * HIST_BUCKETS;
        for (int b = t; b < HIST_BUCKETS; b += HIST_THREADS) {
            const unsigned v = H[0][b] + H[1][b] + H[2][b] + H[3][b];
            if (v) atomicAdd(&out[b], (unsigned long long)v);
        }
    }
    const double mn = wave_min_d(a.mn), mx = wave_max_d(a.mx), sum = wave_sum_d(a.sum), sq = wave_sum_d(a.sq);
    const int fin = wave_sum_i(a.fin), nan = wave_sum_i(a.nan), inf = wave_sum_i(a.inf);
    if ((t & 63) == 0) {
        red[wave][0] = mn, red[wave][1] = mx, red[wave][2] = sum, red[wave][3] = sq;
        redi[wave][0] = fin, redi[wave][1] = nan, redi[wave][2] = inf;
    }
    __syncthreads();
    if (t == 0) {
        double* p = partials + 4 * c;
        p[0] = fmin(fmin(red[0][0], red[1][0]), fmin(red[2][0], red[3][0]));
        p[1] = fmax(fmax(red[0][1], red[1][1]), fmax(red[2][1], red[3][1]));
        p[2] = (red[0][2] + red[1][2]) + (red[2][2] + red[3][2]);
        p[3] = (red[0][3] + red[1][3]) + (red[2][3] + red[3][3]);
        if (len > 0) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int v = redi[0][j] + redi[1][j] + redi[2][j] + redi[3][j];
                if (v) atomicAdd(&tallies[3 * s + j], (unsigned long long)v);
            }
        }
    }
}

__global__ __launch_bounds__(HIST_THREADS) void tensor_hist_final_kernel(const int64_t* __restrict__ seg, int64_t n_chunks,
                                                                         const double* __restrict__ partials, double* __restrict__ stats) {
    __shared__ double red[4][4];
    const int t = threadIdx.x, wave = t >> 6;
    const int64_t s = blockIdx.x;
    const int64_t numel = seg[3 * s + 1], first = seg[3 * s + 2];
    int64_t nch = numel > 0 ? (numel + HIST_CHUNK - 1) / HIST_CHUNK : 0;
    if (first < 0 || first > n_chunks || nch > n_chunks - first) nch = 0;
    double mn = INFINITY, mx = -INFINITY, sum = 0.0, sq = 0.0;
    for (int64_t i = t; i < nch; i += HIST_THREADS) {
        const double* p = partials + 4 * (first + i);
        mn = p[0] < mn ? p[0] : mn;
        mx = p[1] > mx ? p[1] : mx;
        sum += p[2];
        sq += p[3];
    }
    mn = wave_min_d(mn), mx = wave_max_d(mx), sum = wave_sum_d(sum), sq = wave_sum_d(sq);
    if ((t & 63) == 0) red[wave][0] = mn, red[wave][1] = mx, red[wave][2] = sum, red[wave][3] = sq;
    __syncthreads();
    if (t == 0) {
        double* o = stats + 4 * s;
        o[0] = fmin(fmin(red[0][0], red[1][0]), fmin(red[2][0], red[3][0]));
        o[1] = fmax(fmax(red[0][1], red[1][1]), fmax(red[2][1], red[3][1]));
        o[2] = (red[0][2] + red[1][2]) + (red[2][2] + red[3][2]);
        o[3] = (red[0][3] + red[1][3]) + (red[2][3] + red[3][3]);
    }
}

// ---------------------------------------------------------------------------------------------
extern "C" int64_t sdt_tensor_hist_threads(void) { return HIST_THREADS; }
extern "C" int64_t sdt_tensor_hist_chunk(void) { return HIST_CHUNK; }
extern "C" int64_t sdt_tensor_hist_buckets(void) { return HIST_BUCKETS; }
extern "C" int64_t sdt_tensor_hist_max_segments(void) { return HIST_MAX_SEGMENTS; }

extern "C" int sdt_tensor_hist_plan(const int64_t* segments, int n_segments, int64_t n, int64_t* seg_plan, int64_t* chunk_plan,
                                    int64_t chunk_rows, int64_t* n_chunks) {
    SDT_CHECK_ARG(n_chunks != nullptr, "bad argument");
    *n_chunks = 0;
    SDT_CHECK_SUPPORTED(n_segments >= 1 && n_segments <= HIST_MAX_SEGMENTS, "between 1 and 65536 segments per call");
    SDT_CHECK_ARG(segments && n >= 0, "bad argument");
    int64_t total = 0;
    for (int s = 0; s < n_segments; ++s) {
        const int64_t off = segments[2 * s], numel = segments[2 * s + 1];
        SDT_CHECK_SUPPORTED(numel < ((int64_t)1 << 32), "a segment has fewer than 2^32 elements");
        SDT_CHECK_ARG(off >= 0 && numel >= 0 && (off & 3) == 0, "a segment starts at a non-negative multiple of 4 elements");
        SDT_CHECK_ARG(off <= n && numel <= n - off, "a segment runs past the end of the buffer");
        const int64_t nch = cdiv64(numel, HIST_CHUNK);
        if (seg_plan) seg_plan[3 * s] = off, seg_plan[3 * s + 1] = numel, seg_plan[3 * s + 2] = total;
        if (chunk_plan) {
            SDT_CHECK_ARG(total + nch <= chunk_rows, "chunk table too small");
            for (int64_t k = 0; k < nch; ++k) chunk_plan[2 * (total + k)] = s, chunk_plan[2 * (total + k) + 1] = k;
        }
        total += nch;
        SDT_CHECK_SUPPORTED(total <= HIST_MAX_CHUNKS, "at most 2^24 chunks per call");
    }
    *n_chunks = total;
    return SDT_OK;
}

extern "C" int sdt_tensor_hist_f32(const float* flat, int64_t n, const int64_t* seg_plan, int n_segments, const int64_t* chunk_plan,
                                   int64_t n_chunks, const double* edges, int n_edges, float scale, int64_t* counts, int64_t* tallies,
                                   double* stats, double* partials, void* stream) {
    SDT_CHECK_SUPPORTED(n_segments >= 1 && n_segments <= HIST_MAX_SEGMENTS, "between 1 and 65536 segments per call");
    SDT_CHECK_SUPPORTED(n_chunks >= 0 && n_chunks <= HIST_MAX_CHUNKS, "at most 2^24 chunks per call");
    SDT_CHECK_ARG(seg_plan && edges && counts && tallies && stats && n >= 0, "bad argument");
    SDT_CHECK_ARG(n_chunks == 0 || (flat && chunk_plan && partials), "bad argument");
    SDT_CHECK_ARG(n_edges == HIST_EDGES, "the edge table has 1549 entries");
    SDT_CHECK_ARG(scale == scale, "scale is NaN");
    SDT_CHECK_ARG(((uintptr_t)flat % 16) == 0 && (((uintptr_t)counts | (uintptr_t)tallies | (uintptr_t)stats | (uintptr_t)partials |
                                                   (uintptr_t)edges | (uintptr_t)seg_plan | (uintptr_t)chunk_plan) % 8) == 0,
                  "flat must be 16-byte aligned, the other buffers 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, sizeof(int64_t) * HIST_BUCKETS * (size_t)n_segments, s) != hipSuccess ||
        hipMemsetAsync(tallies, 0, sizeof(int64_t) * 3 * (size_t)n_segments, s) != hipSuccess) {
        sdt_set_error("%s: could not zero the outputs", __func__);
        return SDT_ERR_LAUNCH;
    }
    if (n_chunks > 0)
        hipLaunchKernelGGL(tensor_hist_kernel, dim3((unsigned)n_chunks), dim3(HIST_THREADS), 0, s, flat, n, seg_plan, n_segments, chunk_plan,
                           edges, scale, (unsigned long long*)counts, (unsigned long long*)tallies, partials);
    hipLaunchKernelGGL(tensor_hist_final_kernel, dim3((unsigned)n_segments), dim3(HIST_THREADS), 0, s, seg_plan, n_chunks, partials, stats);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
