// Whole-recording demo (DEMO.LONG_FORM; include/sdt_hip.h states the layouts, DESIGN.md section 23 the contract; long_demo.stitch_model /
// smooth_model / report_model in Python are the same operations in the same order): the audio of overlapping windows gathered out of one
// recording, the windows' final float64 poses cross-faded into one sequence, a Savitzky-Golay filter over time, and a report of speed, jerk
// and the windows' disagreement in the overlaps.
//
// Layout (integers only; long_demo.window_layout is the same function): H = W - O, N = 1 + ceil((F - W) / H), s_i = i H for i < N - 1 and
// s_{N-1} = F - W.  With O <= W / 2 at most two of the regular windows and the last one cover a frame; they are visited in ascending i.
//
// Orders of summation, all fixed:
//   blend            the products w_i x_i of the covering windows in ascending i, the first product is the start of the sum; a frame that one
//                    window covers is a copy of that window's value;
//   smoothing        the products c_j x(clamp(t + j)) for j = -m .. m, the first product is the start of the sum;
//   inside a frame   lane k holds keypoint k's term (+0.0 outside the part and for k >= K); the two waves each run the xor butterfly
//                    v += shfl_xor(v, o) for o = 32, 16, 8, 4, 2, 1, then wave 0 + wave 1 (as csrc/clip_metrics.hip);
//   seam             every lane adds its pair terms in lexicographic (i, j) order from +0.0 before the butterfly;
//   over the frames  chunks of 64 frames, serially in ascending t from +0.0, then the chunk partials in order.
// Every multiply, add, subtract and divide goes through sdt_exact::*_rn (no FMA); counts are integers.  No atomics.
#include "exact_lanes.h"

using namespace sdt_exact;

namespace {

constexpr int kMaxK = 128;
constexpr int kMaxHalf = 8;                // largest half-width of the smoothing filter
constexpr int kGroups = 5;                 // speed, jerk of the stitched poses; speed, jerk of the smoothed poses; seam
constexpr int kSums = kGroups * 4;         // float64 sums of a frame, a chunk and the recording: group g, part p at 4 g + p
constexpr int kPartialWords = 24;          // a frame's / a chunk's partial: the 20 sums, word 20 the int64 number of window pairs
constexpr int kPairs = 20;
constexpr int kChunk = 64;                 // frames per chunk
constexpr int kCols = SDT_LONG_REPORT_COLS;

struct Coeffs {
    double c[2 * kMaxHalf + 1];
};
struct PartSizes {
    int64_t n[4];
};

struct Layout {
    int N, W, O, F, H;
};

__host__ __device__ __forceinline__ int window_start(const Layout& g, int i) { return i < g.N - 1 ? i * g.H : g.F - g.W; }

// the windows that cover frame t in ascending order -> their number (1 .. 3)
__device__ __forceinline__ int covering(const Layout& g, int t, int idx[3]) {
    int n = 0;
    const int lo = t - g.W + 1 <= 0 ? 0 : (t - g.W + g.H) / g.H;  // ceil((t - W + 1) / H)
    const int hi = t / g.H < g.N - 2 ? t / g.H : g.N - 2;         // the regular windows are 0 .. N - 2
    for (int i = lo; i <= hi && n < 2; ++i) idx[n++] = i;
    if (t >= g.F - g.W) idx[n++] = g.N - 1;
    return n;
}

__device__ __forceinline__ int weight(const Layout& g, int t, int s) {
    const int a = t - s + 1, b = s + g.W - t, u = a < b ? a : b, R = g.O > 1 ? g.O : 1;
    return u < R ? u : R;
}

// out[i][j] = audio[offsets[i] + j], 0.0f at or past the end of the recording (and before its start)
__global__ __launch_bounds__(256) void long_gather_kernel(const float* __restrict__ audio, int64_t L, const int64_t* __restrict__ offsets, int Lw,
                                                          float* __restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Lw) return;
    const int64_t src = offsets[blockIdx.y] + j;
    out[(size_t)blockIdx.y * Lw + j] = src >= 0 && src < L ? audio[src] : 0.0f;
}

// one workgroup of 256 threads per output frame; thread c handles coordinate c of the frame's 2 K
__global__ __launch_bounds__(256) void long_stitch_kernel(const double* __restrict__ win, Layout g, int K, double* __restrict__ out) {
    const int t = blockIdx.x, c = threadIdx.x;
    if (c >= 2 * K) return;
    int idx[3];
    const int n = covering(g, t, idx);
    const size_t frame = (size_t)2 * K;
    double x[3];
    int w[3];
    for (int q = 0; q < n; ++q) {
        const int s = window_start(g, idx[q]);
        x[q] = win[((size_t)idx[q] * g.W + (t - s)) * frame + c];
        w[q] = weight(g, t, s);
    }
    double v = x[0];  // one window: its value, bit for bit
    if (n > 1) {
        double num = mul_rn((double)w[0], x[0]);
        int den = w[0];
        for (int q = 1; q < n; ++q) {
            num = add_rn(num, mul_rn((double)w[q], x[q]));
            den += w[q];
        }
        v = div_rn(num, (double)den);
    }
    out[(size_t)t * frame + c] = v;
}

// one workgroup of 256 threads per output frame: y(t) = sum_j c_j x(clamp(t + j, 0, F - 1)), j ascending
__global__ __launch_bounds__(256) void long_smooth_kernel(const double* __restrict__ x, int F, int K, Coeffs cf, int m, double* __restrict__ y) {
    const int t = blockIdx.x, c = threadIdx.x;
    if (c >= 2 * K) return;
    const size_t frame = (size_t)2 * K;
    double s = 0.0;
    for (int j = -m; j <= m; ++j) {
        int u = t + j;
        u = u < 0 ? 0 : (u > F - 1 ? F - 1 : u);
        const double p = mul_rn(cf.c[j + m], x[(size_t)u * frame + c]);
        s = j == -m ? p : add_rn(s, p);
    }
    y[(size_t)t * frame + c] = s;
}

// |x(t + 1) - x(t)| and |x(t + 3) - 3 x(t + 2) + 3 x(t + 1) - x(t)| of keypoint k (+0.0 where the frames do not exist)
__device__ __forceinline__ void motion_terms(const double* __restrict__ x, int t, int F, int K, int k, double& speed, double& jerk) {
    speed = 0.0;
    jerk = 0.0;
    const size_t frame = (size_t)2 * K;
    const double* p = x + (size_t)t * frame;
    if (t + 1 < F) speed = sqrt(norm2(sub_rn(p[frame + k], p[k]), sub_rn(p[frame + K + k], p[K + k])));
    if (t + 3 < F) {
        double d[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const double* q = p + a * K + k;
            d[a] = sub_rn(add_rn(sub_rn(q[3 * frame], mul_rn(3.0, q[2 * frame])), mul_rn(3.0, q[frame])), q[0]);
        }
        jerk = sqrt(norm2(d[0], d[1]));
    }
}

// one workgroup of 128 threads per frame; thread k handles keypoint k
__global__ __launch_bounds__(128) void long_report_frame_kernel(const double* __restrict__ win, const double* __restrict__ stitched,
                                                                const double* __restrict__ smoothed, const uint8_t* __restrict__ parts,
                                                                Layout g, int K, int64_t* __restrict__ work) {
    __shared__ double sred[2][kSums];
    const int t = blockIdx.x, k = threadIdx.x, wave = k >> 6, lane = k & 63;
    const bool on = k < K;
    double term[kGroups] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int part = -1;
    int idx[3];
    const int n = covering(g, t, idx);
    if (on) {
        part = parts[k];
        motion_terms(stitched, t, g.F, K, k, term[0], term[1]);
        if (smoothed) motion_terms(smoothed, t, g.F, K, k, term[2], term[3]);
        if (n > 1) {
            double x[3], y[3];
            for (int q = 0; q < n; ++q) {
                const double* p = win + ((size_t)idx[q] * g.W + (t - window_start(g, idx[q]))) * 2 * K;
                x[q] = p[k];
                y[q] = p[K + k];
            }
            double acc = 0.0;
            for (int i = 0; i < n; ++i)
                for (int j = i + 1; j < n; ++j) acc = add_rn(acc, sqrt(norm2(sub_rn(x[i], x[j]), sub_rn(y[i], y[j]))));
            term[4] = acc;
        }
    }
#pragma unroll
    for (int q = 0; q < kGroups; ++q)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const double v = butterfly_sum(on && in_part(p, part) ? term[q] : 0.0);
            if (lane == 0) sred[wave][q * 4 + p] = v;
        }
    __syncthreads();
    int64_t* w = work + (size_t)t * kPartialWords;
    if (k < kSums) w[k] = __double_as_longlong(add_rn(sred[0][k], sred[1][k]));
    else if (k == kPairs) w[k] = n * (n - 1) / 2;
}

// one wave per chunk of 64 frames: word c of the chunk's partial, frames in ascending order
__global__ __launch_bounds__(64) void long_report_chunk_kernel(const int64_t* __restrict__ work, int F, int64_t* __restrict__ chunks) {
    const int c = threadIdx.x;
    const int t0 = blockIdx.x * kChunk, t1 = t0 + kChunk < F ? t0 + kChunk : F;
    double s = 0.0;
    int64_t h = 0;
    if (c < kSums) {
        for (int t = t0; t < t1; ++t) s = add_rn(s, __longlong_as_double(work[(size_t)t * kPartialWords + c]));
    } else if (c == kPairs) {
        for (int t = t0; t < t1; ++t) h += work[(size_t)t * kPartialWords + c];
    }
    if (c < kPartialWords) chunks[(size_t)blockIdx.x * kPartialWords + c] = c < kSums ? __double_as_longlong(s) : h;
}

// one wave: the chunk partials in order, then the divisions
__global__ __launch_bounds__(64) void long_report_final_kernel(const int64_t* __restrict__ chunks, int n_chunks, Layout g, PartSizes ps,
                                                               int has_smooth, int64_t* __restrict__ out) {
    __shared__ int64_t pairs;
    const int c = threadIdx.x;
    double s = 0.0;
    if (c < kSums) {
        for (int i = 0; i < n_chunks; ++i) s = add_rn(s, __longlong_as_double(chunks[(size_t)i * kPartialWords + c]));
    } else if (c == kPairs) {
        int64_t h = 0;
        for (int i = 0; i < n_chunks; ++i) h += chunks[(size_t)i * kPartialWords + c];
        pairs = h;
    }
    const bool nonfinite = __ballot(c < kSums && !finite_d(s)) != 0;
    __syncthreads();
    const int p = c & 3, q = c >> 2;  // (q: the group of a float word, the kind of count of a count word)
    const int64_t n_speed = (int64_t)(g.F - 1) * ps.n[p], n_jerk = (int64_t)(g.F > 3 ? g.F - 3 : 0) * ps.n[p], n_seam = pairs * ps.n[p];
    if (c < kSums) {
        const int64_t n = q == 4 ? n_seam : ((q & 1) ? n_jerk : n_speed);
        out[c] = __double_as_longlong(n == 0 ? 0.0 : div_rn(s, (double)n));
    } else if (c < 24) {
        out[c] = n_speed;
    } else if (c < 28) {
        out[c] = n_jerk;
    } else if (c < 32) {
        out[c] = n_seam;
    } else if (c == 32) {
        out[c] = nonfinite ? 1 : 0;
    } else if (c == 33) {
        out[c] = g.F;
    } else if (c == 34) {
        out[c] = g.N;
    } else if (c == 35) {
        out[c] = has_smooth;
    } else if (c == 36) {
        out[c] = pairs;
    } else if (c < kCols) {
        out[c] = 0;
    }
}

// the shape rules every entry point shares; the message of the first one broken, or nullptr
const char* layout_error(int N, int W, int O, int F, int K) {
    if (K < 1 || K > kMaxK) return "K outside [1, 128]";
    if (W < 2 || W > (1 << 20)) return "W outside [2, 2^20]";
    if (O < 0 || 2 * O > W) return "overlap outside [0, W / 2]";
    if (F < W || F > (1 << 24)) return "F outside [W, 2^24]";
    if ((int64_t)N != 1 + cdiv64((int64_t)F - W, (int64_t)W - O)) return "N is not 1 + ceil((F - W) / (W - O))";
    return nullptr;
}

}  // namespace

extern "C" int sdt_long_windows_gather_f32(const float* audio, int64_t L, const int64_t* offsets, int n, int Lw, float* out, void* stream) {
    SDT_CHECK_ARG(audio && offsets && out, "null pointer");
    SDT_CHECK_ARG(L >= 1, "empty recording");
    SDT_CHECK_ARG(n >= 1 && n <= 65535, "number of windows outside [1, 65535]");
    SDT_CHECK_ARG(Lw >= 1 && Lw <= (1 << 24), "window length outside [1, 2^24]");
    hipLaunchKernelGGL(long_gather_kernel, dim3((unsigned)cdiv64(Lw, 256), (unsigned)n), dim3(256), 0, (hipStream_t)stream, audio, L, offsets, Lw,
                       out);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_long_stitch_f64(const double* windows, int N, int W, int O, int F, int K, double* out, void* stream) {
    SDT_CHECK_ARG(windows && out, "null pointer");
    const char* err = layout_error(N, W, O, F, K);
    SDT_CHECK_ARG(!err, err);
    const Layout g = {N, W, O, F, W - O};
    hipLaunchKernelGGL(long_stitch_kernel, dim3(F), dim3(256), 0, (hipStream_t)stream, windows, g, K, out);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_long_smooth_f64(const double* x, int F, int K, const double* coeffs, int m, double* y, void* stream) {
    SDT_CHECK_ARG(x && y && coeffs, "null pointer");
    SDT_CHECK_ARG(x != y, "the smoother never runs in place");
    SDT_CHECK_ARG(K >= 1 && K <= kMaxK, "K outside [1, 128]");
    SDT_CHECK_ARG(F >= 1 && F <= (1 << 24), "F outside [1, 2^24]");
    SDT_CHECK_ARG(m >= 1 && m <= kMaxHalf, "half-width outside [1, 8]");
    Coeffs cf;
    for (int j = 0; j < 2 * kMaxHalf + 1; ++j) cf.c[j] = j < 2 * m + 1 ? coeffs[j] : 0.0;
    hipLaunchKernelGGL(long_smooth_kernel, dim3(F), dim3(256), 0, (hipStream_t)stream, x, F, K, cf, m, y);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int64_t sdt_long_report_workspace_bytes(int F) {
    if (F < 1 || F > (1 << 24)) return -1;
    return ((int64_t)F + cdiv64(F, kChunk)) * kPartialWords * 8;
}

extern "C" int sdt_long_report_f64(const double* windows, const double* stitched, const double* smoothed, const uint8_t* parts,
                                   const int64_t* part_sizes, int N, int W, int O, int F, int K, void* work, void* out, void* stream) {
    SDT_CHECK_ARG(windows && stitched && parts && part_sizes && work && out, "null pointer");
    const char* err = layout_error(N, W, O, F, K);
    SDT_CHECK_ARG(!err, err);
    PartSizes ps;
    for (int p = 0; p < 4; ++p) {
        SDT_CHECK_ARG(part_sizes[p] >= 0 && part_sizes[p] <= kMaxK, "part size outside [0, 128]");
        ps.n[p] = part_sizes[p];
    }
    const Layout g = {N, W, O, F, W - O};
    const int n_chunks = (int)cdiv64(F, kChunk);
    int64_t* frames = (int64_t*)work;
    int64_t* chunks = frames + (size_t)F * kPartialWords;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(long_report_frame_kernel, dim3(F), dim3(128), 0, s, windows, stitched, smoothed, parts, g, K, frames);
    hipLaunchKernelGGL(long_report_chunk_kernel, dim3(n_chunks), dim3(64), 0, s, (const int64_t*)frames, F, chunks);
    hipLaunchKernelGGL(long_report_final_kernel, dim3(1), dim3(64), 0, s, (const int64_t*)chunks, n_chunks, g, ps, smoothed ? 1 : 0, (int64_t*)out);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
