// A custom speaker's pose statistics (data_preprocess/4_1_calculate_mean_std.py + 4_2_parse_mean_std_npz.py of the reference).
// Two kernels.  sdt_speaker_stats_accum_kernel gives one lane to each (chunk, frame, keypoint) of the 4_1 tables and advances
// both modes' running recurrences (parted and global) over a window of clips, in clip order: the state (count, x, y per mode)
// lives in a float64 buffer between windows.  sdt_speaker_stats_final_kernel averages the per-chunk tables over chunks, then
// over frames, in index order (np.average(axis=0) twice), drops the 16 keypoints 4_2 deletes and reports counts and flags.
// Root deduction and the detection test run in the file's element type; everything after it is float64 with every operation
// rounded on its own (exact_f64.h: no FMA contraction), so the results are the reference's bits.  Contract and numbers: DESIGN.md section 11.
#include "exact_f64.h"

namespace {

using sdt_exact::add_rn;
using sdt_exact::div_rn;
using sdt_exact::mul_rn;
using sdt_exact::sub_rn;

constexpr int kKp = 137, kThreads = 256, kFinalThreads = 64, kMaxFrames = 2048;
constexpr int kFields = 7;  // parted n, x, y | global n, x, y | first non-finite row + 1 (0: none)

// the part root of keypoint k in 4_1's pose_np_deduct_root (:66-71): hands on the wrists, face on node 25+30; -1: none
__device__ __forceinline__ int part_root(int k) {
    if (k >= 95 && k < 116) return 7;
    if (k >= 116) return 4;
    if ((k >= 25 && k < 55) || (k >= 56 && k < 95)) return 55;
    return -1;
}

// 4_2's delete_idx = [1] + 8..14 + 17..24: position of keypoint k in the 121-point layout, -1 if deleted
__device__ __forceinline__ int kept_index(int k) {
    if (k == 1 || (k >= 8 && k <= 14) || (k >= 17 && k <= 24)) return -1;
    return k - (k > 1) - min(max(k - 8, 0), 7) - min(max(k - 17, 0), 8);
}

template <typename T>
__device__ __forceinline__ bool skipped(T qx, T qy, T rx, T ry) {
    // 4_1:88-89: abs(q_x + root_x) < 5 and abs(q_y + root_y) < 5, in the array's dtype
    return fabs(qx + rx) < T(5) && fabs(qy + ry) < T(5);
}

// pass 1: avg = avg*w + (1-w)*q (4_1:91-93);  pass 2: var = var*w + (1-w)*(q-M)**2 (4_1:112-115);  w = n/(n+1)
template <bool kVar>
__device__ __forceinline__ void advance(double& n, double& x, double& y, double qx, double qy, double mx, double my) {
    const double w = div_rn(n, add_rn(n, 1.0));
    const double om = sub_rn(1.0, w);
    if (kVar) {
        const double dx = sub_rn(qx, mx), dy = sub_rn(qy, my);
        qx = mul_rn(dx, dx);
        qy = mul_rn(dy, dy);
    }
    x = add_rn(mul_rn(x, w), mul_rn(om, qx));
    y = add_rn(mul_rn(y, w), mul_rn(om, qy));
    n = add_rn(n, 1.0);
}

// poses: clip j of chunk c at poses + c*chunk_pitch + j*F*274, (F, 2, 137) in T.  Lanes = C*F*137, keypoint fastest.
template <typename T, bool kVar>
__global__ void __launch_bounds__(kThreads) sdt_speaker_stats_accum_kernel(const T* __restrict__ poses, int64_t chunk_pitch, int C, int F,
                                                                          int window, int64_t first_row, int64_t rows_per_chunk,
                                                                          const double* __restrict__ mean137, double* __restrict__ state) {
    const int64_t L = (int64_t)C * F * kKp;
    const int64_t lane = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (lane >= L) return;
    const int k = (int)(lane % kKp);
    const int64_t cf = lane / kKp;
    const int f = (int)(cf % F), c = (int)(cf / F);
    const int pr = part_root(k);
    const int64_t clip_elems = (int64_t)F * 2 * kKp;
    const T* p = poses + (int64_t)c * chunk_pitch + (int64_t)f * 2 * kKp;

    double s[kFields];
#pragma unroll
    for (int i = 0; i < kFields; ++i) s[i] = first_row == 0 ? 0.0 : state[i * L + lane];
    double mpx = 0.0, mpy = 0.0, mgx = 0.0, mgy = 0.0;
    if (kVar) {  // mean137: [mode parted, global][x, y][137]
        mpx = mean137[k];
        mpy = mean137[kKp + k];
        mgx = mean137[2 * kKp + k];
        mgy = mean137[3 * kKp + k];
    }
    const int64_t row0 = (int64_t)c * rows_per_chunk + first_row;
    for (int j = 0; j < window; ++j, p += clip_elems) {
        const T px = p[k], py = p[kKp + k];
        const T rx = p[1], ry = p[kKp + 1];  // the same address for every lane of the frame: a broadcast load
        if (s[6] == 0.0 && !(isfinite(px) && isfinite(py))) s[6] = (double)(row0 + j + 1);
        // pose_np_deduct_root (:61-63): every keypoint but the root itself, relative to the root
        const T gx = k == 1 ? px : px - rx, gy = k == 1 ? py : py - ry;
        T qx = gx, qy = gy;
        if (pr >= 0) {  // :66-71, with the part root already root-relative
            qx = gx - (p[pr] - rx);
            qy = gy - (p[kKp + pr] - ry);
        }
        if (!skipped(qx, qy, rx, ry)) advance<kVar>(s[0], s[1], s[2], (double)qx, (double)qy, mpx, mpy);
        if (!skipped(gx, gy, rx, ry)) advance<kVar>(s[3], s[4], s[5], (double)gx, (double)gy, mgx, mgy);
    }
#pragma unroll
    for (int i = 0; i < kFields; ++i) state[i * L + lane] = s[i];
}

// one workgroup per (mode, keypoint).  Thread f: the chunk average of frame f (sequential over chunks, then / C), into LDS;
// thread 0: the frame average (sequential over frames, then / F), the 4_2 layout, the count, the flags.
template <bool kVar>
__global__ void __launch_bounds__(kFinalThreads) sdt_speaker_stats_final_kernel(const double* __restrict__ state, int C, int F,
                                                                                double* __restrict__ out137, double* __restrict__ out242,
                                                                                double* __restrict__ counts, int64_t* __restrict__ first_bad,
                                                                                int32_t* __restrict__ flags) {
    extern __shared__ double lds[];  // [x | y | count | bad] x F
    const int mode = blockIdx.x / kKp, k = blockIdx.x % kKp;
    const int64_t L = (int64_t)C * F * kKp;
    const double* n_f = state + (3 * mode) * L;
    const double* x_f = state + (3 * mode + 1) * L;
    const double* y_f = state + (3 * mode + 2) * L;
    const double* bad_f = state + 6 * L;
    for (int f = threadIdx.x; f < F; f += kFinalThreads) {
        double sx = 0.0, sy = 0.0, cnt = 0.0, bad = 0.0;
        for (int c = 0; c < C; ++c) {
            const int64_t lane = ((int64_t)c * F + f) * kKp + k;
            double vx = x_f[lane], vy = y_f[lane];
            if (kVar) {  // cal_std_*: np.sqrt(np_var) per chunk, before averaging
                vx = __dsqrt_rn(vx);
                vy = __dsqrt_rn(vy);
            }
            sx = add_rn(sx, vx);
            sy = add_rn(sy, vy);
            cnt += n_f[lane];  // integers far below 2^53: exact in any order
            const double b = bad_f[lane];
            if (b != 0.0 && (bad == 0.0 || b < bad)) bad = b;
        }
        lds[f] = div_rn(sx, (double)C);
        lds[F + f] = div_rn(sy, (double)C);
        lds[2 * F + f] = cnt;
        lds[3 * F + f] = bad;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double tx = 0.0, ty = 0.0, cnt = 0.0, bad = 0.0;
    for (int f = 0; f < F; ++f) {
        tx = add_rn(tx, lds[f]);
        ty = add_rn(ty, lds[F + f]);
        cnt += lds[2 * F + f];
        const double b = lds[3 * F + f];
        if (b != 0.0 && (bad == 0.0 || b < bad)) bad = b;
    }
    const double vx = div_rn(tx, (double)F), vy = div_rn(ty, (double)F);
    out137[(2 * mode) * kKp + k] = vx;
    out137[(2 * mode + 1) * kKp + k] = vy;
    counts[mode * kKp + k] = cnt;
    if (mode == 0) first_bad[k] = (int64_t)bad;
    const int kk = kept_index(k);
    int32_t flag = 0;
    if (!(isfinite(vx) && isfinite(vy))) flag |= 1;
    if (kk >= 0) {
        out242[mode * 242 + kk] = vx;
        out242[mode * 242 + 121 + kk] = vy;
        if (kVar && (vx == 0.0 || vy == 0.0)) flag |= 2;
    }
    flags[mode * kKp + k] = flag;
}

template <typename T, bool kVar>
void launch_accum(const void* poses, int64_t chunk_pitch, int C, int F, int window, int64_t first_row, int64_t rows_per_chunk,
                  const double* mean137, double* state, hipStream_t st) {
    const int64_t L = (int64_t)C * F * kKp;
    hipLaunchKernelGGL((sdt_speaker_stats_accum_kernel<T, kVar>), dim3((unsigned)cdiv64(L, kThreads)), dim3(kThreads), 0, st,
                       (const T*)poses, chunk_pitch, C, F, window, first_row, rows_per_chunk, mean137, state);
}

}  // namespace

extern "C" int64_t sdt_speaker_stats_state_bytes(int num_chunks, int num_frames) {
    if (num_chunks <= 0 || num_frames <= 0 || num_frames > kMaxFrames) return 0;
    return (int64_t)kFields * num_chunks * num_frames * kKp * (int64_t)sizeof(double);
}

extern "C" int sdt_speaker_stats_accumulate(int pass, int elem_bytes, const void* poses, int64_t poses_elems, int64_t chunk_pitch,
                                            int num_chunks, int num_frames, int window, int64_t first_row, int64_t rows_per_chunk,
                                            const double* mean137, void* state, int64_t state_bytes, void* stream) {
    SDT_CHECK_ARG(pass == 1 || pass == 2, "pass must be 1 (mean) or 2 (std)");
    SDT_CHECK_ARG(elem_bytes == 4 || elem_bytes == 8, "elem_bytes must be 4 (float32 poses) or 8 (float64 poses)");
    SDT_CHECK_ARG(poses != nullptr && state != nullptr && (pass == 1 || mean137 != nullptr), "null pointer");
    SDT_CHECK_ARG(num_chunks > 0 && num_frames > 0 && num_frames <= kMaxFrames && window > 0, "bad chunk / frame / window count");
    SDT_CHECK_ARG(first_row >= 0 && rows_per_chunk > 0 && first_row + window <= rows_per_chunk, "window outside the chunk");
    const int64_t clip_elems = (int64_t)num_frames * 2 * kKp;
    SDT_CHECK_ARG(chunk_pitch >= (int64_t)window * clip_elems, "chunk_pitch smaller than one window of clips");
    SDT_CHECK_ARG(poses_elems >= (int64_t)(num_chunks - 1) * chunk_pitch + (int64_t)window * clip_elems, "poses buffer too small");
    SDT_CHECK_ARG(state_bytes >= sdt_speaker_stats_state_bytes(num_chunks, num_frames), "state buffer too small");
    hipStream_t st = (hipStream_t)stream;
    double* s = (double*)state;
    if (elem_bytes == 4) {
        if (pass == 1) launch_accum<float, false>(poses, chunk_pitch, num_chunks, num_frames, window, first_row, rows_per_chunk, mean137, s, st);
        else launch_accum<float, true>(poses, chunk_pitch, num_chunks, num_frames, window, first_row, rows_per_chunk, mean137, s, st);
    } else {
        if (pass == 1) launch_accum<double, false>(poses, chunk_pitch, num_chunks, num_frames, window, first_row, rows_per_chunk, mean137, s, st);
        else launch_accum<double, true>(poses, chunk_pitch, num_chunks, num_frames, window, first_row, rows_per_chunk, mean137, s, st);
    }
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_speaker_stats_finalize(int pass, const void* state, int64_t state_bytes, int num_chunks, int num_frames, double* out137,
                                          double* out242, double* counts, int64_t* first_bad_row, int32_t* flags, void* stream) {
    SDT_CHECK_ARG(pass == 1 || pass == 2, "pass must be 1 (mean) or 2 (std)");
    SDT_CHECK_ARG(state != nullptr && out137 != nullptr && out242 != nullptr && counts != nullptr && first_bad_row != nullptr && flags != nullptr,
                  "null pointer");
    SDT_CHECK_ARG(num_chunks > 0 && num_frames > 0 && num_frames <= kMaxFrames, "bad chunk / frame count");
    SDT_CHECK_ARG(state_bytes >= sdt_speaker_stats_state_bytes(num_chunks, num_frames), "state buffer too small");
    const size_t lds = (size_t)4 * num_frames * sizeof(double);
    hipStream_t st = (hipStream_t)stream;
    if (pass == 1)
        hipLaunchKernelGGL((sdt_speaker_stats_final_kernel<false>), dim3(2 * kKp), dim3(kFinalThreads), lds, st, (const double*)state,
                           num_chunks, num_frames, out137, out242, counts, first_bad_row, flags);
    else
        hipLaunchKernelGGL((sdt_speaker_stats_final_kernel<true>), dim3(2 * kKp), dim3(kFinalThreads), lds, st, (const double*)state,
                           num_chunks, num_frames, out137, out242, counts, first_bad_row, flags);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
