// Clip preparation (data_preprocess/2_2_remove_outlier.py, 2_3_rescale_shoulder_width.py, 3_1_generate_clips.py of the reference)
// from one video's per-frame keypoints (N, 3, 137) and its PCM track.  Stages, one kernel each:
//   frame flags      one wave per group of frames: the 2_2 outlier test over the 121 kept keypoints as a wave ballot, the shoulder
//                    distance of 2_3 in float64, a non-finite flag
//   scan             exclusive prefix sum of the keep flags (integers) and the kept frames' distances packed in frame order
//   shoulder means   2_3's serial recurrence avg = avg*(num/(num+1)) + (1 - num/(num+1))*d, one lane per chunk
//   window measure / pack   a window of F frames is a clip iff the prefix sum says all F are kept; the starts are compacted in
//                    ascending order in two passes (count per block, then write at the block's offset)
//   pose gather      (n_clips, F, 3, 137) = the window's frames times the scalar, the product formed in the element type
//   pcm              integer / float PCM -> float32, channels averaged
//   resample         polyphase FIR with float64 taps, float64 accumulation in ascending tap order, one rounding to float32
//   audio gather     per-clip slices with a length table
//   repair (opt-in)  in front of the frame flags: per-point validity and spike marks, gap filling by interpolation into a second
//                    buffer, the filled points per frame and per clip (integers)
//   retime (opt-in)  in front of the repair: keypoints recorded at P/Q fps onto the 15 fps grid, an integer time map and host-designed
//                    taps per phase, float64 sums over the valid source points, into a second buffer
// Every floating-point operation is rounded on its own (contraction is off for the whole file) and no floating-point value is
// accumulated with atomics, so every output is a fixed function of the inputs.  Contract and numbers: DESIGN.md sections 16, 26, 27.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kKp = 137, kFrameElems = 3 * kKp, kThreads = 256, kFramesPerWave = 4;
constexpr int kResTile = 64;                 // outputs per tile of the resampler: one per lane of its single wave
constexpr int kResTilesPerBlock = 8;         // tiles a block walks when every phase's taps are resident (up <= kResTile)
constexpr int64_t kResMaxLds = 60 * 1024;

// 2_2's pose137_to_pose121: 0, 2..7, 15, 16, 25..136
__device__ __forceinline__ bool kept121(int k) { return k == 0 || (k >= 2 && k <= 7) || k == 15 || k == 16 || k >= 25; }

template <typename T>
__global__ void __launch_bounds__(kThreads) clip_frame_flags_kernel(const T* __restrict__ src, const uint8_t* __restrict__ present,
                                                                    int64_t n, int32_t* __restrict__ keep, double* __restrict__ dist,
                                                                    int32_t* __restrict__ bad) {
    const int64_t wave = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / 64;
    const int lane = threadIdx.x & 63;
    for (int g = 0; g < kFramesPerWave; ++g) {
        const int64_t f = wave * kFramesPerWave + g;
        if (f >= n) break;  // uniform over the wave
        const T* p = src + f * kFrameElems;
        const bool pres = present[f] != 0;
        bool outlier = false, nonfinite = false;
        if (pres) {
            for (int k = lane; k < kKp; k += 64) {
                const T x = p[k], y = p[kKp + k];
                nonfinite |= !(isfinite(x) && isfinite(y));
                if (kept121(k)) outlier |= (x <= T(3) && y <= T(3));
            }
        }
        const bool any_out = __ballot(outlier) != 0, any_nf = __ballot(nonfinite) != 0;
        if (lane == 0) {
            const bool kp = pres && !any_out;
            double d = 0.0;
            if (kp) {
                const double dx = (double)p[2] - (double)p[5], dy = (double)p[kKp + 2] - (double)p[kKp + 5];
                d = __dsqrt_rn(dx * dx + dy * dy);
            }
            keep[f] = kp ? 1 : 0;
            bad[f] = (kp && any_nf) ? 1 : 0;
            dist[f] = d;
        }
    }
}

// one workgroup walks the frames in tiles of kThreads: prefix[f] = kept frames before f, prefix[n] = all of them
__global__ void __launch_bounds__(kThreads) clip_scan_kernel(const int32_t* __restrict__ keep, const double* __restrict__ dist, int64_t n,
                                                             int32_t* __restrict__ prefix, double* __restrict__ dist_kept) {
    __shared__ int wsum[kThreads / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carry = 0;
    for (int64_t base = 0; base < n; base += kThreads) {
        const int64_t f = base + threadIdx.x;
        const bool v = f < n && keep[f] != 0;
        const unsigned long long mask = __ballot(v);
        const int excl = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = __popcll(mask);
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int i = 0; i < kThreads / 64; ++i) {
            if (i < w) woff += wsum[i];
            tot += wsum[i];
        }
        const int at = carry + woff + excl;
        if (f < n) {
            prefix[f] = at;
            if (v) dist_kept[at] = dist[f];
        }
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) prefix[n] = carry;
}

// lane c: the running mean of kept frames [c*stride, (c+1)*stride), stride = kept // chunks (2_3:28-43, :50-52)
__global__ void __launch_bounds__(64) clip_shoulder_means_kernel(const double* __restrict__ dist_kept, const int32_t* __restrict__ prefix,
                                                                 int64_t n, int chunks, double* __restrict__ means) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= chunks) return;
    const int64_t stride = (int64_t)prefix[n] / chunks;
    const double* d = dist_kept + (int64_t)c * stride;
    double avg = 0.0, num = 0.0;
    for (int64_t j = 0; j < stride; ++j) {
        const double weight = num / (num + 1.0);
        avg = avg * weight + (1.0 - weight) * d[j];
        num = num + 1.0;
    }
    means[c] = avg;
}

__device__ __forceinline__ bool window_valid(const int32_t* prefix, int64_t i, int64_t n_cand, int start, int step, int F, int* s_out) {
    if (i >= n_cand) return false;
    const int s = start + (int)i * step;
    *s_out = s;
    return prefix[s + F] - prefix[s] == F;
}

// measure (kPack false): block_counts[b] = valid windows among candidates [b*kThreads, (b+1)*kThreads)
// pack (kPack true): the valid starts written in ascending order at the block's offset; the last block writes the total
template <bool kPack>
__global__ void __launch_bounds__(kThreads) clip_windows_kernel(const int32_t* __restrict__ prefix, int64_t n_cand, int start, int step, int F,
                                                                int32_t* __restrict__ block_counts, int32_t* __restrict__ starts,
                                                                int32_t* __restrict__ n_clips) {
    __shared__ int wsum[kThreads / 64];
    __shared__ int s_off;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int s = 0;
    const bool v = window_valid(prefix, (int64_t)blockIdx.x * kThreads + threadIdx.x, n_cand, start, step, F, &s);
    const unsigned long long mask = __ballot(v);
    if (lane == 0) wsum[w] = __popcll(mask);
    if (kPack && threadIdx.x == 0) {
        int off = 0;
        for (unsigned b = 0; b < blockIdx.x; ++b) off += block_counts[b];
        s_off = off;
    }
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) {
        if (i < w) woff += wsum[i];
        tot += wsum[i];
    }
    if (!kPack) {
        if (threadIdx.x == 0) block_counts[blockIdx.x] = tot;
        return;
    }
    if (v) starts[s_off + woff + __popcll(mask & ((1ull << lane) - 1ull))] = s;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_clips = s_off + tot;
}

template <typename T>
__global__ void __launch_bounds__(kThreads) clip_gather_poses_kernel(const T* __restrict__ src, int64_t n, const int32_t* __restrict__ starts,
                                                                     int64_t total, int F, double scalar, int scale_conf, T* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int64_t per_clip = (int64_t)F * kFrameElems;
    const int64_t c = idx / per_clip, rem = idx % per_clip;
    const int i = (int)(rem / kFrameElems), e = (int)(rem % kFrameElems);
    const int64_t f = (int64_t)starts[c] + i;
    if (f < 0 || f >= n) return;  // (starts come from the pack pass, which only emits windows inside the video)
    T v = src[f * kFrameElems + e];
    if (e < 2 * kKp || scale_conf) v = v * (T)scalar;  // numpy: array * python float, the float converted to the array's dtype first
    out[idx] = v;
}

// fmt 0: uint8, 1: int16, 2: int32, 3: float32 (gesture_dataset._demo_item's divisors); channel mean in numpy's float32 order:
// left to right below eight channels, the pairwise tree at eight
__global__ void __launch_bounds__(kThreads) clip_pcm_kernel(int fmt, const void* __restrict__ pcm, int64_t n, int channels, int64_t first,
                                                            float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n - first) return;
    const int64_t base = (first + i) * channels;
    float r[8];
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) {
        float v = 0.f;
        if (ch < channels) {
            if (fmt == 0) v = ((float)((const uint8_t*)pcm)[base + ch] - 128.0f) / 128.0f;
            else if (fmt == 1) v = (float)((const int16_t*)pcm)[base + ch] / 32768.0f;
            else if (fmt == 2) v = (float)((const int32_t*)pcm)[base + ch] / 2147483648.0f;
            else v = ((const float*)pcm)[base + ch];
        }
        r[ch] = v;
    }
    float sum;
    if (channels == 8) {  // numpy's pairwise sum takes eight values as a tree
        sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    } else {
        sum = r[0];
        for (int ch = 1; ch < channels; ++ch) sum = sum + r[ch];
    }
    out[i] = channels == 1 ? r[0] : sum / (float)channels;
}

// y[j] = sum over q of taps[k0 + up*q] * x[t/up - q], t = (j + n_pre_remove)*down, k0 = t % up: upfirdn's zero-extended sum in
// ascending tap order.  One wave, one output per lane.  LDS: the taps of the tile's phases (all `up` phases when up <= kResTile:
// staged once for every tile the block walks; else one phase per lane, staged per tile) and the input span of the tile.
__global__ void __launch_bounds__(kResTile) clip_resample_kernel(const float* __restrict__ x, int64_t n_in, const double* __restrict__ taps,
                                                                 int n_taps, int up, int down, int64_t n_pre_remove, int q_max, int span_max,
                                                                 int tiles_per_block, float* __restrict__ y, int64_t n_out) {
    extern __shared__ double res_lds[];
    const int slots = up <= kResTile ? up : kResTile;
    double* s_taps = res_lds;                              // [q][slot]
    float* s_x = (float*)(res_lds + (size_t)q_max * slots);  // [span_max]
    const int lane = threadIdx.x;
    for (int r = 0; r < tiles_per_block; ++r) {
        const int64_t j0 = ((int64_t)blockIdx.x * tiles_per_block + r) * kResTile;
        if (j0 >= n_out) break;  // uniform
        const int64_t j = j0 + lane;
        const int64_t t = (j + n_pre_remove) * down;
        const int k0 = (int)(t % up);
        const int64_t ib = t / up;
        const int slot = up <= kResTile ? k0 : lane;
        if (r == 0 || up > kResTile) {
            if (up <= kResTile) {
                for (int e = lane; e < q_max * slots; e += kResTile) {
                    const int q = e / slots, ph = e % slots;
                    const int64_t k = (int64_t)ph + (int64_t)up * q;
                    s_taps[e] = k < n_taps ? taps[k] : 0.0;
                }
            } else {
                for (int q = 0; q < q_max; ++q) {
                    const int64_t k = (int64_t)k0 + (int64_t)up * q;
                    s_taps[q * slots + lane] = k < n_taps ? taps[k] : 0.0;
                }
            }
        }
        // input span of the tile: [lo, lo + span_max), lo = the lowest index any lane reads
        const int64_t lo = ((j0 + n_pre_remove) * down) / up - (q_max - 1);
        for (int e = lane; e < span_max; e += kResTile) {
            const int64_t i = lo + e;
            s_x[e] = (i >= 0 && i < n_in) ? x[i] : 0.f;
        }
        __syncthreads();
        if (j < n_out) {
            double acc = 0.0;
            for (int q = 0; q < q_max; ++q) {
                const int64_t i = ib - q;
                if (i < 0) break;
                if ((int64_t)k0 + (int64_t)up * q >= n_taps) break;
                if (i >= n_in) continue;
                const double prod = s_taps[q * slots + slot] * (double)s_x[(int)(i - lo)];
                acc = acc + prod;
            }
            y[j] = (float)acc;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kThreads) clip_gather_audio_kernel(const float* __restrict__ audio, int64_t n_audio, const int64_t* __restrict__ a0,
                                                                     const int64_t* __restrict__ a1, int64_t l_max, float* __restrict__ out,
                                                                     int32_t* __restrict__ lengths) {
    const int c = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int64_t b = a0[c] < 0 ? 0 : a0[c], e = a1[c] < 0 ? 0 : a1[c];
    b = b > n_audio ? n_audio : b;
    e = e > n_audio ? n_audio : e;
    const int64_t len = e > b ? e - b : 0;  // numpy's interval[a0:a1]: short or empty past the end
    if (i == 0) lengths[c] = (int32_t)len;
    if (i < l_max) out[(int64_t)c * l_max + i] = i < len ? audio[b + i] : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------------- repair
// Opt-in stage in front of the frame flags: short gaps of a keypoint's track are filled by interpolation between
// the nearest valid frames, isolated jumps are marked first and filled the same way.  Out of place: src is read, src_r is written.

constexpr int kRepairMaxGap = 64, kRepairMaxHalf = 3, kRepairWin = 2 * kRepairMaxHalf + 1;

// the 2_2 rule per point, on a frame that has a file; a non-finite coordinate is invalid
template <typename T>
__device__ __forceinline__ bool point_valid(const T* __restrict__ src, const uint8_t* __restrict__ present, int64_t f, int k, T* x_out, T* y_out) {
    const T x = src[f * kFrameElems + k], y = src[f * kFrameElems + kKp + k];
    *x_out = x;
    *y_out = y;
    return present[f] != 0 && isfinite(x) && isfinite(y) && !(x <= T(3) && y <= T(3));
}

// ascending; the unused slots hold +inf and end up behind the m values
__device__ __forceinline__ void sort_win(double (&s)[kRepairWin]) {
#pragma unroll
    for (int i = 0; i < kRepairWin - 1; ++i) {
#pragma unroll
        for (int j = 0; j < kRepairWin - 1 - i; ++j) {
            const double a = s[j], b = s[j + 1];
            const bool swap = a > b;
            s[j] = swap ? b : a;
            s[j + 1] = swap ? a : b;
        }
    }
}

__device__ __forceinline__ double median_win(const double (&s)[kRepairWin], int m) {
    const int lo = (m - 1) / 2, hi = m / 2;
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int i = 0; i < kRepairWin; ++i) {
        if (i == lo) a = s[i];
        if (i == hi) b = s[i];
    }
    return 0.5 * (a + b);
}

// |v - med| > kappa * (1.4826 * mad) + floor_px over the m values of s (m >= 3, the other slots +inf)
__device__ __forceinline__ bool spike_coord(double (&s)[kRepairWin], int m, double v, double kappa, double floor_px) {
    sort_win(s);
    const double med = median_win(s, m);
    double d[kRepairWin];
#pragma unroll
    for (int i = 0; i < kRepairWin; ++i) d[i] = i < m ? fabs(s[i] - med) : (double)INFINITY;
    sort_win(d);
    const double mad = median_win(d, m);
    const double bar = kappa * (1.4826 * mad) + floor_px;
    return fabs(v - med) > bar;
}

// one thread per (frame, keypoint): valid = the point's own test, minus the spikes; every verdict reads src alone
template <typename T>
__global__ void __launch_bounds__(kThreads) clip_repair_valid_kernel(const T* __restrict__ src, const uint8_t* __restrict__ present, int64_t n,
                                                                     int half, double kappa, double floor_px, uint8_t* __restrict__ valid,
                                                                     uint8_t* __restrict__ spike) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n * kKp) return;
    const int64_t f = idx / kKp;
    const int k = (int)(idx % kKp);
    T x, y;
    const bool ok = point_valid(src, present, f, k, &x, &y);
    bool sp = false;
    if (half > 0 && ok) {
        double xs[kRepairWin], ys[kRepairWin];
        int m = 0;
#pragma unroll
        for (int d = -kRepairMaxHalf; d <= kRepairMaxHalf; ++d) {
            const int64_t g = f + d;
            T gx = T(0), gy = T(0);
            const bool in = d >= -half && d <= half && g >= 0 && g < n && point_valid(src, present, g, k, &gx, &gy);
            xs[d + kRepairMaxHalf] = in ? (double)gx : (double)INFINITY;
            ys[d + kRepairMaxHalf] = in ? (double)gy : (double)INFINITY;
            m += in ? 1 : 0;
        }
        if (m >= 3) {
            const bool sx = spike_coord(xs, m, (double)x, kappa, floor_px), sy = spike_coord(ys, m, (double)y, kappa, floor_px);
            sp = sx || sy;
        }
    }
    valid[idx] = (ok && !sp) ? 1 : 0;
    spike[idx] = sp ? 1 : 0;
}

// one wave per group of frames, lanes over the keypoints.  An invalid point looks back and forth along its track for the nearest
// valid frames a < f < b (at most max_gap + 1 steps in all: b - a - 1 <= max_gap) and is filled with xa + (xb - xa) * ((f - a) / (b - a))
// in float64, rounded once to T, confidence 0; the filled kept keypoints of a frame are counted with ballots.
template <typename T>
__global__ void __launch_bounds__(kThreads) clip_repair_fill_kernel(const T* __restrict__ src, const uint8_t* __restrict__ present,
                                                                    const uint8_t* __restrict__ valid, int64_t n, int max_gap,
                                                                    T* __restrict__ src_r, uint8_t* __restrict__ present_r,
                                                                    uint8_t* __restrict__ filled, int32_t* __restrict__ per_frame) {
    const int64_t wave = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / 64;
    const int lane = threadIdx.x & 63;
    for (int g = 0; g < kFramesPerWave; ++g) {
        const int64_t f = wave * kFramesPerWave + g;
        if (f >= n) break;  // uniform over the wave
        const T* p = src + f * kFrameElems;
        T* q = src_r + f * kFrameElems;
        int count = 0;
        for (int k0 = 0; k0 < kKp; k0 += 64) {  // (uniform: every lane reaches the ballot)
            const int k = k0 + lane;
            bool fill = false;
            if (k < kKp) {
                T x = p[k], y = p[kKp + k], c = p[2 * kKp + k];
                if (valid[f * kKp + k] == 0) {
                    int64_t a = -1, b = -1;
                    for (int d = 1; d <= max_gap && f - d >= 0; ++d) {
                        if (valid[(f - d) * kKp + k] != 0) {
                            a = f - d;
                            break;
                        }
                    }
                    if (a >= 0) {
                        const int reach = max_gap + 1 - (int)(f - a);  // b <= a + max_gap + 1
                        for (int d = 1; d <= reach && f + d < n; ++d) {
                            if (valid[(f + d) * kKp + k] != 0) {
                                b = f + d;
                                break;
                            }
                        }
                    }
                    if (b >= 0) {
                        const T* pa = src + a * kFrameElems;
                        const T* pb = src + b * kFrameElems;
                        const double t = (double)(f - a) / (double)(b - a);
                        const double xa = (double)pa[k], xb = (double)pb[k], ya = (double)pa[kKp + k], yb = (double)pb[kKp + k];
                        x = (T)(xa + (xb - xa) * t);
                        y = (T)(ya + (yb - ya) * t);
                        c = T(0);
                        fill = true;
                    }
                }
                q[k] = x;
                q[kKp + k] = y;
                q[2 * kKp + k] = c;
                filled[f * kKp + k] = fill ? 1 : 0;
            }
            count += __popcll(__ballot(fill && kept121(k)));
        }
        if (lane == 0) {
            per_frame[f] = count;
            present_r[f] = (present[f] != 0 || count == 121) ? 1 : 0;
        }
    }
}

// one workgroup walks the frames in tiles of kThreads: prefix[f] = repaired kept keypoints before frame f (integers), prefix[n] = all
__global__ void __launch_bounds__(kThreads) clip_repair_prefix_kernel(const int32_t* __restrict__ per_frame, int64_t n, int64_t* __restrict__ prefix) {
    __shared__ int wsum[kThreads / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += kThreads) {
        const int64_t f = base + threadIdx.x;
        const int v = f < n ? per_frame[f] : 0;
        int incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int i = 0; i < kThreads / 64; ++i) {
            if (i < w) woff += wsum[i];
            tot += wsum[i];
        }
        if (f < n) prefix[f] = carry + woff + incl - v;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) prefix[n] = carry;
}

__global__ void __launch_bounds__(kThreads) clip_repair_clip_counts_kernel(const int64_t* __restrict__ prefix, int64_t n,
                                                                           const int32_t* __restrict__ starts, int64_t n_clips, int F,
                                                                           int32_t* __restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= n_clips) return;
    const int64_t s = starts[c];
    out[c] = (s >= 0 && s + F <= n) ? (int32_t)(prefix[s + F] - prefix[s]) : -1;  // (the pack pass only emits windows inside the video)
}

// ------------------------------------------------------------------------------------------------------------------------- retime
// Opt-in stage in front of the repair stage: keypoints recorded at P/Q fps are resampled onto the 15 fps grid.
// Output frame j sits at source time j*P/D frames, D = 15*Q: a = j*P / D, r = j*P % D in int64 (no floating-point time), phase r / g,
// g = gcd(P, D).  Row `phase` of the host-designed tap table weighs source frames a + i_lo .. a + i_lo + L - 1, i_lo = 1 - L/2; a tap of
// weight 0 takes part in nothing.  Out of place: src is read, src_t is written.

constexpr int kRetimeFrames = kFramesPerWave * (kThreads / 64);  // consecutive output frames of a workgroup
constexpr int kRetimeMaxTaps = 32, kRetimeMaxPhases = 16384;

struct RetimePlan {
    int64_t d, g, n_out, blocks_out, blocks_src;
};

bool retime_plan(int64_t n_src, int64_t p, int64_t q, RetimePlan* rp) {
    if (p < 1 || p > (1 << 20) || q < 1 || q > (1 << 16) || p < q || p > 240 * q) return false;  // 1 <= P/Q <= 240
    if (n_src <= 0 || n_src > (1 << 30)) return false;
    const int64_t d = 15 * q;
    int64_t a = p, b = d;
    while (b != 0) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    if (d / a > kRetimeMaxPhases) return false;
    const int64_t n_out = (n_src - 1) * d / p + 1;  // below 2^51
    if (n_out > (1 << 30)) return false;
    rp->d = d;
    rp->g = a;
    rp->n_out = n_out;
    rp->blocks_out = cdiv64(n_out, kRetimeFrames);
    rp->blocks_src = cdiv64(n_src * kKp, kThreads);
    return true;
}

// one workgroup per kRetimeFrames consecutive output frames: the time map of each frame once (16 threads), the tap rows of their
// phases in LDS, then the frame-flags shape: a wave per kFramesPerWave frames, the lanes over the keypoints, every source row read
// coalesced.  float64 products and sums in ascending tap order, each rounded on its own; one rounding to T.
template <typename T>
__global__ void __launch_bounds__(kThreads) clip_retime_kernel(const T* __restrict__ src, const uint8_t* __restrict__ present, int64_t n_src,
                                                               int64_t p, int64_t d, int64_t g, const double* __restrict__ taps, int n_taps,
                                                               double min_support, int64_t n_out, T* __restrict__ src_t,
                                                               uint8_t* __restrict__ present_t, uint8_t* __restrict__ valid_t,
                                                               uint8_t* __restrict__ taps_used, int32_t* __restrict__ nearest_src,
                                                               int32_t* __restrict__ block_invalid) {
    __shared__ double s_taps[kRetimeFrames * kRetimeMaxTaps];
    __shared__ int64_t s_a[kRetimeFrames];
    __shared__ int s_phase[kRetimeFrames], s_near[kRetimeFrames], s_count[kThreads / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t j0 = (int64_t)blockIdx.x * kRetimeFrames;
    if (threadIdx.x < kRetimeFrames) {
        const int64_t j = j0 + threadIdx.x;
        int64_t a = 0, r = 0;
        if (j < n_out) {
            const int64_t prod = j * p;  // below 2^50
            a = prod / d;
            r = prod - a * d;
        }
        s_a[threadIdx.x] = a;
        s_phase[threadIdx.x] = (int)((int)r / (int)g);  // r < d <= 15 * 2^16
        s_near[threadIdx.x] = 2 * r < d ? 0 : 1;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kRetimeFrames * n_taps; e += kThreads) {
        const int s = e / n_taps, i = e - s * n_taps;
        s_taps[s * kRetimeMaxTaps + i] = taps[(int64_t)s_phase[s] * n_taps + i];  // phase < d / g = the table's rows
    }
    __syncthreads();
    const int i_lo = 1 - n_taps / 2;
    int invalid = 0;
    for (int fg = 0; fg < kFramesPerWave; ++fg) {
        const int s = w * kFramesPerWave + fg;
        const int64_t j = j0 + s;
        if (j < n_out) {  // uniform over the wave
            const int64_t a = s_a[s];
            const double* h = s_taps + s * kRetimeMaxTaps;
            double full = 0.0;
            bool any_present = false;
            for (int i = 0; i < n_taps; ++i) {
                if (h[i] == 0.0) continue;
                full = full + h[i];
                const int64_t f = a + i_lo + i;
                any_present |= f >= 0 && f < n_src && present[f] != 0;
            }
            const double need = min_support * full;
            for (int k0 = 0; k0 < kKp; k0 += 64) {  // (uniform: every lane reaches the ballot)
                const int k = k0 + lane;
                bool ok = false;
                if (k < kKp) {
                    double nx = 0.0, ny = 0.0, nc = 0.0, den = 0.0;
                    int used = 0;
                    for (int i = 0; i < n_taps; ++i) {
                        const double hi = h[i];
                        const int64_t f = a + i_lo + i;
                        if (hi == 0.0 || f < 0 || f >= n_src) continue;  // uniform
                        T x, y;
                        if (!point_valid(src, present, f, k, &x, &y)) continue;
                        const double px = hi * (double)x, py = hi * (double)y, pc = hi * (double)src[f * kFrameElems + 2 * kKp + k];
                        nx = used ? nx + px : px;
                        ny = used ? ny + py : py;
                        nc = used ? nc + pc : pc;
                        den = den + hi;
                        ++used;
                    }
                    ok = den > 0.0 && den >= need;
                    T* o = src_t + j * kFrameElems;
                    o[k] = ok ? (T)(nx / den) : T(0);
                    o[kKp + k] = ok ? (T)(ny / den) : T(0);
                    o[2 * kKp + k] = ok ? (T)(nc / den) : T(0);
                    valid_t[j * kKp + k] = ok ? 1 : 0;
                    taps_used[j * kKp + k] = (uint8_t)used;
                }
                invalid += __popcll(__ballot(k < kKp && !ok));
            }
            if (lane == 0) {
                present_t[j] = any_present ? 1 : 0;
                const int64_t nf = a + s_near[s];
                nearest_src[j] = (int32_t)(nf < n_src ? nf : n_src - 1);
            }
        }
    }
    if (lane == 0) s_count[w] = invalid;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int i = 0; i < kThreads / 64; ++i) tot += s_count[i];
        block_invalid[blockIdx.x] = tot;
    }
}

// one thread per source point: block_counts[2b] = invalid points, [2b + 1] = points with a non-finite x or y, of the block's points
template <typename T>
__global__ void __launch_bounds__(kThreads) clip_retime_source_counts_kernel(const T* __restrict__ src, const uint8_t* __restrict__ present,
                                                                             int64_t n_src, int32_t* __restrict__ block_counts) {
    __shared__ int s_inv[kThreads / 64], s_nf[kThreads / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    bool inv = false, nf = false;
    if (idx < n_src * kKp) {
        T x, y;
        inv = !point_valid(src, present, idx / kKp, (int)(idx % kKp), &x, &y);
        nf = !(isfinite(x) && isfinite(y));
    }
    const int c_inv = __popcll(__ballot(inv)), c_nf = __popcll(__ballot(nf));
    if (lane == 0) {
        s_inv[w] = c_inv;
        s_nf[w] = c_nf;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0, b = 0;
        for (int i = 0; i < kThreads / 64; ++i) {
            a += s_inv[i];
            b += s_nf[i];
        }
        block_counts[2 * (int64_t)blockIdx.x] = a;
        block_counts[2 * (int64_t)blockIdx.x + 1] = b;
    }
}

// one workgroup: counts[0] = invalid source points, [1] = non-finite source points, [2] = invalid output points (integers: any order)
__global__ void __launch_bounds__(kThreads) clip_retime_total_kernel(const int32_t* __restrict__ block_invalid, int64_t blocks_out,
                                                                     const int32_t* __restrict__ block_counts, int64_t blocks_src,
                                                                     int64_t* __restrict__ counts) {
    __shared__ int64_t s_sum[3][kThreads];
    int64_t a = 0, b = 0, c = 0;
    for (int64_t i = threadIdx.x; i < blocks_src; i += kThreads) {
        a += block_counts[2 * i];
        b += block_counts[2 * i + 1];
    }
    for (int64_t i = threadIdx.x; i < blocks_out; i += kThreads) c += block_invalid[i];
    s_sum[0][threadIdx.x] = a;
    s_sum[1][threadIdx.x] = b;
    s_sum[2][threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x < 3) {
        int64_t tot = 0;
        for (int i = 0; i < kThreads; ++i) tot += s_sum[threadIdx.x][i];
        counts[threadIdx.x] = tot;
    }
}

struct ResPlan {
    int q_max, span_max, slots, tiles_per_block;
    int64_t lds;
};

bool res_plan(int n_taps, int up, int down, ResPlan* p) {
    if (n_taps <= 0 || up <= 0 || down <= 0 || up > (1 << 20) || down > (1 << 20)) return false;
    p->q_max = (n_taps + up - 1) / up;
    p->slots = up <= kResTile ? up : kResTile;
    // lanes of a tile read inputs [lo, hi]: lo = first lane's t/up - (q_max-1), hi = last lane's t/up
    const int64_t span = ((int64_t)(kResTile - 1) * down + up - 1) / up + 1 + p->q_max;
    if (span > (1 << 20)) return false;
    p->span_max = (int)span;
    p->tiles_per_block = up <= kResTile ? kResTilesPerBlock : 1;
    p->lds = (int64_t)p->q_max * p->slots * (int64_t)sizeof(double) + (int64_t)p->span_max * (int64_t)sizeof(float);
    return p->lds <= kResMaxLds;
}

}  // namespace

extern "C" int64_t sdt_clip_workspace_bytes(int64_t n_frames) {
    if (n_frames <= 0 || n_frames > (1 << 30)) return -1;
    return cdiv64(n_frames, kThreads) * (int64_t)sizeof(int32_t);  // one count per block of window candidates (at most n_frames of them)
}

extern "C" int sdt_clip_frame_flags(int elem_bytes, const void* src, const void* present, int64_t n_frames, int32_t* keep, double* dist,
                                    int32_t* bad, void* stream) {
    SDT_CHECK_ARG(elem_bytes == 4 || elem_bytes == 8, "elem_bytes must be 4 (float32 keypoints) or 8 (float64 keypoints)");
    SDT_CHECK_ARG(src != nullptr && present != nullptr && keep != nullptr && dist != nullptr && bad != nullptr, "null pointer");
    SDT_CHECK_ARG(n_frames > 0 && n_frames <= (1 << 30), "bad frame count");
    const unsigned grid = (unsigned)cdiv64(n_frames, (int64_t)kFramesPerWave * (kThreads / 64));
    hipStream_t st = (hipStream_t)stream;
    if (elem_bytes == 4)
        hipLaunchKernelGGL((clip_frame_flags_kernel<float>), dim3(grid), dim3(kThreads), 0, st, (const float*)src, (const uint8_t*)present,
                           n_frames, keep, dist, bad);
    else
        hipLaunchKernelGGL((clip_frame_flags_kernel<double>), dim3(grid), dim3(kThreads), 0, st, (const double*)src, (const uint8_t*)present,
                           n_frames, keep, dist, bad);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_clip_scan(const int32_t* keep, const double* dist, int64_t n_frames, int32_t* prefix, double* dist_kept, void* stream) {
    SDT_CHECK_ARG(keep != nullptr && dist != nullptr && prefix != nullptr && dist_kept != nullptr, "null pointer");
    SDT_CHECK_ARG(n_frames > 0 && n_frames <= (1 << 30), "bad frame count");
    hipLaunchKernelGGL(clip_scan_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, keep, dist, n_frames, prefix, dist_kept);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_clip_shoulder_means(const double* dist_kept, const int32_t* prefix, int64_t n_frames, int chunks, double* means, void* stream) {
    SDT_CHECK_ARG(dist_kept != nullptr && prefix != nullptr && means != nullptr, "null pointer");
    SDT_CHECK_ARG(n_frames > 0 && n_frames <= (1 << 30), "bad frame count");
    SDT_CHECK_ARG(chunks >= 1 && chunks <= 65536, "shoulder chunks must be in [1, 65536]");
    hipLaunchKernelGGL(clip_shoulder_means_kernel, dim3((unsigned)cdiv(chunks, 64)), dim3(64), 0, (hipStream_t)stream, dist_kept, prefix, n_frames,
                       chunks, means);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int64_t sdt_clip_window_candidates(int64_t n_frames, int start_frame, int num_frames, int step) {
    if (n_frames <= 0 || n_frames > (1 << 30) || start_frame < 0 || num_frames <= 0 || step <= 0) return -1;
    const int64_t stop = n_frames - num_frames;  // range(start, n - F, step)
    return stop > start_frame ? (stop - start_frame + step - 1) / step : 0;
}

extern "C" int sdt_clip_windows(const int32_t* prefix, int64_t n_frames, int start_frame, int num_frames, int step, void* workspace,
                                int64_t workspace_bytes, int32_t* starts, int64_t starts_capacity, int32_t* n_clips, void* stream) {
    SDT_CHECK_ARG(prefix != nullptr && workspace != nullptr && starts != nullptr && n_clips != nullptr, "null pointer");
    const int64_t n_cand = sdt_clip_window_candidates(n_frames, start_frame, num_frames, step);
    SDT_CHECK_ARG(n_cand >= 0, "bad frame count / start / window / step");
    SDT_CHECK_ARG(starts_capacity >= n_cand, "starts buffer smaller than the candidate count");
    SDT_CHECK_ARG(workspace_bytes >= sdt_clip_workspace_bytes(n_frames), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (n_cand == 0) {  // a video shorter than start + window: zero clips, nothing to launch but the count
        if (hipMemsetAsync(n_clips, 0, sizeof(int32_t), st) != hipSuccess) return SDT_ERR_LAUNCH;
        return SDT_OK;
    }
    const unsigned grid = (unsigned)cdiv64(n_cand, kThreads);
    int32_t* counts = (int32_t*)workspace;
    hipLaunchKernelGGL((clip_windows_kernel<false>), dim3(grid), dim3(kThreads), 0, st, prefix, n_cand, start_frame, step, num_frames, counts,
                       starts, n_clips);
    hipLaunchKernelGGL((clip_windows_kernel<true>), dim3(grid), dim3(kThreads), 0, st, prefix, n_cand, start_frame, step, num_frames, counts,
                       starts, n_clips);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_clip_gather_poses(int elem_bytes, const void* src, int64_t n_frames, const int32_t* starts, int64_t n_clips, int num_frames,
                                     double scalar, int scale_confidence, void* out, int64_t out_elems, void* stream) {
    SDT_CHECK_ARG(elem_bytes == 4 || elem_bytes == 8, "elem_bytes must be 4 or 8");
    SDT_CHECK_ARG(src != nullptr && starts != nullptr && out != nullptr, "null pointer");
    SDT_CHECK_ARG(n_frames > 0 && n_clips > 0 && num_frames > 0 && num_frames <= n_frames, "bad frame / clip / window count");
    const int64_t total = n_clips * num_frames * kFrameElems;
    SDT_CHECK_ARG(out_elems >= total, "output buffer too small");
    SDT_CHECK_ARG(cdiv64(total, kThreads) <= 0x7fffffff, "too many clips for one launch");
    const unsigned grid = (unsigned)cdiv64(total, kThreads);
    hipStream_t st = (hipStream_t)stream;
    if (elem_bytes == 4)
        hipLaunchKernelGGL((clip_gather_poses_kernel<float>), dim3(grid), dim3(kThreads), 0, st, (const float*)src, n_frames, starts, total,
                           num_frames, scalar, scale_confidence, (float*)out);
    else
        hipLaunchKernelGGL((clip_gather_poses_kernel<double>), dim3(grid), dim3(kThreads), 0, st, (const double*)src, n_frames, starts, total,
                           num_frames, scalar, scale_confidence, (double*)out);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_clip_pcm_to_mono_f32(int fmt, const void* pcm, int64_t n_samples, int channels, int64_t first, float* out, int64_t out_elems,
                                        void* stream) {
    SDT_CHECK_ARG(fmt >= 0 && fmt <= 3, "fmt must be 0 (uint8), 1 (int16), 2 (int32) or 3 (float32)");
    SDT_CHECK_ARG(pcm != nullptr && out != nullptr, "null pointer");
    SDT_CHECK_ARG(channels >= 1 && channels <= 8, "1 to 8 channels");
    SDT_CHECK_ARG(n_samples > 0 && first >= 0 && first < n_samples, "cut outside the track");
    SDT_CHECK_ARG(out_elems >= n_samples - first, "output buffer too small");
    SDT_CHECK_ARG(cdiv64(n_samples - first, kThreads) <= 0x7fffffff, "track too long for one launch");
    hipLaunchKernelGGL(clip_pcm_kernel, dim3((unsigned)cdiv64(n_samples - first, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, fmt, pcm,
                       n_samples, channels, first, out);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int64_t sdt_clip_resample_lds_bytes(int n_taps, int up, int down) {
    ResPlan p;
    return res_plan(n_taps, up, down, &p) ? p.lds : -1;
}

extern "C" int sdt_clip_resample_f32(const float* x, int64_t n_in, const double* taps, int n_taps, int up, int down, int64_t n_pre_remove,
                                     float* y, int64_t n_out, void* stream) {
    SDT_CHECK_ARG(x != nullptr && taps != nullptr && y != nullptr, "null pointer");
    ResPlan p;
    SDT_CHECK_ARG(res_plan(n_taps, up, down, &p), "unsupported filter length / ratio");
    SDT_CHECK_ARG(n_in > 0 && n_out > 0 && n_pre_remove >= 0, "bad lengths");
    SDT_CHECK_ARG(n_in <= ((int64_t)1 << 40) / up && n_out + n_pre_remove <= ((int64_t)1 << 40) / down, "track too long");
    const int64_t blocks = cdiv64(n_out, (int64_t)kResTile * p.tiles_per_block);
    SDT_CHECK_ARG(blocks <= 0x7fffffff, "track too long for one launch");
    hipLaunchKernelGGL(clip_resample_kernel, dim3((unsigned)blocks), dim3(kResTile), (size_t)p.lds, (hipStream_t)stream, x, n_in, taps, n_taps, up,
                       down, n_pre_remove, p.q_max, p.span_max, p.tiles_per_block, y, n_out);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_clip_gather_audio(const float* audio, int64_t n_audio, const int64_t* a0, const int64_t* a1, int64_t n_clips, int64_t l_max,
                                     float* out, int64_t out_elems, int32_t* lengths, void* stream) {
    SDT_CHECK_ARG(audio != nullptr && a0 != nullptr && a1 != nullptr && out != nullptr && lengths != nullptr, "null pointer");
    SDT_CHECK_ARG(n_audio > 0 && n_clips > 0 && n_clips <= 65535 && l_max > 0 && l_max <= 0x7fffffff, "bad audio / clip / length count");
    SDT_CHECK_ARG(out_elems >= n_clips * l_max, "output buffer too small");
    hipLaunchKernelGGL(clip_gather_audio_kernel, dim3((unsigned)cdiv64(l_max, kThreads), (unsigned)n_clips), dim3(kThreads), 0, (hipStream_t)stream,
                       audio, n_audio, a0, a1, l_max, out, lengths);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int64_t sdt_clip_repair_workspace_bytes(int64_t n_frames) {
    if (n_frames <= 0 || n_frames > (1 << 30)) return -1;
    return (n_frames + 1) * (int64_t)sizeof(int64_t);  // the prefix sum of repaired_per_frame
}

extern "C" int sdt_clip_repair_valid(int elem_bytes, const void* src, const void* present, int64_t n_frames, int half, double kappa,
                                     double floor_px, uint8_t* valid, uint8_t* spike, void* stream) {
    SDT_CHECK_SUPPORTED(n_frames > 0 && n_frames <= (1 << 30), "unsupported size: frame count outside [1, 2^30]");
    SDT_CHECK_SUPPORTED(half >= 0 && half <= kRepairMaxHalf, "unsupported size: despike half window outside [0, 3]");
    SDT_CHECK_ARG(elem_bytes == 4 || elem_bytes == 8, "elem_bytes must be 4 (float32 keypoints) or 8 (float64 keypoints)");
    SDT_CHECK_ARG(src != nullptr && present != nullptr && valid != nullptr && spike != nullptr, "null pointer");
    SDT_CHECK_ARG(half == 0 || (kappa > 0.0 && kappa <= 1.0e300 && floor_px >= 0.0 && floor_px <= 1.0e300), "kappa must be positive, floor_px not negative, both finite");
    const unsigned grid = (unsigned)cdiv64(n_frames * kKp, kThreads);
    hipStream_t st = (hipStream_t)stream;
    if (elem_bytes == 4)
        hipLaunchKernelGGL((clip_repair_valid_kernel<float>), dim3(grid), dim3(kThreads), 0, st, (const float*)src, (const uint8_t*)present,
                           n_frames, half, kappa, floor_px, valid, spike);
    else
        hipLaunchKernelGGL((clip_repair_valid_kernel<double>), dim3(grid), dim3(kThreads), 0, st, (const double*)src, (const uint8_t*)present,
                           n_frames, half, kappa, floor_px, valid, spike);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_clip_repair_fill(int elem_bytes, const void* src, const void* present, const uint8_t* valid, int64_t n_frames, int max_gap,
                                    void* src_r, uint8_t* present_r, uint8_t* filled, int32_t* repaired_per_frame, void* stream) {
    SDT_CHECK_SUPPORTED(n_frames > 0 && n_frames <= (1 << 30), "unsupported size: frame count outside [1, 2^30]");
    SDT_CHECK_SUPPORTED(max_gap >= 1 && max_gap <= kRepairMaxGap, "unsupported size: max_gap outside [1, 64]");
    SDT_CHECK_ARG(elem_bytes == 4 || elem_bytes == 8, "elem_bytes must be 4 (float32 keypoints) or 8 (float64 keypoints)");
    SDT_CHECK_ARG(src != nullptr && present != nullptr && valid != nullptr && src_r != nullptr && present_r != nullptr && filled != nullptr &&
                      repaired_per_frame != nullptr,
                  "null pointer");
    SDT_CHECK_ARG(src != src_r, "the stage is out of place: src_r must not be src");
    const unsigned grid = (unsigned)cdiv64(n_frames, (int64_t)kFramesPerWave * (kThreads / 64));
    hipStream_t st = (hipStream_t)stream;
    if (elem_bytes == 4)
        hipLaunchKernelGGL((clip_repair_fill_kernel<float>), dim3(grid), dim3(kThreads), 0, st, (const float*)src, (const uint8_t*)present, valid,
                           n_frames, max_gap, (float*)src_r, present_r, filled, repaired_per_frame);
    else
        hipLaunchKernelGGL((clip_repair_fill_kernel<double>), dim3(grid), dim3(kThreads), 0, st, (const double*)src, (const uint8_t*)present, valid,
                           n_frames, max_gap, (double*)src_r, present_r, filled, repaired_per_frame);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_clip_repair_clip_counts(const int32_t* repaired_per_frame, int64_t n_frames, const int32_t* starts, int64_t n_clips,
                                           int num_frames, void* workspace, int64_t workspace_bytes, int32_t* repaired_per_clip, void* stream) {
    SDT_CHECK_SUPPORTED(n_frames > 0 && n_frames <= (1 << 30), "unsupported size: frame count outside [1, 2^30]");
    SDT_CHECK_SUPPORTED(num_frames > 0 && num_frames <= (1 << 24), "unsupported size: window outside [1, 2^24] frames");
    SDT_CHECK_ARG(repaired_per_frame != nullptr && starts != nullptr && workspace != nullptr && repaired_per_clip != nullptr, "null pointer");
    SDT_CHECK_ARG(n_clips > 0 && n_clips <= n_frames && num_frames <= n_frames, "bad clip / window count");
    SDT_CHECK_ARG(workspace_bytes >= sdt_clip_repair_workspace_bytes(n_frames), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    int64_t* prefix = (int64_t*)workspace;
    hipLaunchKernelGGL(clip_repair_prefix_kernel, dim3(1), dim3(kThreads), 0, st, repaired_per_frame, n_frames, prefix);
    hipLaunchKernelGGL(clip_repair_clip_counts_kernel, dim3((unsigned)cdiv64(n_clips, kThreads)), dim3(kThreads), 0, st, prefix, n_frames, starts,
                       n_clips, num_frames, repaired_per_clip);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int64_t sdt_clip_retime_workspace_bytes(int64_t n_src, int64_t fps_num, int64_t fps_den, int n_phases, int n_taps) {
    RetimePlan rp;
    if (!retime_plan(n_src, fps_num, fps_den, &rp)) return -1;
    if ((int64_t)n_phases != rp.d / rp.g || n_taps < 2 || n_taps > kRetimeMaxTaps || (n_taps & 1)) return -1;
    return (rp.blocks_out + 2 * rp.blocks_src) * (int64_t)sizeof(int32_t);  // the blocks' integer counts
}

extern "C" int sdt_clip_retime(int elem_bytes, const void* src, const void* present, int64_t n_src, int64_t fps_num, int64_t fps_den,
                               const double* taps, int n_phases, int n_taps, double min_support, int64_t n_out, void* src_t,
                               uint8_t* present_t, uint8_t* valid_t, uint8_t* taps_used, int32_t* nearest_src, int64_t* counts,
                               void* workspace, int64_t workspace_bytes, void* stream) {
    RetimePlan rp;
    SDT_CHECK_SUPPORTED(retime_plan(n_src, fps_num, fps_den, &rp),
                        "unsupported size: source frames outside [1, 2^30], fps_num outside [1, 2^20], fps_den outside [1, 2^16], a rate outside "
                        "[1, 240] fps, more than 16384 phases or more than 2^30 output frames");
    SDT_CHECK_SUPPORTED((int64_t)n_phases == rp.d / rp.g, "unsupported size: the tap table's rows are not the rate's 15 * fps_den / gcd phases");
    SDT_CHECK_SUPPORTED(n_taps >= 2 && n_taps <= kRetimeMaxTaps && !(n_taps & 1), "unsupported size: taps per phase not even or outside [2, 32]");
    SDT_CHECK_SUPPORTED(min_support > 0.0 && min_support <= 1.0, "unsupported size: min_support outside (0, 1]");
    SDT_CHECK_ARG(elem_bytes == 4 || elem_bytes == 8, "elem_bytes must be 4 (float32 keypoints) or 8 (float64 keypoints)");
    SDT_CHECK_ARG(src != nullptr && present != nullptr && taps != nullptr && src_t != nullptr && present_t != nullptr && valid_t != nullptr &&
                      taps_used != nullptr && nearest_src != nullptr && counts != nullptr && workspace != nullptr,
                  "null pointer");
    SDT_CHECK_ARG(src != src_t, "the stage is out of place: src_t must not be src");
    SDT_CHECK_ARG(n_out == rp.n_out, "n_out is not (n_src - 1) * 15 * fps_den / fps_num + 1");
    SDT_CHECK_ARG(workspace_bytes >= (rp.blocks_out + 2 * rp.blocks_src) * (int64_t)sizeof(int32_t), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    int32_t* block_invalid = (int32_t*)workspace;
    int32_t* block_counts = block_invalid + rp.blocks_out;
    const dim3 grid_out((unsigned)rp.blocks_out), grid_src((unsigned)rp.blocks_src), block(kThreads);
    if (elem_bytes == 4) {
        hipLaunchKernelGGL((clip_retime_kernel<float>), grid_out, block, 0, st, (const float*)src, (const uint8_t*)present, n_src, fps_num, rp.d,
                           rp.g, taps, n_taps, min_support, rp.n_out, (float*)src_t, present_t, valid_t, taps_used, nearest_src, block_invalid);
        hipLaunchKernelGGL((clip_retime_source_counts_kernel<float>), grid_src, block, 0, st, (const float*)src, (const uint8_t*)present, n_src,
                           block_counts);
    } else {
        hipLaunchKernelGGL((clip_retime_kernel<double>), grid_out, block, 0, st, (const double*)src, (const uint8_t*)present, n_src, fps_num, rp.d,
                           rp.g, taps, n_taps, min_support, rp.n_out, (double*)src_t, present_t, valid_t, taps_used, nearest_src, block_invalid);
        hipLaunchKernelGGL((clip_retime_source_counts_kernel<double>), grid_src, block, 0, st, (const double*)src, (const uint8_t*)present, n_src,
                           block_counts);
    }
    hipLaunchKernelGGL(clip_retime_total_kernel, dim3(1), block, 0, st, block_invalid, rp.blocks_out, block_counts, rp.blocks_src, counts);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
