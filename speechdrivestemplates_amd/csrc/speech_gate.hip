// Audio activity gate of the clip builder (clip_builder.py, speech_gate=...; DESIGN.md section 28 is the contract): an opt-in stage that
// drops the windows of a custom speaker's video whose audio carries too little energy above the track's noise floor.  The input is the
// video's cut 16 kHz float32 track of N samples; a hop is 160 samples (10 ms), H = N / 160, the tail is ignored.  Stages:
//   energy   one wave per hop: d[n] = x[n] - (31/32) x[n-1] (x[-1] = 0; the coefficient is exact in binary, so the product is exact and the
//            difference is rounded once), e[h] = sum of d^2 over the hop.  Lane l adds i = l, l + 64, l + 128 (i < 160) in that order from
//            +0.0, then the xor butterfly 32, 16, 8, 4, 2, 1: one fixed order.  A non-finite e[h] sets a flag (integer atomic).
//   mask     the floor f = the energy of rank k in ascending order, by the radix select of radix_select.h on the uint64 images (8 passes
//            of 8 bits, 256-bin histograms with integer atomics, in LDS first); thr = max(f * M, A), the product rounded once;
//            active_raw[h] = e[h] > thr.
//   smooth   integer run-length rules: (a) an active run shorter than min_run_hops becomes inactive, then (b) an inactive run of at most
//            hang_hops with an active hop on both sides becomes active.  Each rule is one pass of three kernels: the last and the first
//            marker (rule a: an inactive hop; rule b: an active hop) of every block of 256 hops, a scan of those over the blocks, and
//            an in-block prefix maximum / suffix minimum that gives every hop the nearest marker on either side.  No serial walk.
//   windows  an int32 prefix sum of the mask; per candidate window the hops wholly inside [a0, min(a1, N)) and the active ones among them;
//            kept iff n_h > 0 and 1000 c >= min_permille n_h in int64; the kept windows compacted in ascending order by a measure pass
//            and a pack pass, as sdt_clip_windows does.
// float64 with every operation rounded on its own (exact_f64.h), no floating-point atomics, every decision after the threshold in integers:
// the same bits on every call.
#include "exact_f64.h"
#include "radix_select.h"

namespace {

using sdt_exact::add_rn;
using sdt_exact::mul_rn;
using sdt_exact::sub_rn;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kHop = 160;
constexpr double kPre = 31.0 / 32.0;
constexpr int64_t kMaxHops = (int64_t)1 << 24, kMaxSamples = kMaxHops * kHop + (kHop - 1), kMaxWindows = (int64_t)1 << 30;
constexpr int kMaxRunHops = 1024;
constexpr int kSelMaxGrid = 512, kSelPerThread = 8;

// ---- hop energies ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) speech_energy_kernel(const float* __restrict__ x, int64_t H, double* __restrict__ energy,
                                                                 int32_t* __restrict__ flag) {
    const int64_t h = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (h >= H) return;  // uniform over the wave
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int i = lane; i < kHop; i += 64) {
        const int64_t n = h * kHop + i;
        const double cur = (double)x[n], prev = n > 0 ? (double)x[n - 1] : 0.0;
        const double d = sub_rn(cur, mul_rn(kPre, prev));
        acc = add_rn(acc, mul_rn(d, d));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = add_rn(acc, __shfl_xor(acc, o, 64));
    if (lane == 0) {
        energy[h] = acc;
        if (!isfinite(acc)) atomicOr(flag, 1);
    }
}

// ---- the floor: exact order statistic ------------------------------------------------------------------------------------------------------
// state of the select, in the workspace: prefix (uint64) | remaining rank (int64) | histogram (256 uint32)
__global__ void __launch_bounds__(kThreads) speech_select_init_kernel(long long rank, unsigned long long* __restrict__ prefix,
                                                                      long long* __restrict__ remain, uint32_t* __restrict__ hist) {
    hist[threadIdx.x] = 0u;
    if (threadIdx.x == 0) {
        *prefix = 0ull;
        *remain = rank;
    }
}

__global__ void __launch_bounds__(kThreads) speech_select_hist_kernel(const double* __restrict__ energy, int64_t H, int pass,
                                                                      const unsigned long long* __restrict__ prefix,
                                                                      uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned long long p = *prefix;
    const int shift = 56 - 8 * pass;
    for (int64_t h = (int64_t)blockIdx.x * kThreads + threadIdx.x; h < H; h += (int64_t)gridDim.x * kThreads) {
        const unsigned long long key = sdt_select::order_key(energy[h]);
        if (pass == 0 || ((key ^ p) >> (shift + 8)) == 0ull) atomicAdd(&s_h[(uint32_t)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t v = s_h[threadIdx.x];
    if (v != 0u) atomicAdd(&hist[threadIdx.x], v);
}

// the byte whose cumulative count passes the remaining rank joins the prefix; the histogram is zeroed for the next pass; the last pass
// writes the value
__global__ void __launch_bounds__(kThreads) speech_select_step_kernel(int pass, unsigned long long* __restrict__ prefix,
                                                                      long long* __restrict__ remain, uint32_t* __restrict__ hist,
                                                                      double* __restrict__ stats) {
    __shared__ uint32_t s_cnt[256];
    s_cnt[threadIdx.x] = hist[threadIdx.x];
    hist[threadIdx.x] = 0u;
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long rem = *remain;
    const int digit = sdt_select::pick_digit(s_cnt, &rem);
    const unsigned long long p = *prefix | ((unsigned long long)digit << (56 - 8 * pass));
    *prefix = p;
    *remain = rem;
    if (pass == 7) stats[0] = sdt_select::order_value(p);
}

__global__ void __launch_bounds__(kThreads) speech_mask_kernel(const double* __restrict__ energy, int64_t H, double margin, double abs_floor,
                                                               double* __restrict__ stats, uint8_t* __restrict__ active) {
    const double scaled = mul_rn(stats[0], margin);
    const double thr = scaled > abs_floor ? scaled : abs_floor;
    const int64_t h = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (h == 0) stats[1] = thr;
    if (h < H) active[h] = energy[h] > thr ? 1 : 0;
}

// ---- smoothing -----------------------------------------------------------------------------------------------------------------------------
// inclusive prefix maximum over the workgroup's threads in index order; *total = the maximum of all of them.  Holds two barriers.
__device__ __forceinline__ int block_prefix_max(int v, int* wmax, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off, 64);
        if (lane >= off) v = max(v, t);
    }
    if (lane == 63) wmax[w] = v;
    __syncthreads();
    int tot = wmax[0];
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        if (i < w) v = max(v, wmax[i]);
        tot = max(tot, wmax[i]);
    }
    __syncthreads();
    *total = tot;
    return v;
}

// kFill false (rule a): the markers are the inactive hops; kFill true (rule b): the active hops
template <bool kFill>
__device__ __forceinline__ bool is_marker(const uint8_t* __restrict__ m, int64_t h, int64_t H) {
    return h >= 0 && h < H && ((m[h] != 0) == kFill);
}

// block_last[b] = the last marker among hops [256 b, 256 (b + 1)) or -1; block_first[b] = the first or H
template <bool kFill>
__global__ void __launch_bounds__(kThreads) speech_marks_kernel(const uint8_t* __restrict__ m, int64_t H, int32_t* __restrict__ block_last,
                                                                int32_t* __restrict__ block_first) {
    __shared__ int s_last[kWaves], s_first[kWaves];
    const int64_t h = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool mark = is_marker<kFill>(m, h, H);
    int last = mark ? (int)h : -1, first = mark ? (int)h : (int)H;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        last = max(last, __shfl_xor(last, o, 64));
        first = min(first, __shfl_xor(first, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        s_last[threadIdx.x >> 6] = last;
        s_first[threadIdx.x >> 6] = first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < kWaves; ++i) {
            last = max(last, s_last[i]);
            first = min(first, s_first[i]);
        }
        block_last[blockIdx.x] = last;
        block_first[blockIdx.x] = first;
    }
}

// one workgroup: carry_last[b] = the last marker in the blocks before b or -1; carry_first[b] = the first marker in the blocks after b or H
__global__ void __launch_bounds__(kThreads) speech_carry_kernel(const int32_t* __restrict__ block_last, const int32_t* __restrict__ block_first,
                                                                int nb, int H, int32_t* __restrict__ carry_last,
                                                                int32_t* __restrict__ carry_first) {
    __shared__ int wmax[kWaves];
    int carry = -1, tot;
    for (int base = 0; base < nb; base += kThreads) {
        const int b = base + threadIdx.x;
        const int incl = block_prefix_max(b < nb ? block_last[b] : -1, wmax, &tot);
        if (b + 1 < nb) carry_last[b + 1] = max(carry, incl);
        carry = max(carry, tot);
    }
    carry = -H;  // the minimum as the maximum of the negated values, over the blocks in descending order
    for (int base = 0; base < nb; base += kThreads) {
        const int r = nb - 1 - (base + threadIdx.x);
        const int incl = block_prefix_max(r >= 0 ? -block_first[r] : -H, wmax, &tot);
        if (r >= 1) carry_first[r - 1] = -max(carry, incl);
        carry = max(carry, tot);
    }
    if (threadIdx.x == 0) {
        carry_last[0] = -1;
        carry_first[nb - 1] = H;
    }
}

// prev = the nearest marker at or before h (-1: none), next = the nearest at or after h (H: none), then the rule
template <bool kFill>
__global__ void __launch_bounds__(kThreads) speech_apply_kernel(const uint8_t* __restrict__ m, int64_t H, int limit,
                                                                const int32_t* __restrict__ carry_last, const int32_t* __restrict__ carry_first,
                                                                uint8_t* __restrict__ out) {
    __shared__ int wmax[kWaves];
    __shared__ int s_next[kThreads];
    const int64_t base = (int64_t)blockIdx.x * kThreads, h = base + threadIdx.x, hr = base + (kThreads - 1 - threadIdx.x);
    int tot;
    const int prev = max(carry_last[blockIdx.x], block_prefix_max(is_marker<kFill>(m, h, H) ? (int)h : -1, wmax, &tot));
    const int neg = block_prefix_max(is_marker<kFill>(m, hr, H) ? -(int)hr : -(int)H, wmax, &tot);  // hops in descending order
    s_next[kThreads - 1 - threadIdx.x] = min(carry_first[blockIdx.x], -neg);
    __syncthreads();
    if (h >= H) return;
    const int next = s_next[threadIdx.x];
    const bool on = m[h] != 0;
    if (!kFill)
        out[h] = (on && next - prev - 1 >= limit) ? 1 : 0;  // an active hop's run lies between the inactive hops prev and next
    else
        out[h] = (on || (prev >= 0 && next < (int)H && next - prev - 1 <= limit)) ? 1 : 0;  // a gap between the active hops prev and next
}

// ---- windows -------------------------------------------------------------------------------------------------------------------------------
// one workgroup walks the hops in tiles of kThreads: prefix[h] = active hops before h, prefix[H] = all of them
__global__ void __launch_bounds__(kThreads) speech_prefix_kernel(const uint8_t* __restrict__ active, int64_t H, int32_t* __restrict__ prefix) {
    __shared__ int wsum[kWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carry = 0;
    for (int64_t base = 0; base < H; base += kThreads) {
        const int64_t h = base + threadIdx.x;
        const bool v = h < H && active[h] != 0;
        const unsigned long long mask = __ballot(v);
        if (lane == 0) wsum[w] = __popcll(mask);
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int i = 0; i < kWaves; ++i) {
            if (i < w) woff += wsum[i];
            tot += wsum[i];
        }
        if (h < H) prefix[h] = carry + woff + __popcll(mask & ((1ull << lane) - 1ull));
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) prefix[H] = carry;
}

// the hops wholly inside [a0, min(a1, N)): 160 h >= a0 and 160 (h + 1) <= a1
__device__ __forceinline__ bool window_kept(const int32_t* __restrict__ prefix, int64_t H, int64_t N, const int64_t* __restrict__ a0,
                                            const int64_t* __restrict__ a1, int64_t i, int64_t n_win, int permille, int* c_out, int* nh_out) {
    if (i >= n_win) return false;
    const int64_t b0 = a0[i] < 0 ? 0 : a0[i], b1 = a1[i] < N ? a1[i] : N;
    const int64_t h0 = (b0 + kHop - 1) / kHop;
    int64_t h1 = b1 < 0 ? 0 : b1 / kHop;
    if (h1 > H) h1 = H;
    const int nh = h1 > h0 ? (int)(h1 - h0) : 0;
    const int c = nh > 0 ? prefix[h1] - prefix[h0] : 0;
    *c_out = c;
    *nh_out = nh;
    return nh > 0 && (int64_t)1000 * c >= (int64_t)permille * nh;
}

// measure (kPack false): counts_all[i] = (c, n_h), block_counts[b] = kept windows among candidates [b*kThreads, (b+1)*kThreads)
// pack (kPack true): the kept windows' start, candidate index and counts in ascending order at the block's offset; the last block writes
// the total
template <bool kPack>
__global__ void __launch_bounds__(kThreads) speech_windows_kernel(const int32_t* __restrict__ prefix, int64_t H, int64_t N,
                                                                  const int32_t* __restrict__ starts, const int64_t* __restrict__ a0,
                                                                  const int64_t* __restrict__ a1, int64_t n_win, int permille,
                                                                  int32_t* __restrict__ block_counts, int32_t* __restrict__ counts_all,
                                                                  int32_t* __restrict__ starts_kept, int32_t* __restrict__ index_kept,
                                                                  int32_t* __restrict__ counts_kept, int32_t* __restrict__ n_kept) {
    __shared__ int wsum[kWaves];
    __shared__ int s_off;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int c = 0, nh = 0;
    const bool v = window_kept(prefix, H, N, a0, a1, i, n_win, permille, &c, &nh);
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
    for (int k = 0; k < kWaves; ++k) {
        if (k < w) woff += wsum[k];
        tot += wsum[k];
    }
    if (!kPack) {
        if (i < n_win) {
            counts_all[2 * i] = c;
            counts_all[2 * i + 1] = nh;
        }
        if (threadIdx.x == 0) block_counts[blockIdx.x] = tot;
        return;
    }
    if (v) {
        const int64_t at = s_off + woff + __popcll(mask & ((1ull << lane) - 1ull));
        starts_kept[at] = starts[i];
        index_kept[at] = (int32_t)i;
        counts_kept[2 * at] = c;
        counts_kept[2 * at + 1] = nh;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_kept = s_off + tot;
}

inline bool sizes_ok(int64_t n_samples, int64_t n_windows) {
    return n_samples >= 0 && n_samples <= kMaxSamples && n_windows >= 0 && n_windows <= kMaxWindows;
}
inline int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }
inline int64_t select_ws_bytes() { return 8 + 8 + 256 * 4; }
// four int32 per block of hops (block_last, block_first, carry_last, carry_first) and the mask between the two rules
inline int64_t smooth_ws_bytes(int64_t H) { return align16(cdiv64(H, kThreads) * 4 * (int64_t)sizeof(int32_t)) + align16(H); }
inline int64_t windows_ws_bytes(int64_t n_windows) { return cdiv64(n_windows, kThreads) * (int64_t)sizeof(int32_t); }

}  // namespace

extern "C" int64_t sdt_clip_speech_workspace_bytes(int64_t n_samples, int64_t n_windows) {
    if (!sizes_ok(n_samples, n_windows)) return -1;
    return std::max<int64_t>(16, std::max(select_ws_bytes(), std::max(smooth_ws_bytes(n_samples / kHop), windows_ws_bytes(n_windows))));
}

extern "C" int sdt_clip_speech_energy(const float* audio, int64_t n_samples, double* energy, int32_t* flag, void* stream) {
    SDT_CHECK_SUPPORTED(sizes_ok(n_samples, 0), "n_samples must lie in [0, 160 * 2^24 + 159]");
    const int64_t H = n_samples / kHop;
    SDT_CHECK_ARG(flag != nullptr && (H == 0 || (audio != nullptr && energy != nullptr)), "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(flag, 0, sizeof(int32_t), st) != hipSuccess) return SDT_ERR_LAUNCH;
    if (H == 0) return SDT_OK;
    hipLaunchKernelGGL(speech_energy_kernel, dim3((unsigned)cdiv64(H, kWaves)), dim3(kThreads), 0, st, audio, H, energy, flag);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_clip_speech_mask(const double* energy, int64_t n_hops, int floor_pct, double margin, double abs_floor, uint8_t* active_raw,
                                    double* stats, void* workspace, int64_t workspace_bytes, void* stream) {
    SDT_CHECK_SUPPORTED(n_hops >= 0 && n_hops <= kMaxHops, "n_hops must lie in [0, 2^24]");
    SDT_CHECK_SUPPORTED(floor_pct >= 0 && floor_pct <= 50, "floor_pct must lie in [0, 50]");
    SDT_CHECK_ARG(margin == margin && abs_floor == abs_floor, "margin and abs_floor must not be NaN");
    SDT_CHECK_ARG(stats != nullptr && workspace != nullptr && (n_hops == 0 || (energy != nullptr && active_raw != nullptr)), "null pointer");
    SDT_CHECK_ARG(workspace_bytes >= select_ws_bytes(), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (n_hops == 0) {  // no hop, no floor: both statistics are 0
        if (hipMemsetAsync(stats, 0, 2 * sizeof(double), st) != hipSuccess) return SDT_ERR_LAUNCH;
        return SDT_OK;
    }
    unsigned long long* prefix = (unsigned long long*)workspace;
    long long* remain = (long long*)(prefix + 1);
    uint32_t* hist = (uint32_t*)(remain + 1);
    const long long rank = ((long long)floor_pct * (n_hops - 1)) / 100;
    const unsigned grid = (unsigned)std::min<int64_t>(kSelMaxGrid, cdiv64(n_hops, (int64_t)kThreads * kSelPerThread));
    hipLaunchKernelGGL(speech_select_init_kernel, dim3(1), dim3(kThreads), 0, st, rank, prefix, remain, hist);
    for (int pass = 0; pass < 8; ++pass) {
        hipLaunchKernelGGL(speech_select_hist_kernel, dim3(grid), dim3(kThreads), 0, st, energy, n_hops, pass, prefix, hist);
        hipLaunchKernelGGL(speech_select_step_kernel, dim3(1), dim3(kThreads), 0, st, pass, prefix, remain, hist, stats);
    }
    hipLaunchKernelGGL(speech_mask_kernel, dim3((unsigned)cdiv64(n_hops, kThreads)), dim3(kThreads), 0, st, energy, n_hops, margin, abs_floor,
                       stats, active_raw);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_clip_speech_smooth(const uint8_t* active_raw, int64_t n_hops, int min_run_hops, int hang_hops, uint8_t* active,
                                      void* workspace, int64_t workspace_bytes, void* stream) {
    SDT_CHECK_SUPPORTED(n_hops >= 0 && n_hops <= kMaxHops, "n_hops must lie in [0, 2^24]");
    SDT_CHECK_SUPPORTED(min_run_hops >= 0 && min_run_hops <= kMaxRunHops && hang_hops >= 0 && hang_hops <= kMaxRunHops,
                        "min_run_hops and hang_hops must lie in [0, 1024]");
    if (n_hops == 0) return SDT_OK;
    SDT_CHECK_ARG(active_raw != nullptr && active != nullptr && workspace != nullptr, "null pointer");
    SDT_CHECK_ARG(active_raw != active, "active must not alias active_raw");
    SDT_CHECK_ARG(workspace_bytes >= smooth_ws_bytes(n_hops), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)cdiv64(n_hops, kThreads), H = (int)n_hops;
    int32_t* block_last = (int32_t*)workspace;
    int32_t *block_first = block_last + nb, *carry_last = block_first + nb, *carry_first = carry_last + nb;
    uint8_t* opened = (uint8_t*)workspace + align16((int64_t)nb * 4 * (int64_t)sizeof(int32_t));
    const dim3 grid((unsigned)nb), block(kThreads);
    hipLaunchKernelGGL((speech_marks_kernel<false>), grid, block, 0, st, active_raw, n_hops, block_last, block_first);
    hipLaunchKernelGGL(speech_carry_kernel, dim3(1), block, 0, st, block_last, block_first, nb, H, carry_last, carry_first);
    hipLaunchKernelGGL((speech_apply_kernel<false>), grid, block, 0, st, active_raw, n_hops, min_run_hops, carry_last, carry_first, opened);
    hipLaunchKernelGGL((speech_marks_kernel<true>), grid, block, 0, st, opened, n_hops, block_last, block_first);
    hipLaunchKernelGGL(speech_carry_kernel, dim3(1), block, 0, st, block_last, block_first, nb, H, carry_last, carry_first);
    hipLaunchKernelGGL((speech_apply_kernel<true>), grid, block, 0, st, opened, n_hops, hang_hops, carry_last, carry_first, active);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_clip_speech_windows(const uint8_t* active, int64_t n_hops, int64_t n_samples, const int32_t* starts, const int64_t* a0,
                                       const int64_t* a1, int64_t n_windows, int min_permille, int32_t* prefix, int32_t* counts_all,
                                       int32_t* starts_kept, int32_t* index_kept, int32_t* counts_kept, int32_t* n_kept, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
    SDT_CHECK_SUPPORTED(sizes_ok(n_samples, n_windows), "n_samples must lie in [0, 160 * 2^24 + 159] and n_windows in [0, 2^30]");
    SDT_CHECK_ARG(n_hops == n_samples / kHop, "n_hops must be n_samples / 160");
    SDT_CHECK_SUPPORTED(min_permille >= 1 && min_permille <= 1000, "min_permille must lie in [1, 1000]");
    SDT_CHECK_ARG(prefix != nullptr && n_kept != nullptr && (n_hops == 0 || active != nullptr), "null pointer");
    SDT_CHECK_ARG(n_windows == 0 || (starts != nullptr && a0 != nullptr && a1 != nullptr && counts_all != nullptr && starts_kept != nullptr &&
                                     index_kept != nullptr && counts_kept != nullptr && workspace != nullptr),
                  "null pointer");
    SDT_CHECK_ARG(workspace_bytes >= windows_ws_bytes(n_windows), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(kThreads);
    hipLaunchKernelGGL(speech_prefix_kernel, dim3(1), block, 0, st, active, n_hops, prefix);
    if (n_windows == 0) {  // the prefix sum all the same; no window, nothing to count or pack
        if (hipMemsetAsync(n_kept, 0, sizeof(int32_t), st) != hipSuccess) return SDT_ERR_LAUNCH;
        SDT_LAUNCH_CHECK();
        return SDT_OK;
    }
    int32_t* block_counts = (int32_t*)workspace;
    const dim3 grid((unsigned)cdiv64(n_windows, kThreads));
    hipLaunchKernelGGL((speech_windows_kernel<false>), grid, block, 0, st, prefix, n_hops, n_samples, starts, a0, a1, n_windows, min_permille,
                       block_counts, counts_all, starts_kept, index_kept, counts_kept, n_kept);
    hipLaunchKernelGGL((speech_windows_kernel<true>), grid, block, 0, st, prefix, n_hops, n_samples, starts, a0, a1, n_windows, min_permille,
                       block_counts, counts_all, starts_kept, index_kept, counts_kept, n_kept);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
