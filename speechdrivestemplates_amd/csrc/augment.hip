// Audio augmentation inside the train step (TRAIN.AUGMENT; include/sdt_hip.h states the layouts, DESIGN.md section 25 the contract; augment.
// philox4x32 / sumsq_model / clip_params_model / audio_model / mel_mask_model in Python are the same operations in the same order): a per-clip
// gain, white noise at a per-clip SNR, a shift of whole samples, a sign flip, and zeroed bands and spans of the power mel.  Everything random
// is a word of Philox4x32-10 with the key (seed low, seed high) and the counter (block, purpose, clip index low, step low), so a clip's
// augmentation depends on (seed, step, clip) only.  No transcendental function runs here: the gain and SNR factors come from 256-entry tables.
//
// Orders of summation, all fixed:
//   sum of squares   chunk c covers samples [1024 c, 1024 c + 1024); thread t of 256 adds the squares of samples 1024 c + t + 256 k for
//                    k = 0, 1, 2, 3 in that order from +0.0 (+0.0 at or past L); each wave runs the xor butterfly v += shfl_xor(v, o) for
//                    o = 32, 16, 8, 4, 2, 1; then ((wave 0 + wave 1) + wave 2) + wave 3 is the chunk's partial;
//   over the chunks  lane l of one wave adds the partials l, l + 64, l + 128, .. in that order from +0.0, then the same butterfly.
// Every float64 multiply, add and divide goes through sdt_exact::*_rn (no FMA); every square is exact in float64.  No atomics.
#include "exact_lanes.h"
#include "philox.h"

using namespace sdt_exact;

namespace {

constexpr int kChunk = 1024;               // samples per chunk of the sum of squares
constexpr int kCols = SDT_AUGMENT_REC_COLS;
constexpr int kMaxMasks = 4;
constexpr int64_t kMaxL = (int64_t)1 << 24;
constexpr double kNoiseScale = 0x1.bb67ae86627e7p-16;  // 1 / sqrt(4 (65536^2 - 1) / 12): unit variance of the centred sum of four 16-bit halves

using sdt_philox::Key;  // Philox4x32-10 lives in philox.h, shared with pose_augment.hip
using sdt_philox::Words;
using sdt_philox::philox4x32;

// one workgroup of 256 threads per (chunk, clip): the chunk's partial sum of squares
__global__ __launch_bounds__(256) void aug_sumsq_chunk_kernel(const float* __restrict__ x, int L, int n_chunks, double* __restrict__ partials) {
    __shared__ double sred[4];
    const int t = threadIdx.x, c = blockIdx.x, b = blockIdx.y;
    const float* xr = x + (size_t)b * L;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int n = c * kChunk + t + 256 * k;
        const double v = n < L ? (double)xr[n] : 0.0;
        s = add_rn(s, mul_rn(v, v));
    }
    s = butterfly_sum(s);
    if ((t & 63) == 0) sred[t >> 6] = s;
    __syncthreads();
    if (t == 0) partials[(size_t)b * n_chunks + c] = add_rn(add_rn(add_rn(sred[0], sred[1]), sred[2]), sred[3]);
}

// one wave per clip: the chunk partials in lane-strided order, then the butterfly
__global__ __launch_bounds__(64) void aug_sumsq_clip_kernel(const double* __restrict__ partials, int n_chunks, double* __restrict__ ss) {
    const int lane = threadIdx.x, b = blockIdx.x;
    double s = 0.0;
    for (int j = lane; j < n_chunks; j += 64) s = add_rn(s, partials[(size_t)b * n_chunks + j]);
    s = butterfly_sum(s);
    if (lane == 0) ss[b] = s;
}

struct ClipOpts {
    Key key;
    uint32_t S;        // largest shift in samples
    uint32_t prob24;   // the noise is on iff (w3 >> 8) < prob24
    int polarity;      // the sign flip is drawn at all
};

// one thread per clip: block 0 of purpose 0 -> the clip's parameters, sigma, the record's words 0 .. 7 (8 .. 31 zero)
__global__ __launch_bounds__(64) void aug_clip_params_kernel(const int64_t* __restrict__ clip_index, const int64_t* __restrict__ step,
                                                             const double* __restrict__ ss, const double* __restrict__ snr_tab, int B, int L,
                                                             ClipOpts o, int64_t* __restrict__ rec) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const Words p = philox4x32(0u, 0u, (uint32_t)clip_index[b], (uint32_t)step[0], o.key);
    const uint32_t ig = p.w[0] >> 24, is = p.w[1] >> 24;
    const int64_t s = (int64_t)(p.w[2] % (2u * o.S + 1u)) - (int64_t)o.S;
    const int noise = (p.w[3] >> 8) < o.prob24 ? 1 : 0;
    const int flip = o.polarity ? (int)(p.w[3] & 1u) : 0;
    const double sum = ss[b];
    const double sigma = noise ? mul_rn(sqrt(div_rn(sum, (double)L)), snr_tab[is]) : 0.0;
    int64_t* r = rec + (size_t)b * kCols;
    r[0] = ig;
    r[1] = is;
    r[2] = s;
    r[3] = flip;
    r[4] = noise;
    r[5] = __double_as_longlong(sigma);
    r[6] = __double_as_longlong(sum);
    r[7] = finite_d(sum) ? 0 : 1;
#pragma unroll
    for (int c = 8; c < kCols; ++c) r[c] = 0;
}

// y[n] = float32(g * (x[n - s] + sigma z[n])) of one clip per blockIdx.y.  Thread 0 of a row writes the elements before the first 16-byte
// boundary of the output row one by one; thread i >= 1 writes the four elements from head + 4 (i - 1) with one 16-byte store, or the row's
// last one to three elements one by one.  Every read is x[b][m] with 0 <= m < L.
__global__ __launch_bounds__(256) void aug_audio_kernel(const float* __restrict__ x, int L, const int64_t* __restrict__ clip_index,
                                                        const int64_t* __restrict__ step, const int64_t* __restrict__ rec,
                                                        const float* __restrict__ gain_tab, Key key, float* __restrict__ y) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int64_t* r = rec + (size_t)b * kCols;
    const float* xr = x + (size_t)b * L;
    float* yr = y + (size_t)b * L;
    int head = (int)(((16u - (unsigned)((uintptr_t)yr & 15u)) & 15u) >> 2);
    head = head < L ? head : L;
    const int n0 = i == 0 ? 0 : head + 4 * (i - 1);
    if (n0 >= L) return;
    const int cnt = i == 0 ? head : (L - n0 < 4 ? L - n0 : 4);
    const int s = (int)r[2];
    const bool noise = r[4] != 0;
    const double sigma = __longlong_as_double(r[5]);
    const float gf = gain_tab[r[0]];
    const double g = (double)(r[3] ? -gf : gf);
    const uint32_t c2 = (uint32_t)clip_index[b], c3 = (uint32_t)step[0];
    float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t cur = 0xffffffffu;  // (no sample has this block: n >> 1 < 2^23)
    Words w = {{0u, 0u, 0u, 0u}};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < cnt) {
            const int n = n0 + j, m = n - s;
            double v = (double)(m >= 0 && m < L ? xr[m] : 0.0f);
            if (noise) {
                const uint32_t blk = (uint32_t)n >> 1;
                if (blk != cur) {
                    w = philox4x32(blk, 1u, c2, c3, key);
                    cur = blk;
                }
                const uint32_t a = (n & 1) ? w.w[2] : w.w[0], c = (n & 1) ? w.w[3] : w.w[1];
                const int h = (int)((a & 0xffffu) + (a >> 16) + (c & 0xffffu) + (c >> 16)) - 131070;
                v = add_rn(v, mul_rn(sigma, mul_rn((double)h, kNoiseScale)));
            }
            out[j] = (float)mul_rn(g, v);
        }
    }
    if (i != 0 && cnt == 4) {
        *reinterpret_cast<f32x4*>(yr + n0) = f32x4{out[0], out[1], out[2], out[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) yr[n0 + j] = out[j];
    }
}

struct MaskOpts {
    Key key;
    int nf, wf, nt, wt;
};

// one wave per clip: thread t < 8 draws mask t & 3 of the frequency (t < 4) or the time (t >= 4) dimension -> the record's words 8 .. 25
__global__ __launch_bounds__(64) void aug_mel_rects_kernel(const int64_t* __restrict__ clip_index, const int64_t* __restrict__ step, int M, int F,
                                                           MaskOpts o, int64_t* __restrict__ rec) {
    const int t = threadIdx.x, b = blockIdx.x;
    int64_t* r = rec + (size_t)b * kCols;
    if (t < 2 * kMaxMasks) {
        const int i = t & 3, time = t >> 2;
        const int n = time ? o.nt : o.nf, wmax = time ? o.wt : o.wf, D = time ? F : M;
        int64_t start = 0, width = 0;
        if (i < n) {
            const Words p = philox4x32((uint32_t)((time ? 5 : 1) + i), 0u, (uint32_t)clip_index[b], (uint32_t)step[0], o.key);
            const uint32_t wd = p.w[0] % (uint32_t)(wmax + 1);
            width = wd < (uint32_t)D ? wd : D;
            start = p.w[1] % (uint32_t)(D - (int)width + 1);
        }
        r[8 + 2 * t] = start;
        r[9 + 2 * t] = width;
    } else if (t == 8) {
        r[24] = o.nf;
    } else if (t == 9) {
        r[25] = o.nt;
    }
}

// one thread per element of the clip's (M, F) mel: +0.0 inside a rectangle, untouched (not even read) outside
__global__ __launch_bounds__(256) void aug_mel_mask_kernel(const int64_t* __restrict__ rec, int M, int F, float* __restrict__ mel) {
    const int e = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (e >= M * F) return;
    const int64_t* r = rec + (size_t)b * kCols;
    const int m = e / F, f = e - m * F;
    bool hit = false;
#pragma unroll
    for (int i = 0; i < kMaxMasks; ++i) {
        const int fs = (int)r[8 + 2 * i], fw = (int)r[9 + 2 * i], ts = (int)r[16 + 2 * i], tw = (int)r[17 + 2 * i];
        hit = hit || (m >= fs && m < fs + fw) || (f >= ts && f < ts + tw);
    }
    if (hit) mel[(size_t)b * M * F + e] = 0.0f;
}

}  // namespace

extern "C" int64_t sdt_augment_workspace_bytes(int B, int64_t L) {
    if (B < 1 || B > 65535 || L < 1 || L > kMaxL) return -1;
    return (int64_t)B * cdiv64(L, kChunk) * 8;
}

extern "C" int sdt_augment_sumsq_f64(const float* audio, int B, int64_t L, void* work, double* ss, void* stream) {
    SDT_CHECK_ARG(audio && work && ss, "null pointer");
    SDT_CHECK_ARG(B >= 1 && B <= 65535, "B outside [1, 65535]");
    SDT_CHECK_ARG(L >= 1 && L <= kMaxL, "L outside [1, 2^24]");
    const int n_chunks = (int)cdiv64(L, kChunk);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(aug_sumsq_chunk_kernel, dim3((unsigned)n_chunks, (unsigned)B), dim3(256), 0, s, audio, (int)L, n_chunks, (double*)work);
    hipLaunchKernelGGL(aug_sumsq_clip_kernel, dim3((unsigned)B), dim3(64), 0, s, (const double*)work, n_chunks, ss);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_augment_audio_f32(const float* audio, int B, int64_t L, const int64_t* clip_index, const int64_t* step, const double* ss,
                                     uint64_t seed, int64_t max_shift, int64_t noise_prob24, int polarity, const float* gain_table,
                                     const double* snr_table, void* rec, float* out, void* stream) {
    SDT_CHECK_ARG(audio && clip_index && step && ss && gain_table && snr_table && rec && out, "null pointer");
    SDT_CHECK_ARG(audio != out, "the audio pass never runs in place");
    SDT_CHECK_ARG(B >= 1 && B <= 65535, "B outside [1, 65535]");
    SDT_CHECK_ARG(L >= 1 && L <= kMaxL, "L outside [1, 2^24]");
    SDT_CHECK_ARG(max_shift >= 0 && max_shift <= kMaxL, "largest shift outside [0, 2^24]");
    SDT_CHECK_ARG(noise_prob24 >= 0 && noise_prob24 <= (1 << 24), "noise probability outside [0, 2^24]");
    SDT_CHECK_ARG(polarity == 0 || polarity == 1, "polarity is 0 or 1");
    const Key key = {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)};
    const ClipOpts o = {key, (uint32_t)max_shift, (uint32_t)noise_prob24, polarity};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(aug_clip_params_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, s, clip_index, step, ss, snr_table, B, (int)L, o,
                       (int64_t*)rec);
    const unsigned blocks = (unsigned)cdiv64(1 + cdiv64(L, 4), 256);
    hipLaunchKernelGGL(aug_audio_kernel, dim3(blocks, (unsigned)B), dim3(256), 0, s, audio, (int)L, clip_index, step, (const int64_t*)rec,
                       gain_table, key, out);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_augment_mel_mask_f32(float* mel, int B, int M, int F, const int64_t* clip_index, const int64_t* step, uint64_t seed, int nf,
                                        int wf, int nt, int wt, void* rec, void* stream) {
    SDT_CHECK_ARG(mel && clip_index && step && rec, "null pointer");
    SDT_CHECK_ARG(B >= 1 && B <= 65535, "B outside [1, 65535]");
    SDT_CHECK_ARG(M >= 1 && M <= 1024, "mel bins outside [1, 1024]");
    SDT_CHECK_ARG(F >= 1 && F <= (1 << 20), "mel columns outside [1, 2^20]");
    SDT_CHECK_ARG(nf >= 0 && nf <= kMaxMasks && nt >= 0 && nt <= kMaxMasks, "number of masks outside [0, 4]");
    SDT_CHECK_ARG(wf >= 0 && wf <= (1 << 20) && wt >= 0 && wt <= (1 << 20), "mask width outside [0, 2^20]");
    const MaskOpts o = {{(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)}, nf, wf, nt, wt};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(aug_mel_rects_kernel, dim3((unsigned)B), dim3(64), 0, s, clip_index, step, M, F, o, (int64_t*)rec);
    if (nf > 0 || nt > 0)
        hipLaunchKernelGGL(aug_mel_mask_kernel, dim3((unsigned)cdiv64((int64_t)M * F, 256), (unsigned)B), dim3(256), 0, s, (const int64_t*)rec, M, F,
                           mel);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
