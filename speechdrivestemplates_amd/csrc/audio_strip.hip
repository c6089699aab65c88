// The audio band under the rendered pictures (SYS.AUDIO_STRIP; include/sdt_hip.h states the layouts, DESIGN.md section 35 the contract;
// audio_strip.envelope_model / raster_model / compose_model in Python are the same operations in the same order).  Three stages:
//   envelope   per column of a host-built table of column start samples the min and max of the finite samples and a flag, and for the
//              recording the peak max |x| over finite samples and the number of non-finite samples;
//   raster     the band image (S, Nc, 3) once per piece: waveform lane, three mark lanes, mel lane;
//   compose    every output image in one pass: the frame's rows copied, the band's window below them, a playhead over the band.
// Every decision is integer arithmetic, a comparison, or one IEEE operation rounded on its own (csrc/exact_f64.h), so the models reproduce
// every byte.  Minima and maxima are taken on an integer order key (-0 below +0), so no result depends on the order of a reduction; a
// non-finite sample is SELECTED away, never compared.  The only atomics are integer ones (a max of bit patterns and a count).
#include <string.h>

#include "exact_f64.h"

using namespace sdt_exact;

namespace {

constexpr int kMarkLanes = SDT_STRIP_MARK_LANES, kMarkRows = SDT_STRIP_MARK_ROWS;
constexpr int kTickW = SDT_STRIP_TICK_WIDTH, kPlayW = SDT_STRIP_PLAYHEAD_WIDTH;
constexpr int kHop = 160, kTickNum = 16000, kTickDen = 300;  // tick k of 1/300 s is at sample k * 16000 // 300
constexpr int kFactors = 255;
constexpr int kRowsPerBlock = 8;  // compose: output rows of one workgroup

struct Colours {  // BGR each
    uint8_t background[3], wave[3], warning[3], mark[kMarkLanes][3];
};
struct Ticks {
    const int32_t* t[kMarkLanes];
    int32_t n[kMarkLanes];
};

__device__ __forceinline__ bool finite_bits(uint32_t u) { return (u & 0x7f800000u) != 0x7f800000u; }
// ascending in the value, -0 below +0
__device__ __forceinline__ uint32_t order_key(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t key_bits(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }

__device__ __forceinline__ uint32_t wave_min_u(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// ---- envelope --------------------------------------------------------------------------------------------------------------------------------
// the recording: stats[0] = bits of max |x| over finite samples (0 without one), stats[1] = number of non-finite samples; both zero on entry
__global__ __launch_bounds__(256) void strip_peak_kernel(const uint32_t* __restrict__ audio, int64_t L, unsigned long long* __restrict__ stats) {
    uint32_t peak = 0, bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += (int64_t)gridDim.x * 256) {
        const uint32_t u = audio[i];
        const bool fin = finite_bits(u);
        const uint32_t a = u & 0x7fffffffu;
        peak = fin && a > peak ? a : peak;
        bad += fin ? 0u : 1u;
    }
    peak = wave_max_u(peak);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
    if ((threadIdx.x & 63) == 0) {
        if (peak) atomicMax(&stats[0], (unsigned long long)peak);
        if (bad) atomicAdd(&stats[1], (unsigned long long)bad);
    }
}

// one wave per column c: samples [max(bounds[c], 0), min(bounds[c + 1], L))
__global__ __launch_bounds__(256) void strip_envelope_kernel(const uint32_t* __restrict__ audio, int64_t L, const int64_t* __restrict__ bounds,
                                                             int Nc, uint32_t* __restrict__ env, int32_t* __restrict__ flags) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= Nc) return;  // (wave-uniform)
    int64_t a = bounds[c], b = bounds[c + 1];
    a = a < 0 ? 0 : a;
    b = b > L ? L : b;
    uint32_t kmin = 0xffffffffu, kmax = 0u, bad = 0u;
    for (int64_t i = a + lane; i < b; i += 64) {
        const uint32_t u = audio[i];
        const bool fin = finite_bits(u);
        const uint32_t k = order_key(u);
        kmin = fin && k < kmin ? k : kmin;
        kmax = fin && k > kmax ? k : kmax;
        bad |= fin ? 0u : 1u;
    }
    kmin = wave_min_u(kmin);
    kmax = wave_max_u(kmax);
    bad = wave_max_u(bad);
    if (lane == 0) {
        const bool any = kmax != 0u;  // (the key of a finite value is never 0: that is the key of a NaN with every bit set)
        env[2 * (size_t)c] = any ? key_bits(kmin) : 0u;
        env[2 * (size_t)c + 1] = any ? key_bits(kmax) : 0u;
        flags[c] = a >= b ? SDT_STRIP_EMPTY : (bad ? SDT_STRIP_NONFINITE : SDT_STRIP_OK);
    }
}

// ---- raster ----------------------------------------------------------------------------------------------------------------------------------
// one workgroup: ref[0] = the largest finite mel power, at least +0
__global__ __launch_bounds__(1024) void strip_mel_ref_kernel(const uint32_t* __restrict__ mel, int64_t count, uint32_t* __restrict__ ref) {
    __shared__ uint32_t red[16];
    uint32_t best = 0;  // bits of +0; a finite power > 0 has larger bits, a negative one is never taken
    for (int64_t i = threadIdx.x; i < count; i += 1024) {
        const uint32_t u = mel[i];
        best = finite_bits(u) && !(u & 0x80000000u) && u > best ? u : best;
    }
    best = wave_max_u(best);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) best = red[w] > best ? red[w] : best;
        ref[0] = best;
    }
}

__device__ __forceinline__ int wave_row(double x, double g, int Sw) {
    double t = sub_rn(1.0, mul_rn(x, g));
    t = add_rn(div_rn(mul_rn(t, (double)(Sw - 1)), 2.0), 0.5);
    t = floor(t);
    t = t < 0.0 ? 0.0 : t;
    t = t > (double)(Sw - 1) ? (double)(Sw - 1) : t;
    return (int)t;
}

__device__ __forceinline__ void put(uint8_t* __restrict__ band, int y, int Nc, int c, const uint8_t* bgr) {
    uint8_t* p = band + ((size_t)y * Nc + c) * 3;
    p[0] = bgr[0];
    p[1] = bgr[1];
    p[2] = bgr[2];
}

// one thread per column, rows top to bottom: neighbouring lanes write neighbouring pixels of a row
__global__ __launch_bounds__(256) void strip_raster_kernel(const float* __restrict__ env, const int32_t* __restrict__ flags,
                                                           const unsigned long long* __restrict__ stats, const int64_t* __restrict__ bounds,
                                                           int Nc, const float* __restrict__ mel, int n_mels, int64_t F,
                                                           const uint32_t* __restrict__ ref_bits, const uint8_t* __restrict__ colormap,
                                                           const float* __restrict__ factors, Ticks ticks, Colours col, int S,
                                                           uint8_t* __restrict__ band) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= Nc) return;
    const int Sw = 3 * S / 8, Sm = S - Sw - kMarkLanes * kMarkRows;
    const int flag = flags[c];
    // waveform lane
    int r0 = 0, r1 = -1;  // the bar's rows [r0, r1]
    if (flag == SDT_STRIP_OK) {
        const double peak = (double)__uint_as_float((uint32_t)stats[0]);
        const double g = div_rn(1.0, peak > 0x1p-15 ? peak : 0x1p-15);
        r0 = wave_row((double)env[2 * (size_t)c + 1], g, Sw);
        r1 = wave_row((double)env[2 * (size_t)c], g, Sw);
    }
    for (int y = 0; y < Sw; ++y)
        put(band, y, Nc, c, flag == SDT_STRIP_NONFINITE ? col.warning : (y >= r0 && y <= r1 ? col.wave : col.background));
    // mark lanes: a tick is drawn in the column that holds its sample and the kTickW - 1 columns after it
    const int64_t lo = bounds[c - (kTickW - 1) > 0 ? c - (kTickW - 1) : 0], hi = bounds[c + 1];
#pragma unroll
    for (int q = 0; q < kMarkLanes; ++q) {
        bool hit = false;
        for (int i = 0; i < ticks.n[q]; ++i) {
            const int32_t k = ticks.t[q][i];
            const int64_t s = (int64_t)k * kTickNum / kTickDen;
            hit |= k >= 0 && s >= lo && s < hi;
        }
        for (int y = 0; y < kMarkRows; ++y) put(band, Sw + q * kMarkRows + y, Nc, c, hit ? col.mark[q] : col.background);
    }
    // mel lane
    int64_t mid = (bounds[c] + bounds[c + 1]) >> 1;  // (floor, also of a negative sum)
    mid = mid < 0 ? 0 : mid;
    int64_t j = mid / kHop;
    j = j > F - 1 ? F - 1 : j;
    const float ref = __uint_as_float(ref_bits[0]);
    const int y0 = Sw + kMarkLanes * kMarkRows;
    for (int y = 0; y < Sm; ++y) {
        if (flag == SDT_STRIP_EMPTY) {
            put(band, y0 + y, Nc, c, col.background);
            continue;
        }
        const int m = (int)(((int64_t)n_mels * (Sm - 1 - y)) / Sm);
        const float p = mel[(size_t)m * F + j];
        if (!finite_bits(__float_as_uint(p))) {
            put(band, y0 + y, Nc, c, col.warning);
            continue;
        }
        int a = 0, b = kFactors;  // the number of thresholds fl32(ref * k[i]) <= p; they ascend
        while (a < b) {
            const int h = (a + b) >> 1;
            if (p >= __fmul_rn(ref, factors[h])) a = h + 1;
            else b = h;
        }
        put(band, y0 + y, Nc, c, colormap + 3 * a);
    }
}

// ---- compose ---------------------------------------------------------------------------------------------------------------------------------
struct ComposeArgs {
    const uint8_t* frames;
    const uint8_t* band;
    const int32_t* c0;
    const int32_t* ph;
    uint8_t* out;
    int64_t rows;  // n * (H + S)
    int H, S, W, Nc;
    uint8_t background[3], playhead[3];
};

// byte ``b`` of row ``y`` of the band part of image i
__device__ __forceinline__ uint8_t band_byte(const ComposeArgs& g, int y, int64_t c0, int64_t ph, int b) {
    const int x = b / 3, ch = b - 3 * x;
    const int64_t p = ph - c0, gc = c0 + x;
    if (ph >= 0 && x >= p && x < p + kPlayW) return g.playhead[ch];
    if (gc >= 0 && gc < g.Nc) return g.band[((size_t)y * g.Nc + (size_t)gc) * 3 + ch];
    return g.background[ch];
}

// kRowsPerBlock output rows per workgroup; VEC: 16 bytes per lane (row length and both bases are multiples of 16), else a byte per lane
template <bool VEC>
__global__ __launch_bounds__(256) void strip_compose_kernel(ComposeArgs g) {
    const int HS = g.H + g.S;
    const int RB = g.W * 3;
    for (int q = 0; q < kRowsPerBlock; ++q) {
        const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + q;
        if (r >= g.rows) return;
        const int64_t i = r / HS;
        const int y = (int)(r - i * HS);
        uint8_t* dst = g.out + (size_t)r * RB;
        if (y < g.H) {
            const uint8_t* src = g.frames + ((size_t)i * g.H + y) * RB;
            if (VEC) {
                for (int k = threadIdx.x; k < RB / 16; k += 256) reinterpret_cast<uint4*>(dst)[k] = reinterpret_cast<const uint4*>(src)[k];
            } else {
                for (int k = threadIdx.x; k < RB; k += 256) dst[k] = src[k];
            }
            continue;
        }
        const int yb = y - g.H;
        const int64_t c0 = g.c0[i], ph = g.ph[i];
        if (VEC) {
            for (int k = threadIdx.x; k < RB / 16; k += 256) {
                const int b = 16 * k, x0 = b / 3, x1 = (b + 15) / 3;
                const int64_t p = ph - c0;
                uint4 v;
                if (c0 + x0 >= 0 && c0 + x1 < g.Nc && !(ph >= 0 && x1 >= p && x0 < p + kPlayW)) {
                    __builtin_memcpy(&v, g.band + ((size_t)yb * g.Nc + (size_t)c0) * 3 + b, 16);  // (any byte alignment)
                } else {
                    uint8_t t[16];
#pragma unroll
                    for (int e = 0; e < 16; ++e) t[e] = band_byte(g, yb, c0, ph, b + e);
                    __builtin_memcpy(&v, t, 16);
                }
                reinterpret_cast<uint4*>(dst)[k] = v;
            }
        } else {
            for (int k = threadIdx.x; k < RB; k += 256) dst[k] = band_byte(g, yb, c0, ph, k);
        }
    }
}

bool lanes_ok(int S) { return S >= SDT_STRIP_MIN_HEIGHT && S <= SDT_STRIP_MAX_HEIGHT; }

}  // namespace

extern "C" int sdt_strip_envelope_f32(const float* audio, int64_t L, const int64_t* bounds, int Nc, float* env, int32_t* flags, int64_t* stats,
                                      void* stream) {
    SDT_CHECK_ARG(audio && bounds && env && flags && stats, "null pointer");
    SDT_CHECK_ARG(L >= 1 && L <= ((int64_t)1 << 40), "samples outside [1, 2^40]");
    SDT_CHECK_ARG(Nc >= 1 && Nc <= SDT_STRIP_MAX_COLUMNS, "columns outside [1, 2^24]");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(stats, 0, 2 * sizeof(int64_t), s) != hipSuccess) {
        sdt_set_error("%s: clearing the statistics failed", __func__);
        return SDT_ERR_LAUNCH;
    }
    const int64_t blocks = std::min<int64_t>(cdiv64(L, 256), 2048);
    hipLaunchKernelGGL(strip_peak_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const uint32_t*)audio, L, (unsigned long long*)stats);
    hipLaunchKernelGGL(strip_envelope_kernel, dim3((unsigned)cdiv(Nc, 4)), dim3(256), 0, s, (const uint32_t*)audio, L, bounds, Nc, (uint32_t*)env,
                       flags);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_strip_raster_u8(const float* env, const int32_t* flags, const int64_t* stats, const int64_t* bounds, int Nc, const float* mel,
                                   int n_mels, int64_t F, const uint8_t* colormap, const float* factors, const int32_t* ticks0, int n0,
                                   const int32_t* ticks1, int n1, const int32_t* ticks2, int n2, const uint8_t* colours, int S, void* work,
                                   uint8_t* band, void* stream) {
    SDT_CHECK_ARG(env && flags && stats && bounds && mel && colormap && factors && colours && work && band, "null pointer");
    SDT_CHECK_ARG(Nc >= 1 && Nc <= SDT_STRIP_MAX_COLUMNS, "columns outside [1, 2^24]");
    SDT_CHECK_ARG(n_mels >= 1 && n_mels <= 4096 && F >= 1 && F <= ((int64_t)1 << 32), "mel bins outside [1, 4096] or frames outside [1, 2^32]");
    SDT_CHECK_ARG(lanes_ok(S), "band height outside [64, 1024]");
    SDT_CHECK_ARG(n0 >= 0 && n1 >= 0 && n2 >= 0 && (n0 == 0 || ticks0) && (n1 == 0 || ticks1) && (n2 == 0 || ticks2),
                  "a tick list with n > 0 needs its pointer");
    Ticks tk = {{ticks0, ticks1, ticks2}, {n0, n1, n2}};
    Colours col;  // ``colours``: a host array of 6 BGR triples, read during the call
    memcpy(&col, colours, sizeof(col));
    static_assert(sizeof(Colours) == 3 * SDT_STRIP_COLOURS, "six BGR triples");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(strip_mel_ref_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t*)mel, (int64_t)n_mels * F, (uint32_t*)work);
    hipLaunchKernelGGL(strip_raster_kernel, dim3((unsigned)cdiv(Nc, 256)), dim3(256), 0, s, env, flags, (const unsigned long long*)stats, bounds,
                       Nc, mel, n_mels, F, (const uint32_t*)work, colormap, factors, tk, col, S, band);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_strip_compose_u8(const uint8_t* frames, int64_t n, int H, int W, const uint8_t* band, int S, int Nc, const int32_t* c0,
                                    const int32_t* ph, const uint8_t* background, const uint8_t* playhead, uint8_t* out, int64_t out_bytes,
                                    void* stream) {
    SDT_CHECK_ARG(frames && band && c0 && ph && background && playhead && out, "null pointer");
    SDT_CHECK_ARG(n >= 1 && H >= 1 && W >= 1 && H <= 65535 && W <= (1 << 24), "images, rows or columns outside their ranges");
    SDT_CHECK_ARG(lanes_ok(S) && Nc >= 1 && Nc <= SDT_STRIP_MAX_COLUMNS, "band height outside [64, 1024] or columns outside [1, 2^24]");
    const int64_t rows = n * (int64_t)(H + S);
    SDT_CHECK_ARG(n <= ((int64_t)1 << 31) / (H + S) * kRowsPerBlock, "too many images for one launch");
    SDT_CHECK_ARG(out_bytes == rows * W * 3, "out must hold n * (H + S) * W * 3 bytes");
    ComposeArgs g;
    g.frames = frames, g.band = band, g.c0 = c0, g.ph = ph, g.out = out, g.rows = rows, g.H = H, g.S = S, g.W = W, g.Nc = Nc;
    memcpy(g.background, background, 3);  // (host arrays, read during the call)
    memcpy(g.playhead, playhead, 3);
    const bool vec = (W * 3) % 16 == 0 && ((uintptr_t)frames & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 grid((unsigned)cdiv64(rows, kRowsPerBlock));
    if (vec) hipLaunchKernelGGL(strip_compose_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL(strip_compose_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, g);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_strip_compose_vectorised(const void* frames, int W, const void* out) {
    return (W * 3) % 16 == 0 && ((uintptr_t)frames & 15) == 0 && ((uintptr_t)out & 15) == 0;
}
