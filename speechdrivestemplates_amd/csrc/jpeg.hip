// Baseline JPEG encoder for the renderer's frames: (N, H, W, 3) uint8 BGR -> one packed buffer of entropy-coded scans
// (SOF0, YCbCr 4:2:0, one scan, restart interval = one MCU row).  Integer arithmetic only, so a host model reproduces
// the stream byte for byte.  Contract and numbers: DESIGN.md section 14.
//   jpeg_dct_kernel      a workgroup takes 8 MCUs of one MCU row: colour conversion with the last row / column
//                        replicated, 2x2 chroma mean, the 13-bit LLM integer forward DCT ("islow"), quantisation;
//                        writes the 6 blocks of each MCU as int16 in zigzag order plus a 64-bit nonzero mask per block.
//   jpeg_entropy_kernel  one wave64 per restart interval, lanes over MCUs.  A lane counts the bits of its MCU, a wave
//                        prefix scan places them, the lanes OR their codes into an LDS staging buffer (LDS atomics), and
//                        the wave emits the finished bytes with 0xFF stuffing through a ballot and a prefix popcount.
//                        Instantiated twice: the measuring pass only returns the interval's byte length, the packing
//                        pass writes the bytes at the interval's final offset.
//   jpeg_scan_kernel     exclusive prefix sum of the interval lengths (one workgroup).
// The Huffman code tables and the quantisation divisors come from the caller (sdt_hip.h: the `tables` words), so the
// file headers and the scan are derived from one source.  A table cannot make the kernels write out of bounds: code
// lengths are clamped to 16 bits, the staging buffer is filled by counted bits, and the packing pass checks every byte
// position against the interval's range from the measuring pass.
#include "common.h"

namespace {

constexpr int kGroup = 8;             // MCUs per workgroup of the DCT kernel
constexpr int kTileW = 16 * kGroup;   // pixels
constexpr int kBlocks = 6 * kGroup;   // 8x8 blocks per workgroup
constexpr int kWsPitch = 72;          // words per block in the transpose buffer (64 + 8: column reads hit 32 banks)
constexpr int kTabWords = SDT_JPEG_TABLE_WORDS;
constexpr int kQuantWords = 128, kDcLum = 128, kDcChr = 144, kAcLum = 160, kAcChr = 416;
constexpr int kStageWords = 4096;     // 131072 bits of staging per wave; one MCU is at most 6 * (27 + 63 * 26 + 3 * 16) bits
constexpr int kStageBits = kStageWords * 32;

// zigzag position of the coefficient at natural index row * 8 + column
__constant__ uint8_t kZigzagOf[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                      41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                      46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// One 1-D pass of the LLM forward DCT in 13-bit fixed point (the "islow" integer DCT).  The first pass keeps 2 extra
// bits (outputs scaled by 4 * sqrt(8) / 2), the second removes them and leaves the factor 8 of the 2-D transform.
template <bool FIRST>
__device__ __forceinline__ void fdct_1d(int (&d)[8]) {
    constexpr int kConst = 13, kPass1 = 2;
    constexpr int sh_odd = FIRST ? kConst - kPass1 : kConst + kPass1;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) << kPass1;
        d[4] = (t10 - t11) << kPass1;
    } else {
        d[0] = (t10 + t11 + (1 << (kPass1 - 1))) >> kPass1;
        d[4] = (t10 - t11 + (1 << (kPass1 - 1))) >> kPass1;
    }
    constexpr int r = 1 << (sh_odd - 1);
    int z1 = (t12 + t13) * 4433;
    d[2] = (z1 + t13 * 6270 + r) >> sh_odd;
    d[6] = (z1 - t12 * 15137 + r) >> sh_odd;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = (a4 + z1 + z3 + r) >> sh_odd;
    d[5] = (a5 + z2 + z4 + r) >> sh_odd;
    d[3] = (a6 + z2 + z3 + r) >> sh_odd;
    d[1] = (a7 + z1 + z4 + r) >> sh_odd;
}

__device__ __forceinline__ int bit_length(unsigned v) { return v ? 32 - __clz((int)v) : 0; }

// Sink of the counting walk: adds code lengths.
struct BitCounter {
    int bits = 0;
    __device__ __forceinline__ void put(uint32_t, int len) { bits += len; }
};

// Sink of the emitting walk: MSB-first bits ORed into big-endian 32-bit words of the LDS staging buffer.  The first and
// the last word of a lane's range are shared with its neighbours, hence atomicOr; the buffer was zeroed before.
struct BitWriter {
    uint32_t* buf;
    uint64_t acc = 0;
    int word, n;  // n < 32 pending bits in the low end of acc, headed for buf[word]
    __device__ BitWriter(uint32_t* b, int start_bit) : buf(b), word(start_bit >> 5), n(start_bit & 31) {}
    __device__ __forceinline__ void put(uint32_t code, int len) {
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            n -= 32;
            if (word < kStageWords) atomicOr(&buf[word], (uint32_t)(acc >> n));
            ++word;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n > 0 && word < kStageWords) atomicOr(&buf[word], (uint32_t)(acc << (32 - n)));
    }
};

// Huffman-codes the 6 blocks of MCU `m` of an interval (coefficients and masks of the interval start at blk / msk) into
// `sink`.  DC prediction runs through the interval per component and starts from 0.
template <class Sink>
__device__ __forceinline__ void walk_mcu(Sink& sink, const int16_t* __restrict__ blk, const uint64_t* __restrict__ msk, int m,
                                         const uint32_t* s_tab) {
#pragma unroll 1
    for (int b = 0; b < 6; ++b) {
        const int16_t* c = blk + ((int64_t)m * 6 + b) * 64;
        const uint32_t* dc_tab = s_tab + (b < 4 ? kDcLum : kDcChr) - kQuantWords;
        const uint32_t* ac_tab = s_tab + (b < 4 ? kAcLum : kAcChr) - kQuantWords;
        int pred;
        if (b >= 1 && b <= 3)
            pred = c[-64];
        else
            pred = m == 0 ? 0 : c[-(b == 0 ? 3 : 6) * 64];  // Y: the previous MCU's fourth block; Cb / Cr: its own block there
        const int diff = (int)c[0] - pred;
        int nb = bit_length((unsigned)abs(diff));
        uint32_t e = dc_tab[nb & 15];
        sink.put(((e & 0xffffu) << nb) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u)), (int)(e >> 16) + nb);
        uint64_t rest = msk[(int64_t)m * 6 + b] & ~1ull;
        int prev = 0;
        while (rest) {
            const int k = __ffsll((unsigned long long)rest) - 1;
            rest &= rest - 1;
            int run = k - prev - 1;
            prev = k;
            for (; run > 15; run -= 16) {
                e = ac_tab[0xf0];
                sink.put(e & 0xffffu, (int)(e >> 16));
            }
            const int v = c[k];
            nb = bit_length((unsigned)abs(v)) & 15;
            e = ac_tab[(run << 4) | nb];
            sink.put(((e & 0xffffu) << nb) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u)), (int)(e >> 16) + nb);
        }
        if (prev != 63) {
            e = ac_tab[0];
            sink.put(e & 0xffffu, (int)(e >> 16));
        }
    }
}

__device__ __forceinline__ uint32_t stage_byte(const uint32_t* buf, int i) { return (buf[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu; }

}  // namespace

__global__ __launch_bounds__(256) void jpeg_dct_kernel(const uint8_t* __restrict__ frames, int H, int W, int mcus_w, int rows,
                                                       const uint32_t* __restrict__ tables, int16_t* __restrict__ coef,
                                                       uint64_t* __restrict__ mask) {
    __shared__ uint8_t s_y[16][kTileW], s_cb[16][kTileW], s_cr[16][kTileW];
    __shared__ int s_ws[kBlocks * kWsPitch];
    __shared__ int16_t s_q[kBlocks][64];
    __shared__ int s_quant[kQuantWords];
    const int tid = threadIdx.x, img = blockIdx.z, my = blockIdx.y, mx0 = blockIdx.x * kGroup;
    const uint8_t* src = frames + (int64_t)img * H * W * 3;
    if (tid < kQuantWords) s_quant[tid] = (int)min(max(tables[tid], 1u), 255u);
    // colour conversion; rows / columns past the image repeat the last one
    for (int i = tid; i < 16 * kTileW; i += 256) {
        const int r = i / kTileW, c = i % kTileW;
        const int y = min(my * 16 + r, H - 1), x = min(mx0 * 16 + c, W - 1);
        const uint8_t* p = src + ((int64_t)y * W + x) * 3;
        const int B = p[0], G = p[1], R = p[2];
        s_y[r][c] = (uint8_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
        s_cb[r][c] = (uint8_t)((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16);
        s_cr[r][c] = (uint8_t)((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16);
    }
    __syncthreads();
    // row pass: item = (block, row)
    for (int item = tid; item < kBlocks * 8; item += 256) {
        const int b = item >> 3, r = item & 7, g = b / 6, k = b % 6;
        int d[8];
        if (k < 4) {
            const uint8_t* s = &s_y[(k >> 1) * 8 + r][g * 16 + (k & 1) * 8];
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = (int)s[j] - 128;
        } else {
            const uint8_t* s0 = (k == 4 ? &s_cb[2 * r][g * 16] : &s_cr[2 * r][g * 16]);
            const uint8_t* s1 = s0 + kTileW;
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = (((int)s0[2 * j] + s0[2 * j + 1] + s1[2 * j] + s1[2 * j + 1] + 1 + (j & 1)) >> 2) - 128;
        }
        fdct_1d<true>(d);
        int* w = s_ws + b * kWsPitch + r * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = d[j];
    }
    __syncthreads();
    // column pass and quantisation: item = (block, column)
    for (int item = tid; item < kBlocks * 8; item += 256) {
        const int b = item >> 3, c = item & 7, k = b % 6;
        const int* w = s_ws + b * kWsPitch + c;
        int d[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = w[j * 8];
        fdct_1d<false>(d);
        const int* q = s_quant + (k < 4 ? 0 : 64) + c;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int qv = q[j * 8], a = (abs(d[j]) + 4 * qv) / (8 * qv);
            s_q[b][kZigzagOf[j * 8 + c]] = (int16_t)(d[j] < 0 ? -a : a);
        }
    }
    __syncthreads();
    // a wave writes one block per step: 128 contiguous bytes, and the ballot is the block's nonzero mask
    const int lane = tid & 63, wave = tid >> 6;
    for (int b = wave; b < kBlocks; b += 4) {
        const int g = b / 6, k = b % 6;
        if (mx0 + g >= mcus_w) continue;  // (uniform over the wave)
        const int16_t v = s_q[b][lane];
        const uint64_t nz = __ballot(v != 0);
        const int64_t block = ((((int64_t)img * rows + my) * mcus_w + mx0 + g) * 6 + k);
        coef[block * 64 + lane] = v;
        if (lane == 0) mask[block] = nz;
    }
}

template <bool WRITE>
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const int16_t* __restrict__ coef, const uint64_t* __restrict__ mask,
                                                          const uint32_t* __restrict__ tables, int mcus_w, int rows,
                                                          const int64_t* __restrict__ offsets, int64_t* __restrict__ lengths,
                                                          uint8_t* __restrict__ out, int64_t out_bytes, int32_t* __restrict__ err) {
    __shared__ uint32_t s_tab[kTabWords - kQuantWords];
    __shared__ uint32_t s_buf[kStageWords];
    const int lane = threadIdx.x;
    const int64_t itv = blockIdx.x;
    for (int i = lane; i < kTabWords - kQuantWords; i += 64) {
        const uint32_t e = tables[kQuantWords + i];
        s_tab[i] = (e & 0xffffu) | (min(e >> 16, 16u) << 16);
    }
    const int16_t* blk = coef + itv * mcus_w * 6 * 64;
    const uint64_t* msk = mask + itv * mcus_w * 6;
    // byte range of this interval in the packed buffer (packing pass); `pos` counts from 0 in the measuring pass
    int64_t pos = 0, end = 0;
    if (WRITE) {
        pos = offsets[itv];
        end = min(offsets[itv + 1], out_bytes);
        if (pos < 0 || pos > end) {
            if (lane == 0) atomicOr(err, SDT_JPEG_ERR_RANGE);
            return;
        }
    }
    bool bad = false;
    int carry_bits = 0;       // < 8 bits left over from the previous chunk ...
    uint32_t carry_word = 0;  // ... in the top of this word
    __syncthreads();
    for (int m0 = 0; m0 < mcus_w;) {
        const int m = m0 + lane;
        int nb = 0;
        if (m < mcus_w) {
            BitCounter cnt;
            walk_mcu(cnt, blk, msk, m, s_tab);
            nb = cnt.bits;
        }
        int incl = nb;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        // the leading lanes whose MCUs fit into the staging buffer form this chunk (incl never decreases)
        const uint64_t fit = __ballot(m < mcus_w && carry_bits + incl <= kStageBits);
        const int k = __popcll(fit);
        if (k == 0) {  // one MCU longer than the staging buffer: impossible with code lengths <= 16
            if (lane == 0) atomicOr(err, SDT_JPEG_ERR_STAGE);
            return;
        }
        const int total = carry_bits + __shfl(incl, k - 1, 64);
        for (int w = lane; w < (total + 31) / 32; w += 64) s_buf[w] = w == 0 ? carry_word : 0u;
        __syncthreads();
        if (lane < k) {
            BitWriter wr(s_buf, carry_bits + incl - nb);
            walk_mcu(wr, blk, msk, m, s_tab);
            wr.finish();
        }
        __syncthreads();
        const int nbytes = total >> 3;
        for (int base = 0; base < nbytes; base += 64) {
            const int i = base + lane;
            const bool valid = i < nbytes;
            const uint32_t byte = valid ? stage_byte(s_buf, i) : 0u;
            const bool ff = valid && byte == 0xffu;
            const uint64_t ffm = __ballot(ff);
            if (WRITE && valid) {
                const int64_t p = pos + lane + __popcll(ffm & ((1ull << lane) - 1ull));
                if (p + (ff ? 1 : 0) < end) {
                    out[p] = (uint8_t)byte;
                    if (ff) out[p + 1] = 0;
                } else {
                    bad = true;
                }
            }
            pos += min(64, nbytes - base) + __popcll(ffm);
        }
        carry_bits = total & 7;
        carry_word = carry_bits ? stage_byte(s_buf, nbytes) << 24 : 0u;
        __syncthreads();  // the next chunk zeroes the buffer
        m0 += k;
    }
    // pad the last byte with 1-bits, then RSTn (n = interval index within the image, modulo 8) or, after the image's
    // last interval, EOI
    const int row = (int)(itv % rows);
    uint8_t tail[4];
    int nt = 0;
    if (carry_bits) {
        const uint32_t byte = (carry_word >> 24) | (0xffu >> carry_bits);
        tail[nt++] = (uint8_t)byte;
        if (byte == 0xffu) tail[nt++] = 0;
    }
    tail[nt++] = 0xff;
    tail[nt++] = row == rows - 1 ? 0xd9 : (uint8_t)(0xd0 + (row & 7));
    if (WRITE) {
        if (lane == 0) {
            if (pos + nt == end)
                for (int i = 0; i < nt; ++i) out[pos + i] = tail[i];
            else
                bad = true;
        }
        if (__ballot(bad) && lane == 0) atomicOr(err, SDT_JPEG_ERR_RANGE);
    } else if (lane == 0) {
        lengths[itv] = pos + nt;
    }
}

// offsets[i] = sum of lengths[0..i), offsets[n] = the total; one workgroup, each thread sums one contiguous slice
__global__ __launch_bounds__(1024) void jpeg_scan_kernel(const int64_t* __restrict__ lengths, int64_t n, int64_t* __restrict__ offsets) {
    __shared__ int64_t s_part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (n + 1023) / 1024, a = min((int64_t)tid * per, n), b = min(a + per, n);
    int64_t s = 0;
    for (int64_t i = a; i < b; ++i) s += lengths[i];
    s_part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t t = tid >= o ? s_part[tid - o] : 0;
        __syncthreads();
        s_part[tid] += t;
        __syncthreads();
    }
    int64_t run = s_part[tid] - s;
    for (int64_t i = a; i < b; ++i) {
        offsets[i] = run;
        run += lengths[i];
    }
    if (tid == 1023) offsets[n] = s_part[1023];
}

namespace {

struct Geometry {
    int mcus_w, rows;
    int64_t intervals, blocks, coef_bytes, mask_bytes, length_bytes;
};

bool geometry(int n, int H, int W, Geometry& g) {
    if (n <= 0 || n > 65535 || H <= 0 || W <= 0 || H > 65535 || W > 65535) return false;
    g.mcus_w = (W + 15) / 16;
    g.rows = (H + 15) / 16;
    g.intervals = (int64_t)n * g.rows;
    if (g.intervals > 0x7fffffff) return false;
    g.blocks = g.intervals * g.mcus_w * 6;
    g.coef_bytes = g.blocks * 128;
    g.mask_bytes = g.blocks * 8;
    g.length_bytes = g.intervals * 8;
    return true;
}

}  // namespace

extern "C" int64_t sdt_jpeg_workspace_bytes(int n, int H, int W) {
    Geometry g;
    return geometry(n, H, W, g) ? g.coef_bytes + g.mask_bytes + g.length_bytes : 0;
}

extern "C" int64_t sdt_jpeg_intervals(int n, int H, int W) {
    Geometry g;
    return geometry(n, H, W, g) ? g.intervals : 0;
}

extern "C" int sdt_jpeg_measure(const uint8_t* frames, int64_t frames_bytes, int n, int H, int W, const uint32_t* tables, void* workspace,
                                int64_t workspace_bytes, int64_t* offsets, int64_t offsets_elems, int32_t* err, void* stream) {
    Geometry g;
    SDT_CHECK_ARG(geometry(n, H, W, g), "need 1 <= n, H, W <= 65535 and at most 2^31 - 1 restart intervals");
    SDT_CHECK_ARG(frames != nullptr && tables != nullptr && workspace != nullptr && offsets != nullptr && err != nullptr, "null pointer");
    SDT_CHECK_ARG(frames_bytes >= (int64_t)n * H * W * 3, "frame buffer too small");
    SDT_CHECK_ARG(workspace_bytes >= g.coef_bytes + g.mask_bytes + g.length_bytes, "workspace too small");
    SDT_CHECK_ARG(offsets_elems >= g.intervals + 1, "offset table too small");
    SDT_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)offsets & 7) == 0, "workspace must be 16-byte, offsets 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int16_t* coef = (int16_t*)workspace;
    uint64_t* mask = (uint64_t*)((char*)workspace + g.coef_bytes);
    int64_t* lengths = (int64_t*)((char*)workspace + g.coef_bytes + g.mask_bytes);
    if (hipMemsetAsync(err, 0, sizeof(int32_t), st) != hipSuccess) {
        sdt_set_error("%s: hipMemsetAsync failed", __func__);
        return SDT_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(jpeg_dct_kernel, dim3(cdiv(g.mcus_w, kGroup), g.rows, n), dim3(256), 0, st, frames, H, W, g.mcus_w, g.rows, tables,
                       coef, mask);
    SDT_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3((unsigned)g.intervals), dim3(64), 0, st, coef, mask, tables, g.mcus_w, g.rows,
                       (const int64_t*)nullptr, lengths, (uint8_t*)nullptr, (int64_t)0, err);
    SDT_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(1024), 0, st, lengths, g.intervals, offsets);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_jpeg_pack(const void* workspace, int64_t workspace_bytes, int n, int H, int W, const uint32_t* tables,
                             const int64_t* offsets, int64_t offsets_elems, uint8_t* out, int64_t out_bytes, int32_t* err, void* stream) {
    Geometry g;
    SDT_CHECK_ARG(geometry(n, H, W, g), "need 1 <= n, H, W <= 65535 and at most 2^31 - 1 restart intervals");
    SDT_CHECK_ARG(tables != nullptr && workspace != nullptr && offsets != nullptr && out != nullptr && err != nullptr, "null pointer");
    SDT_CHECK_ARG(workspace_bytes >= g.coef_bytes + g.mask_bytes + g.length_bytes, "workspace too small");
    SDT_CHECK_ARG(offsets_elems >= g.intervals + 1 && out_bytes > 0, "offset table or output too small");
    SDT_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)offsets & 7) == 0, "workspace must be 16-byte, offsets 8-byte aligned");
    const int16_t* coef = (const int16_t*)workspace;
    const uint64_t* mask = (const uint64_t*)((const char*)workspace + g.coef_bytes);
    hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3((unsigned)g.intervals), dim3(64), 0, (hipStream_t)stream, coef, mask, tables,
                       g.mcus_w, g.rows, offsets, (int64_t*)nullptr, out, out_bytes, err);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
