// Animated-GIF encoder for the renderer's frames: (T, H, W, 3) uint8 BGR -> one palette, (T, h, w) palette indices and one packed
// buffer of per-frame LZW streams.  Integer arithmetic only, so a host model (gif.py: model_*) reproduces every byte.  Contract and
// numbers: include/sdt_hip.h and DESIGN.md section 15.
//   gif_downscale_hist_kernel  a workgroup takes 256 output columns of 4 output rows: each source row of a window is staged in LDS with
//                              aligned dword loads, a thread sums its column window from there; writes RGB (optional) and the 15-bit
//                              bin, and counts the bins in an LDS hash table (a wave whose pixels agree adds once) that is flushed
//                              with one global integer atomic per distinct bin.
//   gif_palette_kernel         one workgroup, 32 bins per thread in registers: binary search for the count of the 256th most
//                              populated bin, then two block scans place the ties (lower bin first) and number the palette.
//   gif_map_kernel             bin -> nearest palette entry in 5-bit space (wide launch, palette in LDS).
//   gif_index_kernel           pixel bin -> palette index.
//   gif_lzw_kernel             one wave64 per segment; the dictionary keys prefix << 8 | byte live in LDS in code order, a lookup is
//                              every lane comparing one entry per step and a ballot.  Only entries younger than the prefix are searched.
//   gif_scan_kernel            per frame the bit offset of every segment, per clip the byte offset of every frame (one workgroup).
//   gif_pack_kernel            one wave64 per segment ORs its codes into an LDS staging buffer (a code's position and width follow from
//                              its index alone) and writes whole words; words shared with a neighbour go out as atomic OR.
#include "common.h"

namespace {

constexpr int kBins = 32768;
constexpr int kMaxSeg = 3838;  // 4096 - 258
constexpr int kTileW = 256, kTileRows = 4;
constexpr int kHashSlots = 2048;                   // >= 2 * kTileW * kTileRows: the open-addressed table never fills
constexpr int kSpanPx = 648;                       // source columns under 256 output columns: <= 256 * (2.5 + 2 / w) + 2
constexpr int kSpanWords = (kSpanPx * 3 + 3) / 4 + 2;
constexpr uint32_t kEmpty = 0xffffffffu;
constexpr int kStageWords = 1360;  // 31 + 9 + bits of 3838 codes + 12 = 43295 bits
constexpr int kClear = 256, kEoi = 257, kFirstFree = 258;

__host__ __device__ __forceinline__ int width_after(int k) { return 9 + (k >= 255) + (k >= 767) + (k >= 1791); }
__host__ __device__ __forceinline__ int bits_before(int k) {
    return 9 * k + (k > 255 ? k - 255 : 0) + (k > 767 ? k - 767 : 0) + (k > 1791 ? k - 1791 : 0);
}

struct Geometry {
    int parts, step;       // segments per row, pixels per segment (the last one takes the rest)
    int64_t pixels, segs;  // of the clip
    int64_t hist_off, table_off, palbins_off, counts_off, words_off, bytes;
};

bool geometry(int n, int h, int w, Geometry& g) {
    if (n <= 0 || n > 65535 || h <= 0 || w <= 0 || h > 65535 || w > 65535) return false;
    g.parts = (w + kMaxSeg - 1) / kMaxSeg;
    g.step = (w + g.parts - 1) / g.parts;
    g.pixels = (int64_t)n * h * w;
    g.segs = (int64_t)n * h * g.parts;
    if (g.pixels > 0x7fffffff || g.segs >= (1ll << 26)) return false;
    g.hist_off = 0;
    g.table_off = g.hist_off + kBins * 4;
    g.palbins_off = g.table_off + kBins;
    g.counts_off = g.palbins_off + 1024;  // 256 uint16 palette bins, the palette size, padding
    g.words_off = g.counts_off + g.segs * 16;
    g.bytes = g.words_off + ((g.pixels * 2 + 15) & ~15ll);  // uint16 per pixel: the bins, later the codes
    return true;
}

__device__ __forceinline__ void hash_add(uint32_t* s_key, uint32_t* s_cnt, uint32_t bin, uint32_t cnt) {
    uint32_t slot = (bin * 2654435761u) >> 21;
    for (;;) {
        const uint32_t prev = atomicCAS(&s_key[slot], kEmpty, bin);
        if (prev == kEmpty || prev == bin) {
            atomicAdd(&s_cnt[slot], cnt);
            return;
        }
        slot = (slot + 1) & (kHashSlots - 1);
    }
}

// sum over the 1024 threads of the workgroup (s_red: 16 words)
__device__ __forceinline__ int block_sum(int v, int* s_red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += s_red[i];
    __syncthreads();
    return s;
}

// exclusive prefix sum over the 1024 threads; *total gets the sum
__device__ __forceinline__ int block_scan(int v, int* s_red, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_red[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int t = s_red[i];
        if (i < wave) before += t;
        all += t;
    }
    __syncthreads();
    *total = all;
    return before + incl - v;
}

}  // namespace

__global__ __launch_bounds__(256) void gif_downscale_hist_kernel(const uint8_t* __restrict__ frames, int64_t frames_bytes, int H, int W, int h,
                                                                 int w, uint8_t* __restrict__ rgb, uint16_t* __restrict__ bins,
                                                                 uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_row[kSpanWords];
    __shared__ uint32_t s_key[kHashSlots], s_cnt[kHashSlots];
    const int tid = threadIdx.x, lane = tid & 63, t = blockIdx.z;
    const int j0 = blockIdx.x * kTileW, j1 = min(j0 + kTileW, w), j = j0 + tid;
    const bool valid = j < j1;
    for (int i = tid; i < kHashSlots; i += 256) {
        s_key[i] = kEmpty;
        s_cnt[i] = 0;
    }
    const int c_lo = (int)((int64_t)j0 * W / w), c_hi = (int)(((int64_t)j1 * W + w - 1) / w);
    if ((c_hi - c_lo) * 3 + 3 > kSpanWords * 4) return;  // (uniform; the host checked the geometry: cannot happen)
    const int cw0 = valid ? (int)((int64_t)j * W / w) : c_lo, cw1 = valid ? (int)(((int64_t)(j + 1) * W + w - 1) / w) : c_lo;
    const uint8_t* s_bytes = (const uint8_t*)s_row;
    for (int rr = 0; rr < kTileRows; ++rr) {
        const int i = blockIdx.y * kTileRows + rr;
        if (i >= h) break;
        const int r0 = (int)((int64_t)i * H / h), r1 = (int)(((int64_t)(i + 1) * H + h - 1) / h);
        int sb = 0, sg = 0, sr = 0;
        for (int y = r0; y < r1; ++y) {
            const int64_t g0 = (((int64_t)t * H + y) * W + c_lo) * 3, g1 = g0 + (int64_t)(c_hi - c_lo) * 3;
            const int64_t a0 = g0 & ~3ll;
            const int ndw = (int)((g1 - a0 + 3) >> 2), skew = (int)(g0 - a0);
            __syncthreads();  // the previous row's readers are done
            for (int d = tid; d < ndw; d += 256) {
                const int64_t a = a0 + 4ll * d;
                uint32_t v = 0;
                if (a + 4 <= frames_bytes) {
                    v = *(const uint32_t*)(frames + a);
                } else {
                    for (int b = 0; b < 4; ++b)
                        if (a + b < frames_bytes) v |= (uint32_t)frames[a + b] << (8 * b);
                }
                s_row[d] = v;
            }
            __syncthreads();
            for (int c = cw0; c < cw1; ++c) {
                const uint8_t* p = s_bytes + skew + (c - c_lo) * 3;
                sb += p[0];
                sg += p[1];
                sr += p[2];
            }
        }
        uint32_t bin = 0;
        if (valid) {
            const int n = (r1 - r0) * (cw1 - cw0);
            const int R = (sr + n / 2) / n, G = (sg + n / 2) / n, B = (sb + n / 2) / n;
            const int64_t o = ((int64_t)t * h + i) * w + j;
            if (rgb != nullptr) {
                rgb[o * 3 + 0] = (uint8_t)R;
                rgb[o * 3 + 1] = (uint8_t)G;
                rgb[o * 3 + 2] = (uint8_t)B;
            }
            bin = (uint32_t)(((R >> 3) << 10) | ((G >> 3) << 5) | (B >> 3));
            bins[o] = (uint16_t)bin;
        }
        // (the table was initialised before the first staging barrier)
        const uint64_t vm = __ballot(valid);
        if (vm) {
            const int first = __ffsll((unsigned long long)vm) - 1;
            const uint32_t b0 = __shfl(bin, first, 64);
            const uint64_t same = __ballot(valid && bin == b0);
            if (same == vm) {
                if (lane == first) hash_add(s_key, s_cnt, b0, (uint32_t)__popcll(vm));
            } else if (valid) {
                hash_add(s_key, s_cnt, bin, 1u);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < kHashSlots; i += 256)
        if (s_key[i] != kEmpty) atomicAdd(&hist[s_key[i] & (kBins - 1)], s_cnt[i]);
}

__global__ __launch_bounds__(1024) void gif_palette_kernel(const uint32_t* __restrict__ hist, uint8_t* __restrict__ palette,
                                                           uint16_t* __restrict__ palbins, int32_t* __restrict__ npal) {
    __shared__ int s_red[16];
    const int tid = threadIdx.x;
    uint32_t c[32];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint4 v = ((const uint4*)hist)[tid * 8 + k];
        c[4 * k] = v.x, c[4 * k + 1] = v.y, c[4 * k + 2] = v.z, c[4 * k + 3] = v.w;
    }
    if (tid < 768) palette[tid] = 0;
    if (tid < 256) palbins[tid] = 0;
    int mine = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) mine += c[k] > 0u;
    const int occupied = block_sum(mine, s_red);
    // cut: bins with a count above it are taken, `quota` of the bins at it (the lower bins) too; cut 0 takes every occupied bin
    uint32_t cut = 0;
    int quota = 0;
    if (occupied > 256) {
        uint32_t lo = 1, hi = 0xffffffffu;  // the largest value that at least 256 bins reach
        while (lo < hi) {
            const uint32_t mid = (uint32_t)(((uint64_t)lo + hi + 1) >> 1);
            int m = 0;
#pragma unroll
            for (int k = 0; k < 32; ++k) m += c[k] >= mid;
            if (block_sum(m, s_red) >= 256)
                lo = mid;
            else
                hi = mid - 1;
        }
        cut = lo;
        int m = 0;
#pragma unroll
        for (int k = 0; k < 32; ++k) m += c[k] > cut;
        quota = 256 - block_sum(m, s_red);
    }
    int ties = 0;
    if (cut > 0) {
#pragma unroll
        for (int k = 0; k < 32; ++k) ties += c[k] == cut;
    }
    int total;
    int tie_rank = block_scan(ties, s_red, &total);
    uint32_t take = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        bool sel = c[k] > cut;
        if (cut > 0 && c[k] == cut) sel = tie_rank++ < quota;
        take |= (uint32_t)sel << k;
    }
    int idx = block_scan(__popc(take), s_red, &total);
    while (take) {
        const int k = __ffs((int)take) - 1;
        take &= take - 1;
        if (idx < 256) {
            const int bin = tid * 32 + k, r = bin >> 10, g = (bin >> 5) & 31, b = bin & 31;
            palbins[idx] = (uint16_t)bin;
            palette[idx * 3 + 0] = (uint8_t)((r << 3) | (r >> 2));
            palette[idx * 3 + 1] = (uint8_t)((g << 3) | (g >> 2));
            palette[idx * 3 + 2] = (uint8_t)((b << 3) | (b >> 2));
        }
        ++idx;
    }
    if (tid == 0) *npal = min(total, 256);
}

__global__ __launch_bounds__(256) void gif_map_kernel(const uint16_t* __restrict__ palbins, const int32_t* __restrict__ npal,
                                                      uint8_t* __restrict__ table) {
    __shared__ int s_pal[256];
    const int n = min(max(*npal, 1), 256);
    s_pal[threadIdx.x] = palbins[threadIdx.x];
    __syncthreads();
    const int bin = blockIdx.x * 256 + threadIdx.x, r = bin >> 10, g = (bin >> 5) & 31, b = bin & 31;
    int best = 0, best_d = 1 << 30;
    for (int k = 0; k < n; ++k) {
        const int p = s_pal[k], dr = r - (p >> 10), dg = g - ((p >> 5) & 31), db = b - (p & 31);
        const int d = dr * dr + dg * dg + db * db;
        if (d < best_d) best_d = d, best = k;
    }
    table[bin] = (uint8_t)best;
}

__global__ __launch_bounds__(256) void gif_index_kernel(const uint16_t* __restrict__ bins, const uint8_t* __restrict__ table, int64_t n,
                                                        uint8_t* __restrict__ indices) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) indices[i] = table[bins[i] & (kBins - 1)];
}

// dynamic LDS: `step` uint32 keys, then `step` pixels
__global__ __launch_bounds__(64) void gif_lzw_kernel(const uint8_t* __restrict__ indices, int w, int parts, int step,
                                                     uint16_t* __restrict__ codes, int32_t* __restrict__ counts) {
    extern __shared__ uint32_t s_dyn[];
    uint32_t* s_key = s_dyn;
    uint8_t* s_pix = (uint8_t*)(s_dyn + step);
    const int lane = threadIdx.x;
    const int64_t seg = blockIdx.x, row = seg / parts;
    const int start = (int)(seg % parts) * step, len = min(step, w - start);
    const uint8_t* src = indices + row * w + start;
    uint16_t* out = codes + row * w + start;  // at most len codes
    for (int i = lane; i < len; i += 64) s_pix[i] = src[i];
    __syncthreads();
    int cur = s_pix[0], n = 0, ncodes = 0;  // n entries in the table: entry e has code 258 + e
    for (int i = 1; i < len; ++i) {
        const int b = __builtin_amdgcn_readfirstlane((int)s_pix[i]);
        const uint32_t key = ((uint32_t)cur << 8) | (uint32_t)b;
        int found = -1;
        for (int base = cur >= kFirstFree ? cur - kFirstFree + 1 : 0; base < n; base += 64) {  // an extension is younger than its prefix
            const int e = base + lane;
            const uint64_t m = __ballot(e < n && s_key[e] == key);
            if (m) {
                found = base + __ffsll((unsigned long long)m) - 1;
                break;
            }
        }
        if (found >= 0) {
            cur = kFirstFree + found;
        } else {
            if (lane == 0) {
                out[ncodes] = (uint16_t)cur;
                s_key[n] = key;
            }
            ++ncodes;
            ++n;
            cur = b;
            __syncthreads();  // (one wave: orders the new key before the next lookup)
        }
    }
    if (lane == 0) {
        out[ncodes] = (uint16_t)cur;
        ++ncodes;
        counts[seg * 4 + 0] = ncodes;
        counts[seg * 4 + 1] = bits_before(ncodes);
        counts[seg * 4 + 2] = width_after(ncodes);  // the width of the Clear / EOI that follows
        counts[seg * 4 + 3] = 0;
    }
}

// offsets[0 .. T]: byte offset of every frame's stream and the total; offsets[T + 1 + s]: bit offset of segment s's first code.
// A frame starts on a byte with a 9-bit Clear; every segment is followed by one code of its end width.
__global__ __launch_bounds__(1024) void gif_scan_kernel(const int32_t* __restrict__ counts, int T, int per_frame, int64_t* __restrict__ offsets) {
    __shared__ int64_t s_part[1024];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int f = wave; f < T; f += 16) {
        int64_t bits = 0;
        for (int s = lane; s < per_frame; s += 64) {
            const int32_t* c = counts + ((int64_t)f * per_frame + s) * 4;
            bits += c[1] + c[2];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bits += __shfl_xor(bits, o, 64);
        if (lane == 0) offsets[f + 1] = (bits + 9 + 7) >> 3;
    }
    if (tid == 0) offsets[0] = 0;
    __syncthreads();
    // inclusive scan of offsets[1 .. T] in place: each thread sums one contiguous slice
    const int per = (T + 1023) / 1024, a = min(tid * per, T), b = min(a + per, T);
    int64_t sum = 0;
    for (int i = a; i < b; ++i) sum += offsets[i + 1];
    s_part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t t = tid >= o ? s_part[tid - o] : 0;
        __syncthreads();
        s_part[tid] += t;
        __syncthreads();
    }
    int64_t run = s_part[tid] - sum;
    for (int i = a; i < b; ++i) {
        run += offsets[i + 1];
        offsets[i + 1] = run;
    }
    __syncthreads();
    for (int f = wave; f < T; f += 16) {
        int64_t run_bits = offsets[f] * 8 + 9;
        for (int s0 = 0; s0 < per_frame; s0 += 64) {
            const int s = s0 + lane;
            int64_t v = 0;
            if (s < per_frame) {
                const int32_t* c = counts + ((int64_t)f * per_frame + s) * 4;
                v = c[1] + c[2];
            }
            int64_t incl = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int64_t t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            if (s < per_frame) offsets[T + 1 + (int64_t)f * per_frame + s] = run_bits + incl - v;
            run_bits += __shfl(incl, 63, 64);
        }
    }
}

__global__ __launch_bounds__(64) void gif_pack_kernel(const uint16_t* __restrict__ codes, const int32_t* __restrict__ counts, int w, int parts,
                                                      int step, int T, int per_frame, const int64_t* __restrict__ offsets,
                                                      uint32_t* __restrict__ out, int64_t out_bytes, int32_t* __restrict__ err) {
    __shared__ uint32_t s_buf[kStageWords];
    const int lane = threadIdx.x;
    const int64_t seg = blockIdx.x, row = seg / parts;
    const int start = (int)(seg % parts) * step, len = min(step, w - start);
    const int64_t f = seg / per_frame;
    const bool first = seg % per_frame == 0, last = seg % per_frame == per_frame - 1;
    const uint16_t* src = codes + row * w + start;
    const int ncodes = counts[seg * 4];
    if (ncodes < 1 || ncodes > len) {  // not a workspace that measure left for this geometry
        if (lane == 0) atomicOr(err, SDT_GIF_ERR_COUNT);
        return;
    }
    // the frame's byte range and this segment's first bit (the frame's first segment also writes the Clear in front of it)
    const int64_t fb = offsets[f], fe = min(offsets[f + 1], out_bytes);
    const int lead = first ? 9 : 0;
    const int64_t bit0 = offsets[T + 1 + seg] - lead;
    if (fb < 0 || fe < fb || bit0 < 0) {
        if (lane == 0) atomicOr(err, SDT_GIF_ERR_RANGE);
        return;
    }
    const int rel0 = (int)(bit0 & 31) + lead;
    const int64_t word0 = bit0 >> 5;
    const int nwords = (rel0 + bits_before(ncodes) + width_after(ncodes) + 31) >> 5;  // <= kStageWords since ncodes <= 3838
    for (int i = lane; i < nwords; i += 64) s_buf[i] = 0;
    __syncthreads();
    if (first && lane == 0) {
        const uint64_t v = (uint64_t)kClear << (rel0 - 9);
        atomicOr(&s_buf[0], (uint32_t)v);
        if (v >> 32) atomicOr(&s_buf[1], (uint32_t)(v >> 32));
    }
    for (int k = lane; k <= ncodes; k += 64) {
        const int width = width_after(k), pos = rel0 + bits_before(k);
        const uint32_t code = (k < ncodes ? (uint32_t)src[k] : (uint32_t)(last ? kEoi : kClear)) & ((1u << width) - 1u);
        const uint64_t v = (uint64_t)code << (pos & 31);
        atomicOr(&s_buf[pos >> 5], (uint32_t)v);
        if (v >> 32) atomicOr(&s_buf[(pos >> 5) + 1], (uint32_t)(v >> 32));
    }
    __syncthreads();
    bool bad = false;
    for (int i = lane; i < nwords; i += 64) {
        uint32_t v = s_buf[i];
        const int64_t byte = (word0 + i) * 4;
        // keep the bytes inside [fb, fe); bits that fall outside are dropped and reported
        uint32_t keep = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (byte + b >= fb && byte + b < fe) keep |= 0xffu << (8 * b);
        if (v & ~keep) bad = true;
        v &= keep;
        if (keep == 0 || byte + 4 > out_bytes) continue;
        if (keep != 0xffffffffu || i == 0 || i == nwords - 1)
            atomicOr(&out[word0 + i], v);  // shared with the neighbouring segment or frame
        else
            out[word0 + i] = v;
    }
    if (__ballot(bad) && lane == 0) atomicOr(err, SDT_GIF_ERR_RANGE);
}

extern "C" int64_t sdt_gif_workspace_bytes(int n, int h, int w) {
    Geometry g;
    return geometry(n, h, w, g) ? g.bytes : 0;
}

extern "C" int sdt_gif_quantise(const uint8_t* frames, int64_t frames_bytes, int n, int H, int W, int h, int w, uint8_t* rgb, int64_t rgb_bytes,
                                uint8_t* indices, int64_t indices_bytes, uint8_t* palette, void* workspace, int64_t workspace_bytes,
                                void* stream) {
    Geometry g;
    SDT_CHECK_ARG(H > 0 && W > 0 && H <= 163839 && W <= 163839, "need 1 <= H, W <= 163839");
    SDT_CHECK_ARG((h == H && w == W) || (h == (int)((2ll * H) / 5) && w == (int)((2ll * W) / 5)),
                  "the output size must be the input size or ((2 H) / 5, (2 W) / 5)");
    SDT_CHECK_ARG(geometry(n, h, w, g), "need 1 <= n, h, w <= 65535, fewer than 2^31 output pixels and 2^26 segments");
    SDT_CHECK_ARG(frames != nullptr && indices != nullptr && palette != nullptr && workspace != nullptr, "null pointer");
    SDT_CHECK_ARG(frames_bytes >= (int64_t)n * H * W * 3, "frame buffer too small");
    SDT_CHECK_ARG(rgb == nullptr || rgb_bytes >= g.pixels * 3, "rgb buffer too small");
    SDT_CHECK_ARG(indices_bytes >= g.pixels, "index buffer too small");
    SDT_CHECK_ARG(workspace_bytes >= g.bytes, "workspace too small");
    SDT_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)frames & 3) == 0, "workspace must be 16-byte, frames 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uint32_t* hist = (uint32_t*)(ws + g.hist_off);
    uint8_t* table = (uint8_t*)(ws + g.table_off);
    uint16_t* palbins = (uint16_t*)(ws + g.palbins_off);
    int32_t* npal = (int32_t*)(ws + g.palbins_off + 512);
    uint16_t* bins = (uint16_t*)(ws + g.words_off);
    if (hipMemsetAsync(hist, 0, kBins * 4, st) != hipSuccess) {
        sdt_set_error("%s: hipMemsetAsync failed", __func__);
        return SDT_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(gif_downscale_hist_kernel, dim3(cdiv(w, kTileW), cdiv(h, kTileRows), n), dim3(256), 0, st, frames,
                       (int64_t)n * H * W * 3, H, W, h, w, rgb, bins, hist);
    SDT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gif_palette_kernel, dim3(1), dim3(1024), 0, st, hist, palette, palbins, npal);
    SDT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gif_map_kernel, dim3(kBins / 256), dim3(256), 0, st, palbins, npal, table);
    SDT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gif_index_kernel, dim3((unsigned)std::min<int64_t>(cdiv64(g.pixels, 256), 65536)), dim3(256), 0, st, bins, table, g.pixels,
                       indices);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_gif_measure(const uint8_t* indices, int64_t indices_bytes, int n, int h, int w, void* workspace, int64_t workspace_bytes,
                               int64_t* offsets, int64_t offsets_elems, int32_t* err, void* stream) {
    Geometry g;
    SDT_CHECK_ARG(geometry(n, h, w, g), "need 1 <= n, h, w <= 65535, fewer than 2^31 pixels and 2^26 segments");
    SDT_CHECK_ARG(indices != nullptr && workspace != nullptr && offsets != nullptr && err != nullptr, "null pointer");
    SDT_CHECK_ARG(indices_bytes >= g.pixels, "index buffer too small");
    SDT_CHECK_ARG(workspace_bytes >= g.bytes, "workspace too small");
    SDT_CHECK_ARG(offsets_elems >= n + 1 + g.segs, "offset table too small");
    SDT_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)offsets & 7) == 0, "workspace must be 16-byte, offsets 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int32_t* counts = (int32_t*)(ws + g.counts_off);
    uint16_t* codes = (uint16_t*)(ws + g.words_off);
    if (hipMemsetAsync(err, 0, sizeof(int32_t), st) != hipSuccess) {
        sdt_set_error("%s: hipMemsetAsync failed", __func__);
        return SDT_ERR_LAUNCH;
    }
    const size_t lds = (size_t)g.step * 4 + (((size_t)g.step + 3) & ~(size_t)3);
    hipLaunchKernelGGL(gif_lzw_kernel, dim3((unsigned)g.segs), dim3(64), lds, st, indices, w, g.parts, g.step, codes, counts);
    SDT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gif_scan_kernel, dim3(1), dim3(1024), 0, st, counts, n, h * g.parts, offsets);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_gif_pack(const void* workspace, int64_t workspace_bytes, int n, int h, int w, const int64_t* offsets, int64_t offsets_elems,
                            uint8_t* out, int64_t out_bytes, int32_t* err, void* stream) {
    Geometry g;
    SDT_CHECK_ARG(geometry(n, h, w, g), "need 1 <= n, h, w <= 65535, fewer than 2^31 pixels and 2^26 segments");
    SDT_CHECK_ARG(workspace != nullptr && offsets != nullptr && out != nullptr && err != nullptr, "null pointer");
    SDT_CHECK_ARG(workspace_bytes >= g.bytes, "workspace too small");
    SDT_CHECK_ARG(offsets_elems >= n + 1 + g.segs, "offset table too small");
    SDT_CHECK_ARG(out_bytes > 0 && (out_bytes & 3) == 0 && ((uintptr_t)out & 3) == 0, "the output must be whole, 4-byte aligned words");
    SDT_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)offsets & 7) == 0, "workspace must be 16-byte, offsets 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const char* ws = (const char*)workspace;
    if (hipMemsetAsync(out, 0, (size_t)out_bytes, st) != hipSuccess) {
        sdt_set_error("%s: hipMemsetAsync failed", __func__);
        return SDT_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(gif_pack_kernel, dim3((unsigned)g.segs), dim3(64), 0, st, (const uint16_t*)(ws + g.words_off),
                       (const int32_t*)(ws + g.counts_off), w, g.parts, g.step, n, h * g.parts, offsets, (uint32_t*)out, out_bytes, err);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
