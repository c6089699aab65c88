// Skeleton rendering: pose videos and long images (core/utils/keypoint_visualization.py:8-110,177-207).
// Two launches.  sdt_render_prepare_kernel turns float64 poses into one 64-byte stroke record per (instance, edge):
// the reference's integer endpoints, colour and thickness, a bounding box clipped to the instance's window and the
// segment clipped near that window.  sdt_render_raster_kernel gives each workgroup a 64x16 pixel tile of one image,
// culls the image's strokes against the tile in draw order (wave64 ballot + prefix count, compacted into LDS) and
// blends the survivors pixel by pixel; tiles that no stroke reaches write background with 16-byte stores.
// Contract and numbers: DESIGN.md section 10.
#include "common.h"

namespace {

constexpr int kTileW = 64, kTileH = 16, kThreads = 256, kRecordWords = 16;
constexpr double kMaxCoord = 16777216.0;  // 2^24
constexpr int kFaceEdges = 63, kHandEdges = 20;

// 68-point face chains (open / closed) of draw_body_parts' face edge list, in list order
struct Chain {
    int a, b, closed;
};
__constant__ Chain kFaceChains[9] = {{0, 16, 0}, {17, 21, 0}, {22, 26, 0}, {27, 30, 0}, {31, 35, 0},
                                     {36, 41, 1}, {42, 47, 1}, {48, 59, 1}, {60, 67, 1}};
__constant__ int kPose121[5][2] = {{1, 4}, {1, 2}, {2, 3}, {4, 5}, {5, 6}};
__constant__ int kPose135[6][2] = {{0, 1}, {0, 4}, {1, 2}, {4, 5}, {2, 3}, {5, 6}};
__constant__ int kPose137[6][2] = {{1, 2}, {1, 5}, {2, 3}, {3, 4}, {5, 6}, {6, 7}};
// cv2's Scalar -> uint8 conversion (round to nearest, saturate) of the green level 255/8*(f+3) of finger f
__constant__ int kFingerG[5] = {96, 128, 159, 191, 223};

inline bool k_supported(int K) { return K == 121 || K == 135 || K == 137; }
inline int n_edges(int K) { return (K == 121 ? 5 : 6) + kFaceEdges + 2 * kHandEdges; }

// edge e of the skeleton of K keypoints -> keypoint indices a, b, thickness, colour (B | G<<8 | R<<16)
__device__ void edge_of(int K, int e, int& a, int& b, int& thick, int& bgr) {
    const int npe = K == 121 ? 5 : 6;
    const int num_pose = K == 121 ? 9 : (K == 135 ? 23 : 25);
    if (e < npe) {
        const int(*t)[2] = K == 121 ? kPose121 : (K == 135 ? kPose135 : kPose137);
        a = t[e][0];
        b = t[e][1];
        thick = 4;
        bgr = 25 | (175 << 8) | (25 << 16);
        return;
    }
    e -= npe;
    if (e < kFaceEdges) {
        int c = 0;
        for (; c < 8; ++c) {
            const int n = kFaceChains[c].b - kFaceChains[c].a + kFaceChains[c].closed;
            if (e < n) break;
            e -= n;
        }
        a = kFaceChains[c].a + e;
        b = a == kFaceChains[c].b ? kFaceChains[c].a : a + 1;
        a += num_pose;
        b += num_pose;
        thick = 2;
        bgr = 100 | (100 << 8) | (100 << 16);
        return;
    }
    e -= kFaceEdges;
    const int hand = e / kHandEdges, he = e % kHandEdges, f = he / 4, s = he % 4;
    const int base = num_pose + 70 + 21 * hand;
    a = base + (s == 0 ? 0 : 4 * f + s);
    b = base + 4 * f + s + 1;
    thick = 3;
    bgr = 255 | (kFingerG[f] << 8);
}

// Liang-Barsky clip of the segment p0 + t*(p1-p0), t in [0,1], to [xl,xh] x [yl,yh]; false if nothing is left
__device__ bool clip_segment(double& x0, double& y0, double& x1, double& y1, double xl, double xh, double yl, double yh) {
    const double dx = x1 - x0, dy = y1 - y0;
    double t0 = 0.0, t1 = 1.0;
    const double p[4] = {-dx, dx, -dy, dy}, q[4] = {x0 - xl, xh - x0, y0 - yl, yh - y0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (p[i] == 0.0) {
            if (q[i] < 0.0) return false;
        } else {
            const double r = q[i] / p[i];
            if (p[i] < 0.0) {
                if (r > t1) return false;
                if (r > t0) t0 = r;
            } else {
                if (r < t0) return false;
                if (r < t1) t1 = r;
            }
        }
    }
    const double ax = x0 + t0 * dx, ay = y0 + t0 * dy;
    x1 = x0 + t1 * dx;
    y1 = y0 + t1 * dy;
    x0 = ax;
    y0 = ay;
    return true;
}

__device__ __forceinline__ double endpoint(double p, double scale, double off) {
    return __dadd_rn(__dmul_rn(p, scale), off);  // the reference's two numpy operations, each rounded: no contraction into an FMA
}

}  // namespace

__global__ __launch_bounds__(256) void sdt_render_prepare_kernel(const double* __restrict__ poses, int64_t n_poses, int K,
                                                                 const sdt_render_instance* __restrict__ inst, int64_t n_inst_total,
                                                                 int E, int H, int W, int32_t* __restrict__ rec,
                                                                 int32_t* __restrict__ skipped) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_inst_total * E) return;
    const int64_t ii = g / E;
    const int e = (int)(g % E);
    int a, b, thick, bgr;
    edge_of(K, e, a, b, thick, bgr);
    const sdt_render_instance in = inst[ii];
    const int cx0 = max(in.clip_x0, 0), cx1 = min(in.clip_x1, W);  // exclusive upper bound
    bool ok = in.pose >= 0 && in.pose < n_poses;
    double xa = 0.0, ya = 0.0, xb = 0.0, yb = 0.0;
    if (ok) {
        const double* p = poses + in.pose * 2 * K;
        xa = endpoint(p[a], in.scale, in.off_x);
        ya = endpoint(p[K + a], in.scale, in.off_y);
        xb = endpoint(p[b], in.scale, in.off_x);
        yb = endpoint(p[K + b], in.scale, in.off_y);
        ok = fabs(xa) <= kMaxCoord && fabs(ya) <= kMaxCoord && fabs(xb) <= kMaxCoord && fabs(yb) <= kMaxCoord;  // false for NaN too
    }
    int ix0 = 0, iy0 = 0, ix1 = 0, iy1 = 0;
    int bx0 = 1, by0 = 1, bx1 = 0, by1 = 0;  // empty
    float f0x = 0.f, f0y = 0.f, f1x = 0.f, f1y = 0.f;
    if (ok) {
        ix0 = (int)xa + in.shift_x;  // the conversion truncates toward zero, like Python's int()
        iy0 = (int)ya;
        ix1 = (int)xb + in.shift_x;
        iy1 = (int)yb;
        const int grow = thick / 2 + 1;  // every pixel with coverage > 0 lies closer than r + 0.5 <= grow to the segment
        const int lx = max(min(ix0, ix1) - grow, cx0), hx = min(max(ix0, ix1) + grow, cx1 - 1);
        const int ly = max(min(iy0, iy1) - grow, 0), hy = min(max(iy0, iy1) + grow, H - 1);
        double sx0 = ix0, sy0 = iy0, sx1 = ix1, sy1 = iy1;
        // clipping the segment to the window grown by `grow` changes no coverage inside the window and keeps the raster
        // pass's fp32 coordinates small
        if (lx <= hx && ly <= hy &&
            clip_segment(sx0, sy0, sx1, sy1, (double)(cx0 - grow), (double)(cx1 - 1 + grow), (double)-grow, (double)(H - 1 + grow))) {
            bx0 = lx;
            by0 = ly;
            bx1 = hx;
            by1 = hy;
            f0x = (float)sx0;
            f0y = (float)sy0;
            f1x = (float)sx1;
            f1y = (float)sy1;
        }
    } else if (skipped != nullptr) {
        atomicAdd(skipped, 1);
    }
    int4* r4 = reinterpret_cast<int4*>(rec + g * kRecordWords);
    r4[0] = make_int4(ix0, iy0, ix1, iy1);
    r4[1] = make_int4(bx0, by0, bx1, by1);
    r4[2] = make_int4(__float_as_int(f0x), __float_as_int(f0y), __float_as_int(f1x), __float_as_int(f1y));
    r4[3] = make_int4(bgr | (thick << 24), in.clip_x0, in.clip_x1, ok ? 1 : 0);
}

__global__ __launch_bounds__(kThreads) void sdt_render_raster_kernel(const int32_t* __restrict__ rec, int S, int H, int W,
                                                                     uint8_t* __restrict__ out) {
    __shared__ float4 s_seg[kThreads];  // a.x, a.y, u.x, u.y (u = b - a)
    __shared__ float2 s_par[kThreads];  // 1/|u|^2 (0 for a point), r + 0.5
    __shared__ int4 s_box[kThreads];
    __shared__ int s_col[kThreads];
    __shared__ int s_wcount[kThreads / 64];
    const int img = blockIdx.z;
    const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
    const int tx1 = min(tx0 + kTileW, W) - 1, ty1 = min(ty0 + kTileH, H) - 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int py = ty0 + (tid >> 4), px0 = tx0 + (tid & 15) * 4;  // a lane owns 4 neighbouring pixels of one row
    const int4* strokes = reinterpret_cast<const int4*>(rec) + (int64_t)img * S * (kRecordWords / 4);
    int val[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) val[q][0] = val[q][1] = val[q][2] = 255;
    bool any = false;
    for (int base = 0; base < S; base += kThreads) {
        const int s = base + tid;
        bool hit = false;
        int4 box = make_int4(1, 1, 0, 0), seg = make_int4(0, 0, 0, 0), misc = make_int4(0, 0, 0, 0);
        if (s < S) {
            const int4* st = strokes + (int64_t)s * (kRecordWords / 4);
            box = st[1];
            hit = box.x <= box.z && box.y <= box.w && box.x <= tx1 && box.z >= tx0 && box.y <= ty1 && box.w >= ty0;
            if (hit) {
                seg = st[2];
                misc = st[3];
            }
        }
        const uint64_t m = __ballot(hit);
        const int pre = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_wcount[wave] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            off += w < wave ? s_wcount[w] : 0;
            total += s_wcount[w];
        }
        if (hit) {
            const int slot = off + pre;  // draw order kept: waves in order, lanes in order within a wave
            const float ax = __int_as_float(seg.x), ay = __int_as_float(seg.y);
            const float ux = __int_as_float(seg.z) - ax, uy = __int_as_float(seg.w) - ay;
            const float l2 = ux * ux + uy * uy;
            s_seg[slot] = make_float4(ax, ay, ux, uy);
            s_par[slot] = make_float2(l2 > 1e-12f ? 1.f / l2 : 0.f, 0.5f * (float)((misc.x >> 24) & 0xff) + 0.5f);
            s_box[slot] = box;
            s_col[slot] = misc.x & 0xffffff;
        }
        __syncthreads();
        for (int j = 0; j < total; ++j) {
            const int4 bb = s_box[j];
            if (py < bb.y || py > bb.w || px0 + 3 < bb.x || px0 > bb.z) continue;
            const float4 sg = s_seg[j];
            const float2 pr = s_par[j];
            const int col = s_col[j];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int px = px0 + q;
                if (px < bb.x || px > bb.z) continue;
                const float wx = (float)px - sg.x, wy = (float)py - sg.y;
                const float t = fminf(fmaxf((wx * sg.z + wy * sg.w) * pr.x, 0.f), 1.f);
                const float dx = wx - t * sg.z, dy = wy - t * sg.w;
                const float c = fminf(pr.y - sqrtf(dx * dx + dy * dy), 1.f);
                if (c <= 0.f) continue;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float bg = (float)val[q][ch], fg = (float)((col >> (8 * ch)) & 0xff);
                    val[q][ch] = (int)floorf(bg + c * (fg - bg) + 0.5f);  // uint8 after every stroke, like cv2.line
                }
            }
        }
        any = any || total > 0;  // uniform over the workgroup
        __syncthreads();         // the next chunk overwrites the LDS lists
    }
    uint8_t* img_out = out + (int64_t)img * H * W * 3;
    if (!any && (W * 3) % 16 == 0 && tx0 + kTileW <= W) {
        // background tile: 16 rows x 192 bytes = 192 aligned 16-byte stores
        if (tid < kTileH * 12) {
            const int y = ty0 + tid / 12;
            if (y < H)
                *reinterpret_cast<uint4*>(img_out + ((int64_t)y * W + tx0) * 3 + (tid % 12) * 16) =
                    make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
        }
        return;
    }
    if (py >= H) return;
    uint8_t* row = img_out + ((int64_t)py * W + px0) * 3;
    if ((W & 3) == 0 && px0 + 3 < W) {
        // 4 pixels = 12 bytes at a pixel index that is a multiple of 4, so 4-byte aligned: three dword stores
        uint32_t* o = reinterpret_cast<uint32_t*>(row);
        o[0] = (uint32_t)val[0][0] | ((uint32_t)val[0][1] << 8) | ((uint32_t)val[0][2] << 16) | ((uint32_t)val[1][0] << 24);
        o[1] = (uint32_t)val[1][1] | ((uint32_t)val[1][2] << 8) | ((uint32_t)val[2][0] << 16) | ((uint32_t)val[2][1] << 24);
        o[2] = (uint32_t)val[2][2] | ((uint32_t)val[3][0] << 8) | ((uint32_t)val[3][1] << 16) | ((uint32_t)val[3][2] << 24);
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (px0 + q < W)
            for (int ch = 0; ch < 3; ++ch) row[q * 3 + ch] = (uint8_t)val[q][ch];
}

extern "C" int sdt_render_edges(int K) { return k_supported(K) ? n_edges(K) : 0; }

extern "C" int64_t sdt_render_workspace_bytes(int n_images, int n_inst, int K) {
    if (n_images <= 0 || n_inst <= 0 || !k_supported(K)) return 0;
    return (int64_t)n_images * n_inst * n_edges(K) * kRecordWords * 4;
}

extern "C" int sdt_render_prepare_f64(const double* poses, int64_t n_poses, int K, const sdt_render_instance* inst, int n_images,
                                      int n_inst, int H, int W, void* workspace, int64_t workspace_bytes, int32_t* skipped,
                                      void* stream) {
    SDT_CHECK_ARG(k_supported(K), "K must be 121, 135 or 137 (draw_body_parts' skeletons)");
    SDT_CHECK_ARG(poses != nullptr && inst != nullptr && workspace != nullptr && n_poses > 0, "null pointer or no poses");
    SDT_CHECK_ARG(n_images > 0 && n_inst > 0 && H > 0 && W > 0 && H <= 65535 * kTileH && W <= (1 << 24), "bad image geometry");
    SDT_CHECK_ARG(workspace_bytes >= sdt_render_workspace_bytes(n_images, n_inst, K), "workspace too small");
    SDT_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (skipped != nullptr && hipMemsetAsync(skipped, 0, sizeof(int32_t), st) != hipSuccess) {
        sdt_set_error("%s: hipMemsetAsync failed", __func__);
        return SDT_ERR_LAUNCH;
    }
    const int64_t total = (int64_t)n_images * n_inst * n_edges(K);
    hipLaunchKernelGGL(sdt_render_prepare_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, poses, n_poses, K, inst,
                       (int64_t)n_images * n_inst, n_edges(K), H, W, (int32_t*)workspace, skipped);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_render_skeleton_u8(const void* workspace, int64_t workspace_bytes, int n_images, int n_inst, int K, int H, int W,
                                      uint8_t* out, int64_t out_bytes, void* stream) {
    SDT_CHECK_ARG(k_supported(K), "K must be 121, 135 or 137 (draw_body_parts' skeletons)");
    SDT_CHECK_ARG(workspace != nullptr && out != nullptr, "null pointer");
    SDT_CHECK_ARG(n_images > 0 && n_images <= 65535 && n_inst > 0 && H > 0 && W > 0 && H <= 65535 * kTileH && W <= (1 << 24),
                  "bad image geometry");
    SDT_CHECK_ARG(workspace_bytes >= sdt_render_workspace_bytes(n_images, n_inst, K), "workspace too small");
    SDT_CHECK_ARG(out_bytes >= (int64_t)n_images * H * W * 3, "output buffer too small");
    SDT_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out & 15) == 0, "workspace and output must be 16-byte aligned");
    const int S = n_inst * n_edges(K);
    hipLaunchKernelGGL(sdt_render_raster_kernel, dim3(cdiv(W, kTileW), cdiv(H, kTileH), n_images), dim3(kThreads), 0,
                       (hipStream_t)stream, (const int32_t*)workspace, S, H, W, out);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
