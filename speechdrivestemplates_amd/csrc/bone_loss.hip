// Limb-length and limb-direction loss on the skeleton (VOICE2POSE.GENERATOR.LAMBDA_BONE / LAMBDA_BONE_DIR / BONE_MIN_LENGTH; DESIGN.md
// section 29): the next member of the family of reg_loss.hip, on the DE-NORMALISED, GLOBAL keypoints of a frame.
//
//   P[k] = double(pred[k]) * std[k] + mean[k] (per x / y);  X[k] = P[k] + (root[k] >= 0 ? P[root[k]] : 0);  Q, Y likewise from gt
//   live(k) = score_x[k] > c and score_y[k] > c and (root[k] < 0 or the same for root[k])   (score NULL: 1)
//   edge e = (a, b):  vp = X[b] - X[a], vg = Y[b] - Y[a], lp = |vp|, lg = |vg|,  m = live(a) and live(b),  md = m and lp > 0 and lg > 0
//   len = |lp - lg| / max(lg, lmin),  dir = 1 - (vp . vg) / (lp lg)
//   losses[0] = lambda_len * sum(m w len) / max(sum m, 1);   losses[1] = lambda_dir * sum(md w dir) / max(sum md, 1)
//
// Forward: one wave per frame (four frames per workgroup) stages X and Y in LDS as float64, its lanes run over the edges, a wave butterfly
// gives one float64 sum and one integer count per term and frame; then one block combines the per-frame partials in a fixed order, divides
// ON THE DEVICE and keeps the two divisors for backward.  Backward: one launch of the same frame shape; the lanes run over the keypoints and
// gather the edges incident to theirs through a CSR list (every edge is recomputed at both of its ends: no scratch buffer, no atomics),
// then the children of a part root are added into the root in ascending keypoint order.  A dead edge is SELECTED away, never multiplied
// by 0: a NaN or a huge value under the mask reaches neither a sum nor a gradient.  Two calls give the same bits.
//
// The direction gradient  -(vg / (lp lg) - (vp . vg) vp / (lp^3 lg))  is evaluated in its 2-D form  -(c / (lp^3 lg)) * (-vp_y, vp_x),
// c = vp_x vg_y - vp_y vg_x  (|vp|^2 vg - (vp . vg) vp = c * (-vp_y, vp_x) in the plane): the same number without the difference of
// two nearly equal vectors, and exactly 0 where vp == vg.  Contraction into FMAs is off in this file, so that P and Q -- the same code
// on two inputs -- cannot be rounded differently (pred == gt gives lp == lg to the bit) and a * b - b * a is exactly 0.
#include "common.h"

#pragma clang fp contract(off)

#define BONE_MAX_K 256
#define BONE_MAX_E 512
#define BONE_FRAMES 4  // frames (waves) per workgroup

namespace {

__device__ __forceinline__ unsigned long long bone_wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double bone_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }  // sign(0) = 0
__device__ __forceinline__ double bone_denorm(float v, double std, double mean) { return (double)v * std + mean; }

struct BoneFrame {
    double* xp;  // [2][K]: X (prediction), x then y
    double* xg;  // [2][K]: Y (ground truth)
    unsigned char* live;
};

// The wave's frame into LDS: every lane takes keypoints lane, lane + 64, ...  The part root is read from global memory again (three
// distinct roots in the default table: broadcast loads), through the same bone_denorm as the keypoint itself.
__device__ __forceinline__ void bone_stage(const BoneFrame& fr, const float* __restrict__ p, const float* __restrict__ g,
                                           const float* __restrict__ score, const double* __restrict__ mean, const double* __restrict__ std,
                                           const int* __restrict__ root, int K, float min_conf, int lane) {
    for (int k = lane; k < K; k += 64) {
        const int r = root[k];
        const bool has_root = (unsigned)r < (unsigned)K;
        bool lv = score == nullptr || (score[k] > min_conf && score[K + k] > min_conf);
        if (has_root && score != nullptr) lv = lv && score[r] > min_conf && score[K + r] > min_conf;
#pragma unroll
        for (int xy = 0; xy < 2; ++xy) {
            const int c = xy * K + k;
            double a = bone_denorm(p[c], std[c], mean[c]);
            double b = bone_denorm(g[c], std[c], mean[c]);
            if (has_root) {
                const int cr = xy * K + r;
                a = a + bone_denorm(p[cr], std[cr], mean[cr]);
                b = b + bone_denorm(g[cr], std[cr], mean[cr]);
            }
            fr.xp[c] = a;
            fr.xg[c] = b;
        }
        fr.live[k] = lv ? 1 : 0;
    }
}

struct BoneEdge {
    double vpx, vpy, vgx, vgy, lp, lg;
    bool m, md;
};

__device__ __forceinline__ BoneEdge bone_edge(const BoneFrame& fr, const int* __restrict__ edges, int e, int K) {
    BoneEdge o;
    const int a = edges[2 * e], b = edges[2 * e + 1];
    o.m = (unsigned)a < (unsigned)K && (unsigned)b < (unsigned)K && fr.live[a] && fr.live[b];
    o.md = false;
    if (o.m) {
        o.vpx = fr.xp[b] - fr.xp[a];
        o.vpy = fr.xp[K + b] - fr.xp[K + a];
        o.vgx = fr.xg[b] - fr.xg[a];
        o.vgy = fr.xg[K + b] - fr.xg[K + a];
        o.lp = sqrt(o.vpx * o.vpx + o.vpy * o.vpy);
        o.lg = sqrt(o.vgx * o.vgx + o.vgy * o.vgy);
        o.md = o.lp > 0.0 && o.lg > 0.0;
    }
    return o;
}

// psum: [0, BT) sums of m w len, [BT, 2 BT) sums of md w dir;  pcnt: the counts of m and md in the same layout
__global__ __launch_bounds__(64 * BONE_FRAMES) void bone_loss_partial_kernel(
    const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ score, const double* __restrict__ mean,
    const double* __restrict__ std, const int* __restrict__ edges, const double* __restrict__ edge_w, const int* __restrict__ root, int BT,
    int T, int K, int E, float min_conf, double min_len, double* __restrict__ psum, unsigned long long* __restrict__ pcnt) {
    __shared__ double s_x[BONE_FRAMES][4 * BONE_MAX_K];
    __shared__ unsigned char s_live[BONE_FRAMES][BONE_MAX_K];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.x * BONE_FRAMES + wv;
    const bool on = f < BT;
    const int C = 2 * K;
    const BoneFrame fr = {s_x[wv], s_x[wv] + C, s_live[wv]};
    if (on) {
        const int64_t row = (int64_t)f * C;
        const int64_t st = (int64_t)(f / T) * C;
        bone_stage(fr, pred + row, gt + row, score ? score + row : nullptr, mean + st, std + st, root, K, min_conf, lane);
    }
    __syncthreads();
    double s_len = 0.0, s_dir = 0.0;
    unsigned long long c_len = 0, c_dir = 0;
    if (on) {
        for (int e = lane; e < E; e += 64) {
            const BoneEdge ed = bone_edge(fr, edges, e, K);
            const double w = edge_w ? edge_w[e] : 1.0;
            if (ed.m) {
                s_len += w * (fabs(ed.lp - ed.lg) / fmax(ed.lg, min_len));
                c_len += 1u;
            }
            if (ed.md) {
                s_dir += w * (1.0 - (ed.vpx * ed.vgx + ed.vpy * ed.vgy) / (ed.lp * ed.lg));
                c_dir += 1u;
            }
        }
    }
    s_len = wave_sum_d(s_len);
    s_dir = wave_sum_d(s_dir);
    c_len = bone_wave_sum_u64(c_len);
    c_dir = bone_wave_sum_u64(c_dir);
    if (on && lane == 0) {
        psum[f] = s_len;
        psum[BT + f] = s_dir;
        pcnt[f] = c_len;
        pcnt[BT + f] = c_dir;
    }
}

// losses[q] = (float)(lambda_q * sum_q / denom_q), denom_q = max(count_q, 1): thread t takes frames t, t + 256, ... in ascending order
__global__ __launch_bounds__(256) void bone_loss_final_kernel(const double* __restrict__ psum, const unsigned long long* __restrict__ pcnt,
                                                              int BT, double lambda_len, double lambda_dir, float* __restrict__ losses,
                                                              double* __restrict__ denom) {
    __shared__ double red[2][4];
    __shared__ unsigned long long redc[2][4];
    double s[2] = {0.0, 0.0};
    unsigned long long k[2] = {0, 0};
    for (int i = threadIdx.x; i < BT; i += 256) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            s[q] += psum[(int64_t)q * BT + i];
            k[q] += pcnt[(int64_t)q * BT + i];
        }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        s[q] = wave_sum_d(s[q]);
        k[q] = bone_wave_sum_u64(k[q]);
        if ((threadIdx.x & 63) == 0) {
            red[q][threadIdx.x >> 6] = s[q];
            redc[q][threadIdx.x >> 6] = k[q];
        }
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int q = threadIdx.x;
        const double sum = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
        const unsigned long long cnt = (redc[q][0] + redc[q][1]) + (redc[q][2] + redc[q][3]);
        const double den = cnt > 0 ? (double)cnt : 1.0;
        denom[q] = den;
        losses[q] = (float)((q == 0 ? lambda_len : lambda_dir) * sum / den);
    }
}

// dX[k] = sum over the edges incident to k (CSR order = ascending edge index) of +-(cl w * dlen/dvp + cd w * ddir/dvp), + at the edge's b end
// and - at its a end, cl = (gout_len / denom[0]) * lambda_len, cd = (gout_dir / denom[1]) * lambda_dir;
// dpred[k] = (float)(std[k] * (dX[k] + sum of dX over the children of k, ascending)).
__global__ __launch_bounds__(64 * BONE_FRAMES) void bone_loss_bwd_kernel(
    const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ score, const double* __restrict__ mean,
    const double* __restrict__ std, const int* __restrict__ edges, const double* __restrict__ edge_w, const int* __restrict__ root,
    const int* __restrict__ inc_ptr, const int* __restrict__ inc_edge, const int* __restrict__ child_ptr, const int* __restrict__ child_idx,
    const float* __restrict__ gout_len, const float* __restrict__ gout_dir, const double* __restrict__ denom, int BT, int T, int K, int E,
    double lambda_len, double lambda_dir, float min_conf, double min_len, float* __restrict__ dpred) {
    __shared__ double s_x[BONE_FRAMES][4 * BONE_MAX_K];
    __shared__ double s_d[BONE_FRAMES][2 * BONE_MAX_K];
    __shared__ unsigned char s_live[BONE_FRAMES][BONE_MAX_K];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.x * BONE_FRAMES + wv;
    const bool on = f < BT;
    const int C = 2 * K;
    const BoneFrame fr = {s_x[wv], s_x[wv] + C, s_live[wv]};
    double* dX = s_d[wv];
    const int64_t row = (int64_t)f * C;
    const int64_t st = (int64_t)(f / T) * C;
    const double cl = gout_len ? (double)gout_len[0] / denom[0] * lambda_len : 0.0;
    const double cd = gout_dir ? (double)gout_dir[0] / denom[1] * lambda_dir : 0.0;
    if (on) bone_stage(fr, pred + row, gt + row, score ? score + row : nullptr, mean + st, std + st, root, K, min_conf, lane);
    __syncthreads();
    if (on) {
        for (int k = lane; k < K; k += 64) {
            double gx = 0.0, gy = 0.0;
            const int i1 = min(inc_ptr[k + 1], 2 * E);
            for (int i = max(inc_ptr[k], 0); i < i1; ++i) {
                const int ent = inc_edge[i];
                const int e = ent >> 1;
                if ((unsigned)e >= (unsigned)E) continue;
                const BoneEdge ed = bone_edge(fr, edges, e, K);
                if (!ed.m) continue;
                const double w = edge_w ? edge_w[e] : 1.0;
                double ex = 0.0, ey = 0.0;
                if (ed.lp > 0.0 && cl != 0.0) {  // the length term: exactly 0 where lp == 0 and where lp == lg
                    const double t = (cl * w) * bone_sign(ed.lp - ed.lg) / fmax(ed.lg, min_len);
                    ex = t * (ed.vpx / ed.lp);
                    ey = t * (ed.vpy / ed.lp);
                }
                if (ed.md && cd != 0.0) {
                    const double c = ed.vpx * ed.vgy - ed.vpy * ed.vgx;
                    const double q = (cd * w) * c / (ed.lp * ed.lp * ed.lp * ed.lg);
                    ex += q * ed.vpy;
                    ey -= q * ed.vpx;
                }
                if (ent & 1) {  // low bit: k is the edge's a end
                    gx -= ex;
                    gy -= ey;
                } else {
                    gx += ex;
                    gy += ey;
                }
            }
            dX[k] = gx;
            dX[K + k] = gy;
        }
    }
    __syncthreads();
    if (on) {
        for (int k = lane; k < K; k += 64) {
            double gx = dX[k], gy = dX[K + k];
            const int j1 = min(child_ptr[k + 1], K);
            for (int j = max(child_ptr[k], 0); j < j1; ++j) {
                const int ch = child_idx[j];
                if ((unsigned)ch >= (unsigned)K) continue;
                gx += dX[ch];
                gy += dX[K + ch];
            }
            dpred[row + k] = (float)(std[st + k] * gx);
            dpred[row + K + k] = (float)(std[st + K + k] * gy);
        }
    }
}

bool bone_dims_ok(int B, int T, int K, int E) {
    return B > 0 && T > 0 && K > 0 && K <= BONE_MAX_K && E >= 0 && E <= BONE_MAX_E && (int64_t)B * T <= (int64_t)1 << 30;
}

}  // namespace

extern "C" int sdt_bone_loss_fwd_f32(const float* pred, const float* gt, const float* score, const double* mean, const double* std,
                                     const int32_t* edges, const double* edge_w, const int32_t* root, int B, int T, int K, int E,
                                     double lambda_len, double lambda_dir, float min_conf, double min_len, double* psum, int64_t* pcnt,
                                     float* losses, double* denom, void* stream) {
    SDT_CHECK_ARG(pred && gt && mean && std && root && psum && pcnt && losses && denom && (edges || E == 0), "null pointer");
    SDT_CHECK_ARG(bone_dims_ok(B, T, K, E), "B, T > 0, 0 < K <= 256 and 0 <= E <= 512 are required");
    SDT_CHECK_ARG(lambda_len >= 0.0 && lambda_dir >= 0.0, "the weights must be >= 0");  // (false for NaN too)
    SDT_CHECK_ARG(min_len > 0.0, "min_len must be > 0");
    SDT_CHECK_ARG(score == nullptr || min_conf == min_conf, "min_conf is NaN");
    hipStream_t s = (hipStream_t)stream;
    const int BT = B * T;
    hipLaunchKernelGGL(bone_loss_partial_kernel, dim3(cdiv(BT, BONE_FRAMES)), dim3(64 * BONE_FRAMES), 0, s, pred, gt, score, mean, std,
                       edges, edge_w, root, BT, T, K, E, min_conf, min_len, psum, (unsigned long long*)pcnt);
    hipLaunchKernelGGL(bone_loss_final_kernel, dim3(1), dim3(256), 0, s, psum, (const unsigned long long*)pcnt, BT, lambda_len, lambda_dir,
                       losses, denom);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}

extern "C" int sdt_bone_loss_bwd_f32(const float* pred, const float* gt, const float* score, const double* mean, const double* std,
                                     const int32_t* edges, const double* edge_w, const int32_t* root, const int32_t* inc_ptr,
                                     const int32_t* inc_edge, const int32_t* child_ptr, const int32_t* child_idx, const float* gout_len,
                                     const float* gout_dir, const double* denom, int B, int T, int K, int E, double lambda_len,
                                     double lambda_dir, float min_conf, double min_len, float* dpred, void* stream) {
    SDT_CHECK_ARG(pred && gt && mean && std && root && inc_ptr && child_ptr && denom && dpred, "null pointer");
    SDT_CHECK_ARG((edges && inc_edge) || E == 0, "null edge table");
    SDT_CHECK_ARG(bone_dims_ok(B, T, K, E), "B, T > 0, 0 < K <= 256 and 0 <= E <= 512 are required");
    SDT_CHECK_ARG(lambda_len >= 0.0 && lambda_dir >= 0.0, "the weights must be >= 0");
    SDT_CHECK_ARG(min_len > 0.0, "min_len must be > 0");
    SDT_CHECK_ARG(score == nullptr || min_conf == min_conf, "min_conf is NaN");
    const int BT = B * T;
    hipLaunchKernelGGL(bone_loss_bwd_kernel, dim3(cdiv(BT, BONE_FRAMES)), dim3(64 * BONE_FRAMES), 0, (hipStream_t)stream, pred, gt, score,
                       mean, std, edges, edge_w, root, inc_ptr, inc_edge, child_ptr, child_idx, gout_len, gout_dir, denom, BT, T, K, E,
                       lambda_len, lambda_dir, min_conf, min_len, dpred);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
