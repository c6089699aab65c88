// Pose augmentation inside the train step (TRAIN.POSE_AUGMENT; include/sdt_hip.h states the layouts, DESIGN.md section 30 the contract;
// pose_augment.params_model / pose_model in Python are the same operations in the same order): a left/right mirror of the skeleton about the
// neck, a per-clip uniform scale and a per-clip in-plane rotation about the neck, applied to the de-normalised coordinates and normalised
// again with the target keypoint's own statistics.  Everything random is one block of Philox4x32-10 with the key (seed low, seed high) and the
// counter (0, purpose 2, clip index low, step low or 0), so a clip's transformation depends on (seed, step, clip) only.  No transcendental
// function runs here: the scale factors and the (cos, sin) pairs come from 256-entry float64 tables made on the host.
// Every float64 multiply, add, subtract and divide goes through sdt_exact::*_rn (no FMA).  No atomics, no scratch, no allocation.
#include "exact_lanes.h"
#include "philox.h"

using namespace sdt_exact;

namespace {

constexpr int kCols = SDT_POSE_AUGMENT_REC_COLS;
constexpr int kMaxK = 128;

struct Perm {
    uint8_t p[kMaxK];  // the mirror partner of each keypoint, validated on the host
};

struct PoseOpts {
    sdt_philox::Key key;
    uint32_t prob24;   // the mirror is on iff (w0 >> 8) < prob24
    int per_clip;      // the counter's step word is 0
    int64_t n_clips;
};

// one thread per clip: block 0 of purpose 2 -> the record's 8 words and the effective clip index
__global__ __launch_bounds__(64) void pose_aug_params_kernel(const int64_t* __restrict__ clip_index, const int64_t* __restrict__ step,
                                                             const double* __restrict__ scale_tab, const double* __restrict__ rot_tab, int B,
                                                             PoseOpts o, int64_t* __restrict__ rec, int64_t* __restrict__ eff_index) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int64_t clip = clip_index[b];
    const sdt_philox::Words p = sdt_philox::philox4x32(0u, 2u, (uint32_t)clip, o.per_clip ? 0u : (uint32_t)step[0], o.key);
    const int mirror = (p.w[0] >> 8) < o.prob24 ? 1 : 0;
    const uint32_t is = p.w[1] >> 24, ir = p.w[2] >> 24;
    const double s = scale_tab[is], c = rot_tab[2 * ir], sn = rot_tab[2 * ir + 1];
    const int64_t eff = clip + (mirror ? o.n_clips : 0);
    int64_t* r = rec + (size_t)b * kCols;
    r[0] = mirror;
    r[1] = is;
    r[2] = ir;
    r[3] = bits_of(s);
    r[4] = bits_of(c);
    r[5] = bits_of(sn);
    r[6] = eff;
    r[7] = (!mirror && s == 1.0 && c == 1.0 && sn == 0.0) ? 1 : 0;
    eff_index[b] = eff;
}

// one thread per (frame, keypoint) of the clip blockIdx.y: both coordinates of keypoint k from both coordinates of its partner m.  Consecutive
// threads write consecutive dwords of the x row and of the y row of a frame; every read is poses[b][t][.][m] with m < K.
__global__ __launch_bounds__(256) void pose_aug_kernel(const float* __restrict__ poses, const float* __restrict__ score,
                                                       const double* __restrict__ mean, const double* __restrict__ sd, int T, int K,
                                                       const int64_t* __restrict__ rec, Perm perm, float* __restrict__ out,
                                                       float* __restrict__ score_out) {
    const int b = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)T * K) return;
    const int64_t t = e / K;
    const int k = (int)(e - t * K);
    const int64_t* r = rec + (size_t)b * kCols;
    const bool mirror = r[0] != 0, identity = r[7] != 0;
    const int m = mirror ? (int)perm.p[k] : k;
    const size_t row = ((size_t)b * T + (size_t)t) * 2 * (size_t)K;  // poses[b][t][0][0]
    const uint32_t* in32 = reinterpret_cast<const uint32_t*>(poses);
    uint32_t* out32 = reinterpret_cast<uint32_t*>(out);
    if (score != nullptr) {  // permuted as bits
        const uint32_t* s32 = reinterpret_cast<const uint32_t*>(score);
        uint32_t* so32 = reinterpret_cast<uint32_t*>(score_out);
        so32[row + k] = s32[row + m];
        so32[row + K + k] = s32[row + K + m];
    }
    if (identity) {  // the input's bits: no (n s + mu - mu) / s
        out32[row + k] = in32[row + k];
        out32[row + K + k] = in32[row + K + k];
        return;
    }
    const double s = double_of(r[3]), c = double_of(r[4]), sn = double_of(r[5]);
    const double* mu = mean + (size_t)b * 2 * K;
    const double* sg = sd + (size_t)b * 2 * K;
    double dx = add_rn(mul_rn((double)poses[row + m], sg[m]), mu[m]);
    double dy = add_rn(mul_rn((double)poses[row + K + m], sg[K + m]), mu[K + m]);
    if (mirror) dx = -dx;
    double rx, ry;
    if (c == 1.0 && sn == 0.0) {  // no rotation: the coordinates stay apart (a NaN in y does not reach x)
        rx = mul_rn(s, dx);
        ry = mul_rn(s, dy);
    } else {
        rx = mul_rn(s, sub_rn(mul_rn(c, dx), mul_rn(sn, dy)));
        ry = mul_rn(s, add_rn(mul_rn(sn, dx), mul_rn(c, dy)));
    }
    out[row + k] = (float)div_rn(sub_rn(rx, mu[k]), sg[k]);
    out[row + K + k] = (float)div_rn(sub_rn(ry, mu[K + k]), sg[K + k]);
}

}  // namespace

extern "C" int sdt_pose_augment_f32(const float* poses, const float* score_or_null, const double* mean, const double* std, int B, int T, int K,
                                    const int64_t* clip_index, const int64_t* step, int64_t n_clips, uint64_t seed, int64_t mirror_prob24,
                                    int per_clip, const int32_t* perm, const double* scale_table, const double* rot_table, float* poses_out,
                                    float* score_out, int64_t* eff_index, void* rec, void* stream) {
    SDT_CHECK_SUPPORTED(K >= 1 && K <= kMaxK, "K outside [1, 128]");
    SDT_CHECK_SUPPORTED(B >= 1 && B <= 65535, "B outside [1, 65535]");
    SDT_CHECK_SUPPORTED(T >= 1 && T <= (1 << 24), "T outside [1, 2^24]");
    SDT_CHECK_SUPPORTED(n_clips >= 1 && n_clips <= ((int64_t)1 << 40), "n_clips outside [1, 2^40]");
    SDT_CHECK_ARG(poses && mean && std && clip_index && step && perm && scale_table && rot_table && poses_out && eff_index && rec, "null pointer");
    SDT_CHECK_ARG(score_or_null == nullptr || score_out != nullptr, "a score needs score_out");
    SDT_CHECK_ARG(poses != poses_out, "the pose pass never runs in place");
    SDT_CHECK_ARG(score_or_null == nullptr || score_or_null != score_out, "the pose pass never runs in place");
    SDT_CHECK_ARG(mirror_prob24 >= 0 && mirror_prob24 <= (1 << 24), "mirror probability outside [0, 2^24]");
    SDT_CHECK_ARG(per_clip == 0 || per_clip == 1, "per_clip is 0 or 1");
    Perm pm;
    bool seen[kMaxK] = {};
    for (int k = 0; k < kMaxK; ++k) pm.p[k] = 0;
    for (int k = 0; k < K; ++k) {
        SDT_CHECK_ARG(perm[k] >= 0 && perm[k] < K && !seen[perm[k]], "perm is not a permutation of 0 .. K - 1");
        seen[perm[k]] = true;
        pm.p[k] = (uint8_t)perm[k];
    }
    const PoseOpts o = {{(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)}, (uint32_t)mirror_prob24, per_clip, n_clips};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pose_aug_params_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, s, clip_index, step, scale_table, rot_table, B, o,
                       (int64_t*)rec, eff_index);
    const unsigned blocks = (unsigned)cdiv64((int64_t)T * K, 256);
    hipLaunchKernelGGL(pose_aug_kernel, dim3(blocks, (unsigned)B), dim3(256), 0, s, poses, score_or_null, mean, std, T, K, (const int64_t*)rec, pm,
                       poses_out, score_out);
    SDT_LAUNCH_CHECK();
    return SDT_OK;
}
