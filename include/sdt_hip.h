/*
 * sdt_hip.h -- C ABI of libsdt_hip.so: the MI355X (gfx950) kernels behind the SDT voice2pose
 * training hot path.  Plain pointers + sizes + a hipStream_t (passed as void*); no torch types.
 *
 * All activation tensors are CHANNELS-LAST fp32 in HBM:
 *     2-D stage  (B, H, W, C)      1-D stage (B, T, C)  == (B, 1, T, C)
 * Conv weights are (Cout, taps, Cin) with Cin contiguous (taps = kh*kw, row-major).  The host
 * mirror keeps the reference's logical shapes (Cout,Cin,kh,kw)/(Cout,Cin,k) as strided views of
 * that storage, so reference checkpoints load unchanged.
 *
 * Every entry point: allocates nothing, launches on the caller's stream, returns 0 on success or
 * a negative sdt_status; sdt_last_error() gives the message.  Each comment names the reference
 * operator (file:line in ShenhanQian/SpeechDrivesTemplates) the entry point replaces.
 */
#ifndef SDT_HIP_H
#define SDT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDT_MAX_TAPS 20
/* What sdt_abi_version() of a library built from this header returns: a consumer compares the two to catch a stale .so */
#define SDT_ABI_VERSION 5

enum sdt_status { SDT_OK = 0, SDT_ERR_ARG = -1, SDT_ERR_LAUNCH = -2, SDT_ERR_UNSUPPORTED = -3 };
/* Element type of a tensor argument of the *_t / *_bf16 entry points (the bf16-storage path of BASELINE config 4: activations of the
 * Conv2d chain and the conv operands' weight copies live in HBM as bf16, statistics / accumulation / master weights / gradients fp32) */
enum sdt_dtype { SDT_F32 = 0, SDT_BF16 = 1 };

const char* sdt_last_error(void);
int sdt_abi_version(void);

/*
 * Tap-table convolution geometry (implicit GEMM):
 *   Y[b, oy*osy+ooy, ox*osx+oox, n] = bias[n] +
 *       sum_{t<ntaps} sum_{c<Cin} X[b, oy*sy+dy[t], ox*sx+dx[t], c] * W[n, wt[t], c]
 * for (b,oy,ox) in B x Ho x Wo; out-of-range X reads are 0.  X is (B,Hi,Wi,Cin), Y is
 * (B,Hy,Wy,Cout), W is (Cout,Tw,Cin).  One geometry describes a forward conv (any stride), and --
 * with transposed weights and flipped taps -- the input-gradient of a stride-1 conv or one output
 * parity class of a strided conv.
 */
typedef struct sdt_conv_geom {
    int32_t B, Hi, Wi, Cin;
    int32_t Ho, Wo;
    int32_t Hy, Wy, Cout;
    int32_t sy, sx;
    int32_t osy, osx, ooy, oox;
    int32_t ntaps, Tw;
    int32_t dy[SDT_MAX_TAPS], dx[SDT_MAX_TAPS], wt[SDT_MAX_TAPS];
} sdt_conv_geom;

/* nn.Conv2d / nn.Conv1d forward and input-gradient (building_blocks.py:15-22,31-38; ATen conv). */
int sdt_conv_taps_f32(const float* x, const float* w, const float* bias, float* y,
                      const sdt_conv_geom* g, void* stream);
/* The same forward conv with the statistics pass of the normalisation that follows fused into its epilogue:
 * stats[(g * Cout + n) * 2 + {0,1}] += sum / sum of squares of Y[., n] over the output rows m (= (b*Ho+oy)*Wo+ox) with
 * m / rows_per_group == g (InstanceNorm2d: rows_per_group = Ho*Wo; BatchNorm: B*Ho*Wo).  stats must be zero on entry.
 * sdt_conv_taps_stats_supported: 1 if the geometry qualifies (dense output, Cin % 32 == 0, no split-K, fp32 math). */
int sdt_conv_taps_stats_supported(const sdt_conv_geom* g, int rows_per_group);
int sdt_conv_taps_stats_f32(const float* x, const float* w, const float* bias, float* y, const sdt_conv_geom* g,
                            double* stats, int rows_per_group, void* stream);
/* Split-K form for launches with too few output tiles to fill the chip (the 1-D stage): slice z of `splitk`
 * writes its partial sums to partial + z*numel(Y) (no bias); after ALL launches that share the Y tensor (the parity
 * classes of an input-gradient) sdt_splitk_reduce_f32 sums the slabs in a fixed order (deterministic) and adds bias.
 * splitk == 1 is sdt_conv_taps_f32.  sdt_conv_taps_splitk_hint returns a suitable slice count for a geometry. */
int sdt_conv_taps_splitk_hint(const sdt_conv_geom* g);
int sdt_conv_taps_splitk_f32(const float* x, const float* w, const float* bias, float* y,
                             const sdt_conv_geom* g, int splitk, float* partial, void* stream);
int sdt_splitk_reduce_f32(const float* partial, const float* bias, float* y, int64_t n, int cout, int splitk, void* stream);
/* Input gradient of a strided convolution in ONE launch: `ncls` (1..4) output parity classes -- geometries that share X (= dY),
 * W (= transposed weights) and the Y (= dX) tensor and write disjoint output positions (ATen's conv backward-data,
 * building_blocks.py:15-22,31-38).  Same split-K contract as sdt_conv_taps_splitk_f32.
 * nb != NULL (fp32 math, splitk == 1, Cin % 32 == 0): the epilogue also accumulates the per-(group, channel) sums the backward
 * of the InstanceNorm2d / BatchNorm + LeakyReLU that produced this conv's input needs (building_blocks.py:24-26,46), so that
 * sdt_colnorm_bwd_f32(stats_ready = 1) skips its statistics pass over dz and y:
 *   sums[(grp*C + n)*2 + 0] += sum gg,  [..+1] += sum gg*yhat,  gg = dX * act'(gamma*yhat + beta), yhat = (y - mean)*rstd
 * y = raw output of the conv below (same shape as dX), grp = batch item (groups == B) or 0 (groups == 1); sums zero on entry. */
typedef struct sdt_norm_bwd {
    const void* y;      /* element type of the launch's x (fp32; bf16 for sdt_convsk_bf16) */
    const float* mean;  /* [groups*C] */
    const float* rstd;  /* [groups*C] */
    const float* gamma; /* [C] or NULL */
    const float* beta;  /* [C] or NULL */
    double* sums;       /* [groups*C*2] */
    float slope;
    int32_t groups;
} sdt_norm_bwd;
int sdt_conv_taps_multi_f32(const float* x, const float* w, float* y, const sdt_conv_geom* geoms, int ncls, int splitk,
                            float* partial, const sdt_norm_bwd* nb, void* stream);
/*
 * Persistent stream-K form of the same convolution (csrc/convsk.hip; round 3) for the MFMA-bound Conv2d launches of the audio
 * encoder (generator.py:15-30 through building_blocks.py:15-22): forward (ncls = 1) or input gradient (ncls parity classes) with
 * Cin % 32 == 0 and Cout % 64 == 0.  One or two resident workgroups per CU each walk a contiguous range of the launch's (tile, live K step) list, so every
 * CU gets the same number of K steps whatever the tile count; tiles that straddle two ranges are combined in a fixed order
 * (bit-identical from run to run).  128x128x32 or 128x64x32 tiles, software-pipelined, fp32 accumulation in chunks of 256 products.
 *   sdt_convsk_supported     1 if the geometry pack qualifies
 *   sdt_convsk_plan_bytes    size of the PLAN of a geometry pack: per GEMM row {X byte offset, mask of the taps outside X, Y byte offset,
 *                            statistics group} (the row ORDER is the plan's choice: image-row-major where that culls >= 5 % of the K
 *                            steps), per m-tile {live-tap mask, tap rotation}, prefix sums of live K steps, first tile of
 *                            each workgroup's range.  Built on the host once per geometry (sdt_convsk_plan_build), kept by the caller
 *                            in host AND device memory and handed to every launch
 *   rows_per_group > 0       statistics group of output row m = m / rows_per_group (forward statistics, as sdt_conv_taps_stats_f32);
 *   rows_per_group <= 0      group = batch item (bwd_groups == B) or 0 (bwd_groups == 1) (backward statistics, as sdt_norm_bwd)
 *   sdt_convsk_workspace_bytes  partial-tile slabs + flags: one buffer per stream, ZERO-FILLED ONCE by the caller, then passed to every
 *                            launch on that stream.  epoch >= 1 is the flag value of the launch; the workgroup that consumes a flag lowers it
 *                            again, so every flag is zero between launches and the same epoch may be passed every time (a launch recorded
 *                            into a hipGraph replays correctly).  The word after the flags is an error code: non-zero = the owner of a
 *                            split tile gave up waiting for a partner (sdt_convsk_set_spin_limit polls: the partner was never dispatched,
 *                            e.g. another process holds its slot); that tile is stored as NaN, never with a partial sum missing, and the
 *                            host mirror raises when it sees the word (core/pipelines/trainer.py)
 *   sdt_convsk_f32           the launch; stats / nb as in sdt_conv_taps_stats_f32 / sdt_conv_taps_multi_f32 (at most one of them);
 *                            xbytes / wbytes / ybytes: sizes of the X, W and Y tensors
 */
/*   sdt_convsk_f32_w3        the same launch for a split-fp32 plan (sdt_convsk_set_f32_split) with the weights ALREADY split: w3 = three bf16 planes
 *                            [hi | mid | lo] of the (N, Tw, Cin) weight tensor (sdt_wt_desc.planes = 3 makes them); wbytes = the fp32 tensor's size.
 *                            Bit-identical results to sdt_convsk_f32 on the fp32 weights (the same split, made once per optimiser step instead of in
 *                            every tile on every K step).  ABI 5. */
int sdt_convsk_supported(const sdt_conv_geom* geoms, int ncls);
int sdt_convsk_grid(void);
int sdt_convsk_set_wg_per_cu(int n); /* 1 or 2 persistent workgroups per CU for plans built afterwards (default 2) */
/* fp32 plans built afterwards with ONE workgroup per CU: the split-fp32 form of the 8-wave kernel (csrc/convbf.hip: each fp32 operand = three bf16
 * planes made by the loader, six bf16 MFMAs per fragment pair -- products exact to 2^-23, fp32 accumulation).  Default 0. */
int sdt_convsk_set_f32_split(int on);
/* Workgroup slots (of the GPU's 512 two-per-CU slots; multiple of 8, <= 256 = half of the GPU) that plans built afterwards leave free: a persistent
 * launch that fills the GPU cannot share it with another long-lived kernel (a collective's); data-parallel runs plan their backward launches with a
 * reserve.  A one-per-CU workgroup (the 8-wave kernels) counts as two slots.  Default 0. */
int sdt_convsk_set_reserved_slots(int n);
/* K order of the 8-wave kernels' tiles for launches made afterwards (a launch-time setting, not a plan property): 0 = tap-major (all 128-byte channel
 * chunks of a tap, then the next tap), 1 = chunk-major (all live taps of a chunk, then the next chunk: neighbouring taps re-read the cache lines of
 * the step before while the CU's vector L1 still holds them).  ABI 5. */
int sdt_convsk_set_k_order(int order);
/* Split-fp32 weight-gradient plans built afterwards (sdt_convsk_dw_plan_build_t with sdt_convsk_set_f32_split(1)): 1 = 128-wide column tiles with a
 * ragged last one when taps * Cin = 64 (mod 128); 0 (default) = tiles by divisibility, the rule of rounds 3-5.  ABI 5. */
int sdt_convsk_set_dw_wide_tiles(int on);
int sdt_convsk_f32_w3(const float* x, const void* w3, const float* bias, float* y, const void* plan_host, const void* plan_dev, void* workspace,
                      unsigned epoch, double* stats, const sdt_norm_bwd* nbw, int64_t xbytes, int64_t wbytes, int64_t ybytes, void* stream);
/* Polls (each ~1 us under load) of a partner's flag before the owner of a split tile declares the launch failed.  Default 1 << 22. */
int sdt_convsk_set_spin_limit(unsigned polls);
unsigned sdt_convsk_get_spin_limit(void);
int64_t sdt_convsk_plan_bytes(const sdt_conv_geom* geoms, int ncls);
int64_t sdt_convsk_workspace_bytes(void);
int sdt_convsk_plan_build(const sdt_conv_geom* geoms, int ncls, int rows_per_group, int bwd_groups, void* out, int64_t out_bytes);
/* The same for a given element type of x / w (x_dtype) and of y (y_dtype): the plan's byte offsets and its K step (128 bytes of an input
 * row: 32 fp32 or 64 bf16 channels) depend on them.  bf16 needs Cin % 64 == 0. */
int sdt_convsk_supported_t(const sdt_conv_geom* geoms, int ncls, int x_dtype);
int64_t sdt_convsk_plan_bytes_t(const sdt_conv_geom* geoms, int ncls, int x_dtype);
int sdt_convsk_plan_build_t(const sdt_conv_geom* geoms, int ncls, int rows_per_group, int bwd_groups, int x_dtype, int y_dtype, void* out,
                            int64_t out_bytes);
/* Weight gradient of a forward geometry on the same persistent machinery (dense dY, Cout % 64 == 0, Cin % 64 == 0; 128- or 64-wide tiles):
 * the reduction over the output positions is split over the workgroups, partial tiles go to slabs of `workspace`
 * (sdt_convsk_dw_workspace_bytes() bytes, contents irrelevant) and a second kernel adds them to dw (Cout, Tw, Cin) in a fixed order:
 * no atomics, bit-identical from run to run (what the reference asks of cuDNN with cudnn.deterministic = True, main.py:37-38).
 * ACCUMULATES into dw like sdt_conv_dw_f32.  Plan: sdt_convsk_dw_plan_bytes / _build, host + device copy as above. */
int sdt_convsk_dw_supported(const sdt_conv_geom* g);
int64_t sdt_convsk_dw_plan_bytes(const sdt_conv_geom* g);
int64_t sdt_convsk_dw_workspace_bytes(void);
int sdt_convsk_dw_plan_build(const sdt_conv_geom* g, void* out, int64_t out_bytes);
int sdt_convsk_dw_f32(const float* x, const float* dy, float* dw, const void* plan_host, const void* plan_dev, void* workspace,
                      int64_t xbytes, int64_t ybytes, void* stream);
int sdt_convsk_f32(const float* x, const float* w, const float* bias, float* y, const void* plan_host, const void* plan_dev,
                   void* workspace, unsigned epoch, double* stats, const sdt_norm_bwd* nb, int64_t xbytes, int64_t wbytes, int64_t ybytes,
                   void* stream);
/* bf16-storage path: x, w, y and nb->y are bf16 tensors (plan from sdt_convsk_plan_build_t(.., SDT_BF16, SDT_BF16, ..)); products on
 * v_mfma_f32_32x32x16_bf16 (16x the fp32 MFMA rate), fp32 accumulation, bias and statistics (taken from the fp32 accumulators before the
 * output is rounded).  sdt_convsk_dw_bf16: bf16 x / dy, fp32 gradient accumulated into dw; 64 output positions per K step, operands
 * transposed on the way out of LDS by ds_read_b64_tr_b16. */
int sdt_convsk_bf16(const void* x, const void* w, const float* bias, void* y, const void* plan_host, const void* plan_dev,
                    void* workspace, unsigned epoch, double* stats, const sdt_norm_bwd* nb, int64_t xbytes, int64_t wbytes, int64_t ybytes,
                    void* stream);
int sdt_convsk_dw_supported_t(const sdt_conv_geom* g, int dtype);
int64_t sdt_convsk_dw_plan_bytes_t(const sdt_conv_geom* g, int dtype);
int sdt_convsk_dw_plan_build_t(const sdt_conv_geom* g, int dtype, void* out, int64_t out_bytes);
int sdt_convsk_dw_bf16(const void* x, const void* dy, float* dw, const void* plan_host, const void* plan_dev, void* workspace,
                       int64_t xbytes, int64_t ybytes, void* stream);
/* Weight gradient, ACCUMULATED into dw (Cout,Tw,Cin):
 *   dw[n, wt[t], c] += sum_{b,oy,ox} dY[b, oy*osy+ooy, ox*osx+oox, n] * X[b, oy*sy+dy[t], ox*sx+dx[t], c] */
int sdt_conv_dw_f32(const float* x, const float* dy, float* dw, const sdt_conv_geom* g, void* stream);
/* The same weight gradient without atomics: every row range of the split reduction stores its partial product into its own slab of
 * `workspace` (>= sdt_conv_dw_workspace_bytes(g) bytes, 16-byte aligned) and the slabs are added to dw in a fixed order, so the
 * result is bit-identical from run to run (torch.use_deterministic_algorithms territory; the reference's cuDNN weight gradient
 * is not deterministic either, core/pipelines/trainer.py never asks for it).  fp32 MFMA only. */
int64_t sdt_conv_dw_workspace_bytes(const sdt_conv_geom* g);
int sdt_conv_dw_det_f32(const float* x, const float* dy, float* dw, const sdt_conv_geom* g, void* workspace, int64_t workspace_bytes,
                        void* stream);
/* Which kernel instantiation the two entry points above pick for a geometry (16-B aligned operands assumed):
 * (BM*1000+BN)*10 + vec4, e.g. 1281281 = conv_taps_kernel<128,128,true>.  Used by bench.py to attribute timings. */
int sdt_conv_taps_variant(const sdt_conv_geom* g);
/* 1 when sdt_conv_taps_f32 / _splitk_f32 / _multi_f32 on these classes with this K split run the 1-D stage's small-K kernel
 * (conv1d_small_kernel: Hi = 1, Cin % 32 == 0, Cout % 64 == 0, <= 8 K steps per workgroup, exact fp32, no statistics epilogue) */
int sdt_conv1d_small_used(const sdt_conv_geom* geoms, int ncls, int splitk);
int sdt_conv_dw_variant(const sdt_conv_geom* g);
/* (Cout,T,Cin) -> (Cin,T,Cout): operand layout for the input-gradient GEMM. */
int sdt_weight_transpose_f32(const float* w, float* wt, int cout, int taps, int cin, void* stream);
/* Multiplication arithmetic of sdt_conv_taps(_splitk)_f32 for geometries with Cin % 32 == 0 (process-wide switch; tensors
 * stay fp32 in HBM and accumulation stays fp32 in every mode):
 *   SDT_MATH_F32    exact fp32 products on v_mfma_f32_32x32x2_f32 (default; what every parity claim refers to)
 *   SDT_MATH_BF16   operands rounded to bf16 (v_mfma_f32_32x32x16_bf16) -- BASELINE config 4's precision
 *   SDT_MATH_BF16X3 2-piece split, 3 bf16 products per fp32 product (~16 significant bits)
 *   SDT_MATH_BF16X6 exact 3-piece split of the 24-bit significand, 6 bf16 products (dropped terms < 2^-23 |ab|) */
enum { SDT_MATH_F32 = 0, SDT_MATH_BF16 = 1, SDT_MATH_BF16X3 = 3, SDT_MATH_BF16X6 = 6 };
int sdt_set_conv_math(int mode);
int sdt_get_conv_math(void);


/* Deterministic weight gradients of up to 24 SMALL layers in one grid + one ordered reduce (the generator's sixteen Conv1d blocks: launched one by
 * one each layer splits its rows ~32 ways to fill the chip and spends its time on slab traffic; together they need 2 row ranges each).
 * plan: host-built once per set of geometries (sdt_conv_dw_group_plan_bytes(n) bytes; the caller keeps a host and a device copy);
 * *workspace_bytes: slab space, no initialisation needed.  Accumulates into every dw[i] like sdt_conv_dw_det_f32 (fixed order, exact fp32).  */
int64_t sdt_conv_dw_group_plan_bytes(int n);
int sdt_conv_dw_group_plan(const sdt_conv_geom* const* geoms, int n, void* plan_out, int64_t* workspace_bytes);
int sdt_conv_dw_group_f32(const void* const* x, const void* const* dy, void* const* dw, int n, const void* plan_host, const void* plan_dev,
                          void* workspace, void* stream);
/* The same transposition for many layers in ONE launch (all mirrors of an optimiser group are refreshed right after its
 * Adam step).  table: device array of n_layers descriptors; tile_begin = running sum of
 * ceil(cin/32)*ceil(cout/32)*taps over the preceding layers, total_tiles = that sum over all layers. */
typedef struct sdt_wt_desc {
    const float* w; /* (cout, taps, cin) */
    float* wt;      /* (cin, taps, cout); nullable */
    void* w16;      /* nullable: bf16 copy of w (round to nearest even), the bf16-storage path's forward / weight operand */
    void* wt16;     /* nullable: bf16 copy of the mirror */
    int32_t cout, taps, cin, tile_begin;
    int32_t planes; /* what w16 / wt16 receive: 1 (or 0) = one bf16 copy; 3 = the exact three-way bf16 split [hi | mid | lo], three planes of
                       cout * taps * cin elements each: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) -- the pre-split B operand of
                       sdt_convsk_f32_w3 (ABI 5) */
    int32_t reserved;
} sdt_wt_desc;
int sdt_weight_transpose_batched_f32(const sdt_wt_desc* table, int n_layers, int total_tiles, void* stream);

/* out[c] += sum_rows x[row, c]  (bias gradient of the k1 head conv, generator.py:103). */
int sdt_col_sum_f32(const float* x, float* out, int64_t rows, int c, void* stream);

/*
 * Column-statistics normalisation over a (G, R, C) view: statistics per (g, c) over R rows.
 *   G=B, R=H*W  -> nn.InstanceNorm2d            (building_blocks.py:26)
 *   G=1, R=B*HW -> nn.BatchNorm{1,2}d, training (building_blocks.py:24,39)
 * followed by LeakyReLU(slope) (slope = 0 -> ReLU)  (building_blocks.py:46).
 * sums: workspace of 2*G*C doubles that MUST BE ZERO ON ENTRY (fp64 atomics accumulate into it; the call leaves it
 * dirty -- callers carve it from a region zeroed once per step instead of paying a memset per layer).
 * num_batches_tracked (nullable) is the
 * BatchNorm int64 counter, incremented on the device.  gamma/beta/running_* may be NULL (IN).
 * stats_ready != 0: sums already holds sum(y), sum(y^2) per (g, c) (sdt_conv_taps_stats_f32) -- the statistics pass is skipped.
 * *_t: the same with explicit element types (enum sdt_dtype) of the activation tensors -- the bf16-storage path: statistics, mean / rstd
 * and the arithmetic stay fp32, only what moves through HBM is bf16.  Built combinations: all fp32; forward y bf16 -> z bf16 | fp32;
 * backward y and dy bf16 with dz bf16 | fp32.
 * fwd writes z, mean[G*C], rstd[G*C]; if running_mean != NULL updates running stats with
 * momentum (unbiased variance), as nn.BatchNorm does in training mode -- with G > 1 as G consecutive calls of the module on the G
 * slices would: G updates in slice order, num_batches_tracked += G (the two no-grad pose-encoder passes of a train step in one launch).
 * eval: z = act(gamma*(y-running_mean)/sqrt(running_var+eps)+beta).
 */
int sdt_colnorm_fwd_f32(const float* y, float* z, double* sums, float* mean, float* rstd,
                        const float* gamma, const float* beta, float* running_mean, float* running_var,
                        int64_t* num_batches_tracked, int G, int64_t R, int C, float eps, float momentum,
                        float slope, int stats_ready, void* stream);
int sdt_colnorm_fwd_t(const void* y, int y_dtype, void* z, int z_dtype, double* sums, float* mean, float* rstd,
                      const float* gamma, const float* beta, float* running_mean, float* running_var,
                      int64_t* num_batches_tracked, int G, int64_t R, int C, float eps, float momentum,
                      float slope, int stats_ready, void* stream);
int sdt_colnorm_eval_f32(const float* y, float* z, const float* gamma, const float* beta,
                         const float* running_mean, const float* running_var,
                         int64_t rows, int C, float eps, float slope, void* stream);
/* bwd: dy <- d(loss)/dy given dz; dgamma/dbeta (nullable) are ACCUMULATED. dy may alias dz.
 * stats_ready != 0: sums already holds sum gg, sum gg*yhat per (g, c) (accumulated by the epilogue of the input-gradient
 * conv that produced dz, sdt_conv_taps_multi_f32 with nb) -- the statistics pass over dz and y is skipped. */
int sdt_colnorm_bwd_f32(const float* dz, const float* y, float* dy, double* sums, const float* mean,
                        const float* rstd, const float* gamma, const float* beta, float* dgamma,
                        float* dbeta, int G, int64_t R, int C, float slope, int stats_ready, void* stream);
int sdt_colnorm_bwd_t(const void* dz, int dz_dtype, const void* y, int y_dtype, void* dy, int dy_dtype, double* sums, const float* mean,
                      const float* rstd, const float* gamma, const float* beta, float* dgamma,
                      float* dbeta, int G, int64_t R, int C, float slope, int stats_ready, void* stream);

/*
 * First audio-encoder block fused for Cin == 1: Conv2d(1,64,k3,s1,p1,bias=False) -> InstanceNorm2d (groups = B) or
 * training-mode BatchNorm2d (groups = 1) -> LeakyReLU(slope)   (generator.py:16, building_blocks.py:15-26,46).
 * The statistics of all 64 channels are derived from 9+45 fp64 moments of the mel image, so z (B,H,W,64) is written once
 * and the raw conv output is never stored; backward recomputes the normalised pre-activation from mel.
 *   (both workspaces MUST BE ZERO ON ENTRY and are left dirty, like sdt_colnorm_*'s)
 *   fwd: mom = workspace of 54*B doubles; writes z, mean[groups*64], rstd[groups*64] (+ BN running stats / counter).
 *   bwd: mom = the moments fwd left in its workspace (read-only); sums = workspace of 11*groups*64 doubles;
 *        dw (64,9) and dgamma/dbeta (nullable) are ACCUMULATED.  One pass over dz: the weight gradient is assembled
 *        from 11 sums per (group, channel) and the mel moments.
 */
int sdt_l0_block_fwd_f32(const float* mel, const float* w, float* z, double* mom, float* mean, float* rstd,
                         const float* gamma, const float* beta, float* running_mean, float* running_var,
                         int64_t* num_batches_tracked, int B, int H, int W, int groups, float eps, float momentum,
                         float slope, void* stream);
int sdt_l0_block_bwd_f32(const float* dz, const float* mel, const float* w, const float* mean, const float* rstd,
                         const float* gamma, const float* beta, const double* mom, double* sums, float* dw, float* dgamma,
                         float* dbeta, int B, int H, int W, int groups, float slope, void* stream);
/* The same with z written / dz read as z_dtype / dz_dtype (enum sdt_dtype): the block's output is the first bf16 tensor of the bf16-storage
 * path, its backward reads the bf16 gradient the L1 input-gradient launch wrote.  mel, weights, moments, statistics: fp32 / fp64 as above. */
int sdt_l0_block_fwd_t(const float* mel, const float* w, void* z, int z_dtype, double* mom, float* mean, float* rstd,
                       const float* gamma, const float* beta, float* running_mean, float* running_var,
                       int64_t* num_batches_tracked, int B, int H, int W, int groups, float eps, float momentum,
                       float slope, void* stream);
int sdt_l0_block_bwd_t(const void* dz, int dz_dtype, const float* mel, const float* w, const float* mean, const float* rstd,
                       const float* gamma, const float* beta, const double* mom, double* sums, float* dw, float* dgamma,
                       float* dbeta, int B, int H, int W, int groups, float slope, void* stream);

/*
 * Row normalisation over C for each of `rows` rows + LeakyReLU: the reference's InstanceNorm1d
 * applied to the (B,T,C)-permuted tensor (building_blocks.py:50-51) == per-(b,t) LayerNorm, no affine.
 */
int sdt_rownorm_fwd_f32(const float* y, float* z, float* mean, float* rstd, int64_t rows, int C,
                        float eps, float slope, void* stream);
int sdt_rownorm_bwd_f32(const float* dz, const float* y, const float* mean, const float* rstd, float* dy,
                        int64_t rows, int C, float slope, void* stream);
/* rownorm_fwd fused with the split-K reduction of the producing conv: partial = nslab slabs of (rows, C) written by
 * sdt_conv_taps_splitk_f32; y <- their sum in slab order (what sdt_splitk_reduce_f32 computes), z/mean/rstd as above. */
int sdt_rownorm_slabs_fwd_f32(const float* partial, int nslab, float* y, float* z, float* mean, float* rstd,
                              int64_t rows, int C, float eps, float slope, void* stream);

/*
 * F.interpolate(x,(1,T),'bilinear') on the (B,H,W,C) encoder output, squeezed, with the gathered
 * clip code broadcast-concatenated along channels (generator.py:41-42,110-111; voice2pose.py:94):
 *   out (B,T,C+D);  out[b,t,C+d] = table[idx[b], d]   (D may be 0, table/idx NULL).
 */
int sdt_resize_concat_fwd_f32(const float* x, const float* table, const int64_t* idx, float* out,
                              int B, int H, int W, int C, int T, int D, void* stream);
/* dx (B,H,W,C) is fully written; dtable rows are ACCUMULATED (dense gradient of the code table). */
int sdt_resize_concat_bwd_f32(const float* dout, const int64_t* idx, float* dx, float* dtable,
                              int B, int H, int W, int C, int T, int D, void* stream);

/* F.interpolate(prev, To, 'linear') (+ skip) on (B,Ti,C)->(B,To,C) (generator.py:79-83, autoencoder.py:62-66). */
int sdt_upsample_add_fwd_f32(const float* prev, const float* skip, float* out, int B, int Ti, int To, int C, void* stream);
int sdt_upsample_add_bwd_f32(const float* dout, float* dprev, int B, int Ti, int To, int C, void* stream);

/* ---- The generator's Conv1d stage as one persistent launch per direction (csrc/chain1d.hip) ------------------------------------------
 * A CHAIN of ConvNormRelu('1d', norm='IN') blocks (building_blocks.py:31-51: Conv1d without bias -> normalisation of every (clip, frame) over
 * the channels -> LeakyReLU) with the wiring of UNet_1D + the decoder stack (generator.py:53-85,96-103): a block's input is the external
 * tensor (block 0), the activated output of an earlier block, or F.interpolate(earlier block, Ti, 'linear') + the activated output of another
 * one (generator.py:79-83).  Every block has 256 output channels; <= 64 frames per clip; Cin a multiple of 32 (<= 320, block 0 only: the
 * others read 256-channel block outputs).  Only the RAW conv outputs y travel between blocks; normalisation and activation are applied by
 * the consumer on load.  8 workgroups own a clip (see the file header); a launch holds 8 * (CUs / 64) clips (32 on MI355X) with every cluster
 * co-resident, a larger batch runs as consecutive launches.                                                                                  */
enum { SDT_CHAIN_PLAIN = 0, SDT_CHAIN_NORM = 1, SDT_CHAIN_UPADD = 2 };
typedef struct sdt_chain1d_layer {
    int32_t Ti, To, Cin, k, stride, pad;
    int32_t in_mode;        /* SDT_CHAIN_PLAIN: x0 | _NORM: act(norm(y[src_a])) | _UPADD: upsample(act(norm(y[src_a])), Ti) + act(norm(y[src_b])) */
    int32_t src_a, src_b;   /* indices of earlier blocks (-1: unused) */
    int32_t reserved;
    const float* w;         /* (256, k, Cin) weights */
    const float* wt;        /* (Cin, k, 256) mirror (backward only) */
    float* y;               /* (B, To, 256) raw conv output: written by forward, read by backward */
    float* x;               /* (B, Ti, 256) the conv's input as consumed, for the weight-gradient launch (NULL: not wanted; unused for block 0) */
    float* dy;              /* (B, To, 256) backward: gradient of y (the weight gradient's other operand) */
    float* dx;              /* (B, Ti, Cin) backward: gradient of the conv's input */
} sdt_chain1d_layer;
/* 1 when every block maps to a built K loop, every block but the last has a consumer (at most two direct ones and one upsampling one) and the
 * current device can hold a window of clusters, else 0.  The forward and the backward entry refuse (SDT_ERR_ARG, no launch) exactly what this refuses. */
int sdt_chain1d_supported(const sdt_chain1d_layer* layers, int nlayers, int B);
/* zout (B, To_last, 256) = act(norm(y[nlayers-1])).  counters: >= min(B, 8 * (CUs / 64)) zero-initialised uint32 (zero again when a launch ends); err: one uint32
 * that a launch sets non-zero when a workgroup gave up waiting for its cluster (sdt_convsk_set_spin_limit) -- results are then invalid. */
int sdt_chain1d_fwd_f32(const sdt_chain1d_layer* layers, int nlayers, const float* x0, float* zout, int B, float slope, float eps,
                        int math, void* counters, void* err, void* stream);
/* math: SDT_MATH_F32 (exact fp32 products, the default everywhere) or SDT_MATH_BF16 (products of bf16-rounded operands on the bf16 MFMA,
 * fp32 tensors and accumulation: what the bf16-storage step -- BASELINE config 4 -- runs; the global sdt_set_conv_math is NOT consulted).
 * gz (B, To_last, 256): gradient of zout.  Writes dy of every block and dx of every block (block 0 only when need_dx0). */
int sdt_chain1d_bwd_f32(const sdt_chain1d_layer* layers, int nlayers, const float* gz, int B, float slope, float eps, int need_dx0,
                        int math, void* counters, void* err, void* stream);

/* nn.L1Loss(reduction='none')(pred,gt)*lambda .mean() (voice2pose.py:141-142). partial: >=256 doubles. */
int sdt_l1_loss_fwd_f32(const float* pred, const float* gt, int64_t n, float lambda, double* partial, float* loss, void* stream);
int sdt_l1_loss_bwd_f32(const float* pred, const float* gt, const float* gout, int64_t n, float lambda, float* dpred, void* stream);
/*
 * The L1 loss with a confidence mask, per-channel weights and a velocity term (csrc/reg_loss.hip), on (B, T, C) fp32:
 *   e = double(pred) - double(gt);  d[b,t,c] = e[b,t+1,c] - e[b,t,c] for t < T-1
 *   m = score > min_conf ? 1 : 0 (score NULL: 1 everywhere, min_conf unused; the comparison is strict);  m2[b,t,c] = m[b,t,c] * m[b,t+1,c]
 *   w[c] = chan_w[c] (C floats; NULL: 1)
 *   losses[0] = lambda_reg * sum(m * w * |e|) / max(sum m, 1);   losses[1] = lambda_vel * sum(m2 * w * |d|) / max(sum m2, 1)
 * The denominators count live elements (the weights are not in them); an empty sum gives exactly 0.  Sums are float64 per-block partials
 * combined by one block in a fixed order, counts are exact integers, no atomics: two calls give the same bits.  Masked elements are selected
 * away, so whatever sits under the mask (NaN included) reaches neither a loss nor a gradient.  Nothing is read on the host: forward leaves
 * denom[0..1] = the two denominators on the device and backward divides by them.
 *   partial: >= 512 doubles, counts: >= 512 int64 (workspaces, contents irrelevant);  losses: 2 floats;  denom: 2 doubles.
 * Forward is two launches (partials, final block), backward one:
 *   kr = (gout_reg / denom[0]) * lambda_reg * w;   kv = (gout_vel / denom[1]) * lambda_vel * w      (float64, in this order)
 *   dpred = (float)(kr * m * sign(e) + kv * m2[t-1] * sign(d[t-1]) - kv * m2[t] * sign(d[t]))
 * with sign(0) = 0, terms of frames outside [0, T) absent, everything in float64 and rounded once.  The order is the one torch's autograd
 * takes on the float64 expression above, so terms that cancel there cancel here to the same exact 0.  gout_reg / gout_vel: one device
 * float each, NULL = that loss has no upstream gradient (its term is 0).
 */
int sdt_reg_loss_fwd_f32(const float* pred, const float* gt, const float* score, const float* chan_w, int B, int T, int C,
                         double lambda_reg, double lambda_vel, float min_conf, double* partial, int64_t* counts, float* losses,
                         double* denom, void* stream);
int sdt_reg_loss_bwd_f32(const float* pred, const float* gt, const float* score, const float* chan_w, const float* gout_reg,
                         const float* gout_vel, const double* denom, int B, int T, int C, double lambda_reg, double lambda_vel,
                         float min_conf, float* dpred, void* stream);
/*
 * Limb-length and limb-direction loss on the skeleton (csrc/bone_loss.hip).  pred, gt: fp32 (B, T, 2, K), channel
 * c = xy * K + k of a frame's C = 2 K;  mean, std: float64 (B, C);  score: fp32 (B, T, C) or NULL;  edges: int32 (E, 2);  edge_w: float64
 * (E) or NULL (1);  root: int32 (K), the part root of each keypoint or -1 (a root is itself in no part).  K <= 256, E <= 512.
 *   P[k] = double(pred[k]) * std[k] + mean[k];  X[k] = P[k] + (root[k] >= 0 ? P[root[k]] : 0);  Q, Y the same from gt
 *   live(k) = score_x[k] > min_conf and score_y[k] > min_conf and (root[k] < 0 or the same for root[k])   (score NULL: 1; strict)
 *   edge (a, b): vp = X[b] - X[a], vg = Y[b] - Y[a], lp = |vp|, lg = |vg|, m = live(a) and live(b), md = m and lp > 0 and lg > 0
 *   losses[0] = lambda_len * sum(m  w |lp - lg| / max(lg, min_len)) / max(sum m , 1)
 *   losses[1] = lambda_dir * sum(md w (1 - vp.vg / (lp lg)))        / max(sum md, 1)
 * Everything in float64, one rounding to fp32; per-frame partial sums and integer counts combined by one block in a fixed order, no
 * atomics: two calls give the same bits.  Dead edges are selected away: what sits under the mask (NaN included) reaches neither a loss nor
 * a gradient.  An empty sum gives exactly 0.  Nothing is read on the host: forward leaves denom[0..1] on the device for backward.
 *   psum: >= 2 B T doubles, pcnt: >= 2 B T int64 (workspaces, contents irrelevant);  losses: 2 floats;  denom: 2 doubles.
 * Forward is two launches, backward one:
 *   dX[b] += g_e, dX[a] -= g_e over the live edges incident to a keypoint, in ascending edge order, with
 *   g_e = cl w sign(lp - lg) / max(lg, min_len) * vp / lp  (0 where lp = 0)  -  cd w (vg / (lp lg) - (vp.vg) vp / (lp^3 lg))  (md only),
 *   cl = (gout_len / denom[0]) * lambda_len, cd = (gout_dir / denom[1]) * lambda_dir;
 *   dpred[k] = (float)(std[k] * (dX[k] + sum of dX[j] over the children j of k in ascending order)).
 * inc_ptr (K + 1) / inc_edge (2 E): the edges incident to each keypoint, entry = 2 * e + (1 if the keypoint is the edge's a end);
 * child_ptr (K + 1) / child_idx: the children of each keypoint (root[j] == k), ascending.  gout_len / gout_dir: one device float each,
 * NULL = that loss has no upstream gradient.
 */
int sdt_bone_loss_fwd_f32(const float* pred, const float* gt, const float* score, const double* mean, const double* std,
                          const int32_t* edges, const double* edge_w, const int32_t* root, int B, int T, int K, int E, double lambda_len,
                          double lambda_dir, float min_conf, double min_len, double* psum, int64_t* pcnt, float* losses, double* denom,
                          void* stream);
int sdt_bone_loss_bwd_f32(const float* pred, const float* gt, const float* score, const double* mean, const double* std,
                          const int32_t* edges, const double* edge_w, const int32_t* root, const int32_t* inc_ptr, const int32_t* inc_edge,
                          const int32_t* child_ptr, const int32_t* child_idx, const float* gout_len, const float* gout_dir,
                          const double* denom, int B, int T, int K, int E, double lambda_len, double lambda_dir, float min_conf,
                          double min_len, float* dpred, void* stream);
/* LSGAN terms (voice2pose.py:171-189, nn.MSELoss against a constant): loss = lambda * mean((scores - target)^2);
 * dscores = gout * 2 * lambda / n * (scores - target). */
int sdt_mse_const_fwd_f32(const float* scores, int64_t n, float target, float lambda, float* loss, void* stream);
int sdt_mse_const_bwd_f32(const float* scores, const float* gout, int64_t n, float target, float lambda, float* dscores, void* stream);

/*
 * Clip-code batch KL (voice2pose.py:147-157): code = table[idx] (B,D); mu/unbiased var over the batch;
 * loss = 0.5*mean(-log v + mu^2 + v - 1)*lambda if every v != 0 else 0; valid[0] = that predicate
 * (kept on the device: no host sync).  code_out (B,D) receives the gathered rows.
 * N = rows of the table: an index outside [0, N) reads nothing (the reference raises IndexError there) -- its code row
 * becomes NaN, which poisons the losses, and its gradient row is dropped.
 */
int sdt_code_kl_fwd_f32(const float* table, const int64_t* idx, int N, int B, int D, float lambda,
                        float* code_out, float* loss, int32_t* valid, void* stream);
int sdt_code_kl_bwd_f32(const float* code, const int32_t* valid, const float* gout, const int64_t* idx,
                        int N, int B, int D, float lambda, float* dtable, void* stream);

/*
 * GestureDataset.get_final_results x2 + Voice2Pose.evaluate_step (gesture_dataset.py:193-220,
 * voice2pose.py:412-430), float64 like the reference: final_* (B,T,2,K) f64 (nullable),
 * metrics[0]=L2_dist, metrics[1]=lip_sync_error_n.  work: >= 3*B*T + 4 doubles, contents irrelevant (per-frame
 * partial sums, combined in a fixed order: no atomics, bit-identical from run to run).
 */
int sdt_final_metrics_f64(const float* pred, const float* gt, const double* mean, const double* std,
                          const double* scale, int hierarchical, int B, int T, int K,
                          double* final_pred, double* final_gt, double* work, double* metrics, void* stream);

/* torch.optim.Adam(betas, eps, weight_decay) step over a flat fp32 buffer (voice2pose.py:249-279,302-304).
 * lr_dev: device float (so that LR schedules do not invalidate a captured hipGraph);
 * state_dev: 16 device bytes {int64 step; float bc1; float bc2_sqrt}, zero-initialised by the caller;
 * the call increments `step` on the device and derives the bias corrections from it.
 * grad_scale multiplies g on load (1/world_size after a summing all-reduce: DDP's gradient averaging). */
int sdt_adam_step_f32(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1,
                      float beta2, float eps, float weight_decay, float grad_scale, void* state_dev, void* stream);

/*
 * Mel front end (torchaudio 0.7 MelSpectrogram as configured at voice2pose.py:27-30):
 * reflect-pad 256, 512-sample frames every 160, periodic-Hann(400) centred, |rFFT|^2, HTK filterbank.
 * The STFT is run as an MFMA GEMM by sdt_conv_taps_f32 over the hop matrix:
 *   sdt_stft_frames_f32 : audio (B,L) -> hops (B, nhops, 160), hops[b, j] = reflect_pad(audio)[j + 56]
 *   sdt_conv_taps_f32   : X = hops as (B,1,nhops,160), W = windowed DFT basis (514, 3, 160)
 *                         (row 2f = w*cos, 2f+1 = -w*sin of bin f; taps >= 400 samples are zero) -> spec (B,F,514)
 *   sdt_mel_fb_f32      : spec (B,F,2*nfreq) interleaved re/im -> mel (B, nmel, F) = fb^T |spec|^2 (sparse rows only)
 */
int sdt_stft_frames_f32(const float* audio, float* hops, int B, int L, int nhops, void* stream);
/* bin_lo/bin_hi (nmel ints each, device): [lo,hi) range of non-zero filterbank rows of every mel filter (triangles). */
int sdt_mel_fb_f32(const float* spec, const float* fb, const int32_t* bin_lo, const int32_t* bin_hi, float* mel, int B, int F,
                   int nfreq, int nmel, void* stream);

/* dst[idx[b], :] += src[b, :]  -- dense gradient of the clip-code table for `clips_code[clip_indices]` (voice2pose.py:94).
 * dst has N rows; rows with idx outside [0, N) are skipped. */
int sdt_rows_scatter_add_f32(const float* src, const int64_t* idx, float* dst, int N, int B, int D, void* stream);

/* y[i] = a[i+stride]-a[i] helper for the motion discriminator input (voice2pose.py:187-188): (B,T,C)->(B,T-1,C) */
int sdt_time_diff_fwd_f32(const float* x, float* y, int B, int T, int C, void* stream);
int sdt_time_diff_bwd_f32(const float* dy, float* dx, int B, int T, int C, void* stream);

/* Batch assembly from a clip store resident in HBM -- the device-side form of GestureDataset.__getitem__ + collate
 * (core/datasets/gesture_dataset.py:85-119): for every b, clip = idx[b]:
 *   raw (N, Tstore, 3, 137) OpenPose x / y / confidence  -> first T frames, 137 -> 122 -> 121 keypoints (:124-145),
 *   relative to the root joint, optionally hierarchical ("parted": head / hand offsets, :157-165), then
 *   (x - mean) / std with fp32 statistics (242,) (:167-176);  poses (B,T,2,121), score (B,T,2,121) = confidence twice.
 * Same fp32 operation order as the reference's torch code -> bit-identical results.
 *   sdt_rows_gather_f32: dst[b, :] = src[idx[b], :]   (the cropped / zero-padded audio rows, n_cols % 4 == 0 not required) */
int sdt_clip_poses_prepare_f32(const float* raw, const int64_t* idx, const float* mean, const float* std, float* poses,
                               float* score, int N, int Tstore, int B, int T, int hierarchical, void* stream);
int sdt_rows_gather_f32(const float* src, const int64_t* idx, float* dst, int N, int B, int64_t n_cols, void* stream);

/*
 * Skeleton rendering (core/utils/keypoint_visualization.py:8-110,177-207: draw_body_parts, vis_relative_pose_clip,
 * vis_relative_pose_pair_clip, draw_pose_frames_in_long_img; DESIGN.md section 10 is the drawing contract).
 * A launch draws n_images images of H x W BGR uint8 pixels, (n_images, H, W, 3) row-major.  Each image is the list of
 * its n_inst instances (instance k of image i = inst[i*n_inst + k]), drawn in that order; an instance is one pose of
 * the skeleton table of K in {121, 135, 137} keypoints (sdt_render_edges(K) = 108 / 109 / 109 edges).
 * Endpoint of keypoint j: (int)(p[j]*scale + off) with the multiply and the add rounded separately (float64, no FMA),
 * truncated toward zero, then shifted by shift_x columns.  An edge with a non-finite endpoint or |p*scale + off| > 2^24,
 * or of an instance whose pose index lies outside [0, n_poses), is not drawn and is counted in *skipped (nullable).
 * Workspace: sdt_render_workspace_bytes(n_images, n_inst, K) bytes; prepare writes all of it (one record of 16 int32 per
 * stroke: x0 y0 x1 y1 | bbox x0 y0 x1 y1, inclusive, empty if x0 > x1 | the segment clipped near the window, 4 floats |
 * B | G<<8 | R<<16 | thickness<<24, clip_x0, clip_x1, drawn), skeleton_u8 reads it and writes every output byte.
 */
typedef struct sdt_render_instance {
    int64_t pose;             /* index of the (2, K) float64 pose slice: x row then y row */
    double off_x, off_y;      /* canvas centre, added after the multiply */
    double scale;             /* VISUALIZATION_SCALING (1.0 for the long image) */
    int32_t shift_x;          /* integer column origin of the instance's window (long image), added after truncation */
    int32_t clip_x0, clip_x1; /* columns [clip_x0, clip_x1) the instance may touch (clamped to [0, W)) */
    int32_t reserved;
} sdt_render_instance;

int64_t sdt_render_workspace_bytes(int n_images, int n_inst, int K);
int sdt_render_edges(int K);
int sdt_render_prepare_f64(const double* poses, int64_t n_poses, int K, const sdt_render_instance* inst, int n_images, int n_inst,
                           int H, int W, void* workspace, int64_t workspace_bytes, int32_t* skipped, void* stream);
int sdt_render_skeleton_u8(const void* workspace, int64_t workspace_bytes, int n_images, int n_inst, int K, int H, int W,
                           uint8_t* out, int64_t out_bytes, void* stream);

/*
 * A speaker's pose statistics (data_preprocess/4_1_calculate_mean_std.py:59-116,193-225 and 4_2_parse_mean_std_npz.py:16-23;
 * DESIGN.md section 11 is the contract).  The training clips are split into num_chunks chunks of rows_per_chunk clips; clip j of
 * chunk c is (num_frames, 2, 137) x / y in pixels, float32 (elem_bytes 4) or float64 (elem_bytes 8), at
 * poses + c*chunk_pitch + (j - first_row)*num_frames*274 elements for j in [first_row, first_row + window).
 * accumulate advances, for every (chunk, frame, keypoint) and both modes (parted = pose_np_deduct_root, global = root only), the
 * running mean (pass 1, cal_mean_*: avg = avg*w + (1-w)*q, w = n/(n+1)) or the running variance around the pass-1 means
 * (pass 2, cal_std_*: var = var*w + (1-w)*(q - M)**2; mean137 = finalize's out137 of pass 1) over the window's clips in order,
 * skipping a keypoint when |q_x + root_x| < 5 and |q_y + root_y| < 5.  The root deduction and that test are computed in the
 * pose element type, the rest in float64 with every operation rounded on its own.  first_row == 0 starts from zero; later
 * windows continue from the state buffer (sdt_speaker_stats_state_bytes(num_chunks, num_frames) bytes, float64).  A non-finite
 * x / y is recorded as the first such row (c*rows_per_chunk + j) of its lane.
 * finalize (one launch per pass): out137 (2 modes parted / global, 2 coordinates, 137) = the per-chunk tables averaged over
 * chunks, then frames, in index order (pass 2: the square root of each chunk's variance first, :116); out242 (2 modes, 242) =
 * the same without 4_2's 16 deleted keypoints, x row then y row; counts (2, 137) = kept detections; first_bad_row (137) = 1 + the
 * first row with a non-finite coordinate of that keypoint, 0 if none; flags (2, 137): bit 0 = a non-finite result,
 * bit 1 (pass 2) = a kept keypoint with a zero std.  No allocation; every pointer is a device buffer; every index is checked
 * against the sizes given.
 */
int64_t sdt_speaker_stats_state_bytes(int num_chunks, int num_frames);
int sdt_speaker_stats_accumulate(int pass, int elem_bytes, const void* poses, int64_t poses_elems, int64_t chunk_pitch, int num_chunks,
                                 int num_frames, int window, int64_t first_row, int64_t rows_per_chunk, const double* mean137, void* state,
                                 int64_t state_bytes, void* stream);
int sdt_speaker_stats_finalize(int pass, const void* state, int64_t state_bytes, int num_chunks, int num_frames, double* out137,
                               double* out242, double* counts, int64_t* first_bad_row, int32_t* flags, void* stream);

/*
 * The per-epoch clip-code figure (core/pipelines/voice2pose.py:479-510 and pose2pose.py:314-345, draw_figure_epoch: PCA(n_components=2)
 * of the clip-code table and plt.scatter of the projection; logged by core/pipelines/trainer.py:404-405,281-283; DESIGN.md section 12
 * is the contract).  x is the (n_rows, dim) fp32 table, 2 <= dim <= 64, 2 <= n_rows <= 2^30; all arithmetic is float64.
 * Workspace: sdt_code_pca_workspace_bytes(n_rows, dim) bytes (0: unsupported sizes), shared by moments and project, never read before
 * it is written.  No allocation; every pointer is a device buffer; every index is checked against the sizes given.
 *   moments (voice2pose.py:495-498, the centring and the scatter matrix inside pca.fit): mean (dim) = column sums / n_rows,
 *     cov (dim, dim) = centred products / (n_rows - 1), both from per-workgroup partials reduced in workgroup order (fixed grid, no
 *     floating-point atomics: the same bits on every call).  first_bad_row[0] = 1 + the first row with a non-finite entry, 0 if none.
 *   eigh (the decomposition inside pca.fit): cyclic Jacobi, one workgroup, until off(A) <= rel_tol * ||cov||_F.  evals (dim),
 *     descending; comps (2, dim) = the two leading eigenvectors, each signed so that its entry of largest magnitude (first of equals)
 *     is positive; info (4) = sweeps done, final off-diagonal Frobenius norm, ||cov||_F, trace(cov); err[0]: bit 0 = not converged
 *     within max_sweeps, bit 1 = trace(cov) is not positive.
 *   project (voice2pose.py:499, pca.transform): X (n_rows, 2) float64 = (x - mean) . comps^T, dim ascending; limits (8) = min0, max0,
 *     min1, max1 of X, then the axis limits lo0, hi0, lo1, hi1 = min - 0.05 span, max + 0.05 span (an axis with hi <= lo:
 *     [min - 0.5, max + 0.5]).
 *   raster (voice2pose.py:500, plt.scatter(alpha=0.2, edgecolors='none', s=1)): plot rectangle = the canvas inset by `margin` pixels
 *     with a 1-pixel black ring around it.  Point n -> column min(int(floor((X0 - lo0) * (Pw / (hi0 - lo0)))), Pw - 1), row likewise on
 *     axis 1 and flipped, every operation rounded on its own; the marker_px x marker_px block from (col - (marker_px-1)/2,
 *     row - (marker_px-1)/2), clipped to the rectangle, is counted into counts (Ph, Pw) uint32 with integer atomics; points outside
 *     axis_limits (4: lo0, hi0, lo1, hi1) or not finite are skipped.  Then out (H, W, 3) uint8 RGB = table[min(count, table_len - 1)]
 *     inside the rectangle (table: (table_len, 3) uint8, entry k = k markers composited over white), white outside.  The CALLER zeroes
 *     counts before the call; the kernels leave the counts in it.
 */
int64_t sdt_code_pca_workspace_bytes(int64_t n_rows, int dim);
int sdt_code_pca_moments(const float* x, int64_t n_rows, int dim, void* workspace, int64_t workspace_bytes, double* mean, double* cov,
                         int64_t* first_bad_row, void* stream);
int sdt_code_pca_eigh(const double* cov, int dim, int max_sweeps, double rel_tol, double* evals, double* comps, double* info, int32_t* err,
                      void* stream);
int sdt_code_pca_project(const float* x, int64_t n_rows, int dim, const double* mean, const double* comps, double* X, void* workspace,
                         int64_t workspace_bytes, double* limits, void* stream);
int sdt_code_pca_raster(const double* X, int64_t n_rows, const double* axis_limits, const uint8_t* table, int table_len, int H, int W,
                        int margin, int marker_px, uint32_t* counts, int64_t counts_elems, uint8_t* out, int64_t out_bytes, void* stream);

/*
 * Principal template axes and nearest template codes (code_axes.py; DESIGN.md section 17 is the contract): what a user needs to pick the
 * codes of the two demo modes (pose2pose.py:50-56 DEMO.CODE_PATH; voice2pose.py:107-117 DEMO.CODE_INDEX / CODE_INDEX_B).  x is the
 * (n_rows, dim) fp32 table.  Supported sizes: 2 <= n_rows <= 2^30, 2 <= dim <= 64, 1 <= n_queries <= 65536, 1 <= n_ranks <= 16; outside
 * them the workspace queries return 0 and the entry points SDT_ERR_UNSUPPORTED.  All arithmetic is float64 on values converted exactly
 * from fp32, every operation rounded on its own; no floating-point atomics: the same bits on every call.  No allocation; every pointer
 * is a device buffer; every index is checked against the sizes given.  Mean and covariance come from sdt_code_pca_moments.
 *   eigh: as sdt_code_pca_eigh (the same device code), but comps is (dim, dim): every eigenvector, ranked by descending eigenvalue
 *     (ties: the lower original column first), each signed so that its entry of largest magnitude (first of equals) is positive.
 *     evals[0:2] and rows 0 and 1 of comps carry the bits sdt_code_pca_eigh returns.  0 <= max_sweeps <= 1000; info and err as there.
 *   project: P (n_rows, dim) float64, P[n,k] = sum over d ascending of (x[n,d] - mean[d]) * comps[k,d]; columns 0 and 1 carry the bits
 *     of sdt_code_pca_project's X.
 *   quantiles: out (dim, n_ranks), out[k,r] = the element of column k of P that an ascending sort puts at position ranks[r]
 *     (0 <= ranks[r] < n_rows, a device array of int64; the caller checks the range), by a radix select on the order-preserving uint64
 *     image of the float64 bits: exact; -0.0 and +0.0 may come back as either zero.  Workspace:
 *     sdt_code_axes_quantiles_workspace_bytes(n_rows, dim, n_ranks) bytes, never read before it is written.
 *   nearest: d2(q, n) = sum over d ascending of (queries[q,d] - x[n,d])^2 with queries (n_queries, dim) float64; index[q] = the smallest
 *     n that attains the minimum, dist2[q] = that minimum.  first_bad_query[0] = the first query with a non-finite entry, -1 if none;
 *     such a query gets index -1 and dist2 NaN.  Workspace: sdt_code_axes_nearest_workspace_bytes(n_rows, dim, n_queries) bytes.
 */
int sdt_code_axes_eigh(const double* cov, int dim, int max_sweeps, double rel_tol, double* evals, double* comps, double* info, int32_t* err,
                       void* stream);
int sdt_code_axes_project(const float* x, int64_t n_rows, int dim, const double* mean, const double* comps, double* P, void* stream);
int64_t sdt_code_axes_quantiles_workspace_bytes(int64_t n_rows, int dim, int n_ranks);
int sdt_code_axes_quantiles(const double* P, int64_t n_rows, int dim, const int64_t* ranks, int n_ranks, double* out, void* workspace,
                            int64_t workspace_bytes, void* stream);
int64_t sdt_code_axes_nearest_workspace_bytes(int64_t n_rows, int dim, int64_t n_queries);
int sdt_code_axes_nearest(const float* x, int64_t n_rows, int dim, const double* queries, int64_t n_queries, int64_t* index, double* dist2,
                          int64_t* first_bad_query, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * Clusters of the template-code table and the row that stands for each (code_clusters.py; DESIGN.md section 19 is the contract): k-means
 * on the (n_rows, dim) fp32 table x, so that a user can name DEMO.CODE_INDEX / CODE_INDEX_B (voice2pose.py:107-117) and write a
 * DEMO.CODE_PATH file with one code per cluster (pose2pose.py:50-56).  Supported sizes: 2 <= n_rows <= 2^24, 2 <= dim <= 64, 1 <= k <= 64,
 * k <= n_rows; outside them the workspace queries return 0 and the entry points SDT_ERR_UNSUPPORTED.  All arithmetic is float64 on values
 * converted exactly from fp32, every operation rounded on its own; d2(a, b) = sum over d ascending of (a[d] - b[d])^2.  Rows form chunks
 * of 1024 consecutive rows; every sum over rows runs rows ascending inside a chunk from +0.0, then chunks ascending.  No floating-point
 * atomics, no allocation, no workspace read before it is written; every pointer is a device buffer; row and cluster numbers read from
 * device buffers are checked against the sizes given.  The table must be finite (sdt_code_pca_moments reports the first row that is not).
 *   seed_update: m[n] = d2(x[n], x[seeds[j]]) if first != 0, else min(m[n], that); leaves in the workspace, per chunk, the ordered sum of
 *     m, the largest m with its lowest row, and the last row with m > 0.  0 <= j < 64.
 *   seed_pick (after seed_update, same workspace) writes seeds[j], 1 <= j < min(64, n_rows).  mode 0, k-means++ with 0 <= u <= 1: P[c] =
 *     running sum of the chunk sums, T = P[last], r = u T; the chunk is the first with P[c] > r; inside it the running sum starts at
 *     P[c - 1] (0 for c = 0) and adds m[n] ascending; the seed is the first row whose running sum exceeds r, else the chunk's last row
 *     with m > 0; no chunk passes: the table's last row with m > 0; T == 0: the lowest row not among seeds[0, j).  mode 1, farthest: the
 *     row of the largest m, of equals the lowest; a largest m of 0: the T == 0 rule.  info (4 float64): T (mode 1: the largest m), r, the
 *     chunk or -1, the rule that chose (0 the walk, 1 the chunk's last positive row, 2 the table's, 3 T == 0, 4 farthest).
 *   assign: labels[n] = argmin over c of d2(x[n], centers[c]), of equals the lowest c; changed[0] = the number of rows whose label differs
 *     from the one labels held before (first != 0: labels is not read and every row counts).  centers is (k, dim) float64.
 *   update: total[c][d] = the ordered sum of x[n, d] over the rows with labels[n] == c, counts[c] = their number (int32),
 *     centers[c][d] = total / (double)count; a cluster without rows keeps its centre.  Workspace:
 *     sdt_code_clusters_update_workspace_bytes(n_rows, dim, k) bytes (chunks * k * dim float64 partials and the chunk counts).
 *   final: assigns against centers once more, then numbers the clusters by descending count (ties: the lower number first) and writes, in
 *     that numbering, labels (n_rows int32), centers_out (k, dim; must not be centers), counts (k int32), within_ss (k) = the ordered sum
 *     of d2 over the members, code_index (k int64) = the member with the smallest (d2, row) and code_dist2 (k) its d2 (-1 and +inf for a
 *     cluster without rows), order (k int32) = the old number of every new cluster, inertia[0] = the ascending sum of within_ss.
 *     Workspace: sdt_code_clusters_final_workspace_bytes(n_rows, dim, k) bytes.
 */
int64_t sdt_code_clusters_seed_workspace_bytes(int64_t n_rows, int dim);
int sdt_code_clusters_seed_update(const float* x, int64_t n_rows, int dim, const int64_t* seeds, int j, int first, double* m, void* workspace,
                                  int64_t workspace_bytes, void* stream);
int sdt_code_clusters_seed_pick(const double* m, int64_t n_rows, int mode, double u, int64_t* seeds, int j, double* info, void* workspace,
                                int64_t workspace_bytes, void* stream);
int sdt_code_clusters_assign(const float* x, int64_t n_rows, int dim, const double* centers, int k, int32_t* labels, int first, int64_t* changed,
                             void* stream);
int64_t sdt_code_clusters_update_workspace_bytes(int64_t n_rows, int dim, int k);
int sdt_code_clusters_update(const float* x, int64_t n_rows, int dim, const int32_t* labels, int k, double* centers, int32_t* counts,
                             void* workspace, int64_t workspace_bytes, void* stream);
int64_t sdt_code_clusters_final_workspace_bytes(int64_t n_rows, int dim, int k);
int sdt_code_clusters_final(const float* x, int64_t n_rows, int dim, const double* centers, int k, int32_t* labels, double* centers_out,
                            int32_t* counts, double* within_ss, double* inertia, int64_t* code_index, double* code_dist2, int32_t* order,
                            void* workspace, int64_t workspace_bytes, void* stream);

/*
 * The epoch-level validation metric, the Frechet gesture distance (core/utils/fgd.py:6-64, called from voice2pose.py:432-446; DESIGN.md
 * section 13 is the contract).  A feature row is row r of the fp32 (rows, d0) tensor x0 followed by row r of the fp32 (rows, d1) tensor
 * x1 (x1 NULL with d1 = 0); dim = d0 + d1, 2 <= dim <= 64.  All arithmetic is float64.  No allocation; every pointer except the two
 * state-pointer arrays of finalize (host arrays, read during the call) is a device buffer; every size is checked before the launch.
 *   state: sdt_fgd_state_bytes(dim) bytes (0: unsupported dim), 8-byte aligned, ZEROED by the caller once (and again to reset it).  In 8-byte
 *     words: rows (int64) | 1 + the first non-finite row, 0 if none (int64) | shift (dim) | sums of x - shift (dim) | upper triangle of the
 *     sums of (x - shift)(x - shift)^T, row-major (dim (dim + 1) / 2).  The shift is the first row the state ever sees (a non-finite entry
 *     of it: 0).
 *   accumulate: adds `rows` rows (1 <= rows <= 2^30) to a state, one workgroup, the rows in ascending order per entry: the state does not
 *     depend on how the rows were cut into calls, and equal call sequences give equal bits.  A non-finite value records
 *     rows_seen_base + r of the first such row (the first record stays) and makes the sums non-finite; finalize reports it.
 *   finalize: states_a / states_b are num_states (1..64) state pointers per side (one per rank after an all-gather), merged in index order
 *     with the pairwise update of (n, mean, M2); states without rows are skipped.  On the leading dim_used x dim_used block
 *     (2 <= dim_used <= dim), with mean and covariance as numpy's (ddof = 1):
 *       C_A = V L V^T (cyclic Jacobi until off(A) <= rel_tol ||A||_F), S = V sqrt(max(L, 0)) V^T, mu = eig(sym(S C_B S)) (Jacobi again),
 *       FGD = |mean_A - mean_B|^2 + tr C_A + tr C_B - 2 sum_i sqrt(max(mu_i, 0))   (not clamped at zero).
 *     out (16 float64): FGD, |mean_A - mean_B|^2, tr C_A, tr C_B, sum_i sqrt(max(mu_i, 0)), rows of A, rows of B, sweeps and final
 *     off-diagonal Frobenius norm of the first decomposition, the same of the second, the smallest eigenvalue of the first and of the second,
 *     the first non-finite row of A and of B (-1: none), 0.  err[0]: bit 0 = a decomposition did not converge within max_sweeps (FGD is
 *     the value reached), bit 1 = fewer than 2 rows on a side, bit 2 = a non-finite row was recorded; with bit 1 or 2 every float field but
 *     the rows and the bad rows is NaN.
 */
int64_t sdt_fgd_state_bytes(int dim);
int sdt_fgd_accumulate(const float* x0, int d0, const float* x1, int d1, int64_t rows, void* state, int64_t state_bytes,
                       int64_t rows_seen_base, void* stream);
int sdt_fgd_finalize(const void* const* states_a, const void* const* states_b, int num_states, int dim, int dim_used, int max_sweeps,
                     double rel_tol, double* out, int32_t* err, void* stream);

/*
 * Baseline JPEG encoding of the renderer's frames (DESIGN.md section 14 is the contract; integer arithmetic only, a host model
 * reproduces the bytes).  frames: (n, H, W, 3) uint8 BGR, any 1 <= n, H, W <= 65535.  The stream is SOF0, YCbCr 4:2:0, one scan, one
 * restart interval per MCU row (ceil(W / 16) MCUs), DC prediction reset per interval.  The library writes the entropy-coded part only:
 * for image i the bytes [offsets[i * rows], offsets[(i + 1) * rows]) of `out`, rows = ceil(H / 16), are everything that follows the SOS
 * header: the intervals, each padded with 1-bits to a byte and with 0x00 stuffed after every 0xFF, RST0..7 cycling between them, and EOI.
 * The caller writes the headers and owns the tables they announce:
 *   tables (SDT_JPEG_TABLE_WORDS uint32, device): 64 luminance then 64 chrominance quantisation values (1..255, clamped) in natural
 *     (row-major) order | 16 DC luminance | 16 DC chrominance | 256 AC luminance | 256 AC chrominance Huffman entries, indexed by symbol,
 *     each code | length << 16 (length <= 16, clamped; 0 = no code).
 *   colour:  Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
 *     Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16 (arithmetic shifts); the last row and column are repeated up to a
 *     multiple of 16; chroma = (a + b + c + d + bias) >> 2 over 2 x 2 with bias 1, 2, 1, 2, ... along the output columns.
 *   transform: level shift -128, the 13-bit LLM integer forward DCT (rows with 2 extra bits, then columns; outputs carry a factor 8),
 *     quantised as sign(c) * ((|c| + 4 q) / (8 q)).
 * measure = transform + the exact byte length of every interval + their exclusive prefix sum: offsets (intervals + 1 int64, device),
 *   offsets[intervals] = the total.  pack writes the bytes; it needs the workspace measure left and out_bytes >= the total.
 * workspace: sdt_jpeg_workspace_bytes(n, H, W) bytes (0: unsupported sizes), 16-byte aligned, written before it is read.
 * err (device int32; measure zeroes it): SDT_JPEG_ERR_STAGE = one MCU's codes exceed the staging buffer (only with a malformed table),
 *   SDT_JPEG_ERR_RANGE = pack met a byte position outside its interval's range (offsets not from measure on the same input); nothing
 *   is written outside `out` in either case.  No allocation; every index is checked against the sizes given.
 */
#define SDT_JPEG_TABLE_WORDS 672
#define SDT_JPEG_ERR_STAGE 1
#define SDT_JPEG_ERR_RANGE 2
int64_t sdt_jpeg_workspace_bytes(int n, int H, int W);
int64_t sdt_jpeg_intervals(int n, int H, int W);
int sdt_jpeg_measure(const uint8_t* frames, int64_t frames_bytes, int n, int H, int W, const uint32_t* tables, void* workspace,
                     int64_t workspace_bytes, int64_t* offsets, int64_t offsets_elems, int32_t* err, void* stream);
int sdt_jpeg_pack(const void* workspace, int64_t workspace_bytes, int n, int H, int W, const uint32_t* tables, const int64_t* offsets,
                  int64_t offsets_elems, uint8_t* out, int64_t out_bytes, int32_t* err, void* stream);

/*
 * Animated-GIF encoding of the renderer's frames for the TensorBoard video summary (core/utils/video_processing.py:72-98; DESIGN.md
 * section 15 is the contract; integer arithmetic only, gif.py's model_* functions reproduce the bytes).  frames: (n, H, W, 3) uint8 BGR.
 *   downscale (F.interpolate(scale_factor=0.4, mode='area')): h = (2 H) / 5, w = (2 W) / 5 (or h = H, w = W: no downscale); output pixel
 *     (i, j) = per channel (sum + cnt / 2) / cnt over source rows [floor(i H / h), ceil((i + 1) H / h)) and the same range of columns,
 *     cnt = the number of source pixels in the window; channels swapped to RGB.
 *   quantisation: bin = (R >> 3) << 10 | (G >> 3) << 5 | (B >> 3); one histogram over the clip (32-bit integer counts).  The palette is the
 *     at most 256 most populated non-empty bins, ties at the cut won by the lower bin, listed in ascending bin order; a palette colour is
 *     c5 << 3 | c5 >> 2 per channel, unused entries are 0.  Every bin maps to the palette entry with the smallest squared distance in
 *     5-bit space, ties to the lower entry.
 *   LZW (GIF89a, minimum code size 8: Clear 256, EOI 257, first free code 258, 9-bit start, LSB first): a row of a frame is one segment, or,
 *     if w > 3838, parts = ceil(w / 3838) segments of ceil(w / parts) pixels, the last taking the rest.  A frame's stream is Clear at 9 bits,
 *     then per segment its codes from an EMPTY table followed by Clear (after the frame's last segment: EOI) at the width the segment ended
 *     in.  Code k of a segment (k = 0, 1, ...) is 9 + (k >= 255) + (k >= 767) + (k >= 1791) bits wide, and so is the code that follows a
 *     segment of k codes.  Frames start on a byte; the last byte of a frame is padded with 0-bits.
 * quantise writes rgb (n, h, w, 3; nullable), indices (n, h, w) and palette (256, 3).  measure codes every segment and writes offsets
 *   (int64, device): [0 .. n] the byte offset of every frame's stream and the total, [n + 1 + s] the bit offset of the first code of segment
 *   s = (frame * h + row) * parts + part.  pack zeroes out[0, out_bytes) and writes the streams; it needs the workspace measure left,
 *   out 4-byte aligned and out_bytes a multiple of 4 that is >= the total.
 * workspace: sdt_gif_workspace_bytes(n, h, w) bytes (0: unsupported sizes), 16-byte aligned, written before it is read; quantise and
 *   measure / pack may share it (measure overwrites what quantise left).
 * err (device int32; measure zeroes it): SDT_GIF_ERR_RANGE = pack met a bit outside its frame's byte range (offsets not from measure on the
 *   same input): it is dropped; SDT_GIF_ERR_COUNT = a segment's code count in the workspace exceeds its length: the segment is skipped.
 *   Nothing is written outside `out` in either case.  No allocation; every index is checked against the sizes given.
 */
#define SDT_GIF_ERR_RANGE 1
#define SDT_GIF_ERR_COUNT 2
int64_t sdt_gif_workspace_bytes(int n, int h, int w);
int sdt_gif_quantise(const uint8_t* frames, int64_t frames_bytes, int n, int H, int W, int h, int w, uint8_t* rgb, int64_t rgb_bytes,
                     uint8_t* indices, int64_t indices_bytes, uint8_t* palette, void* workspace, int64_t workspace_bytes, void* stream);
int sdt_gif_measure(const uint8_t* indices, int64_t indices_bytes, int n, int h, int w, void* workspace, int64_t workspace_bytes,
                    int64_t* offsets, int64_t offsets_elems, int32_t* err, void* stream);
int sdt_gif_pack(const void* workspace, int64_t workspace_bytes, int n, int h, int w, const int64_t* offsets, int64_t offsets_elems,
                 uint8_t* out, int64_t out_bytes, int32_t* err, void* stream);

/*
 * Clip preparation for a custom speaker (data_preprocess/2_2_remove_outlier.py, 2_3_rescale_shoulder_width.py and
 * 3_1_generate_clips.py of the reference; DESIGN.md section 16 is the contract).  One video at a time: src is its (n_frames, 3, 137)
 * keypoint array in float32 (elem_bytes 4) or float64 (8), present (n_frames uint8) marks the frames whose file exists.  Every
 * floating-point operation is rounded on its own, nothing is accumulated with atomics: the same bits on every call.
 *   frame_flags: keep[f] = present and no keypoint of 0, 2..7, 15, 16, 25..136 with x <= 3 and y <= 3 (compared in the element
 *     type); dist[f] = sqrt((x2-x5)^2 + (y2-y5)^2) in float64 (0 for a dropped frame); bad[f] = a kept frame with a non-finite x / y.
 *   scan: prefix (n_frames + 1 int32) = exclusive prefix sum of keep; dist_kept (n_frames) = the kept frames' dist, packed in order.
 *   shoulder_means: means[c] = avg = avg*(num/(num+1)) + (1 - num/(num+1))*d over kept frames [c*stride, (c+1)*stride),
 *     stride = prefix[n_frames] / chunks, in float64.
 *   windows: starts = the s of range(start_frame, n_frames - num_frames, step) whose num_frames frames are all kept, ascending;
 *     n_clips (device int32) their count.  sdt_clip_window_candidates = len(range(...)) is the capacity starts needs (negative:
 *     unsupported sizes); workspace: sdt_clip_workspace_bytes(n_frames) bytes (negative: unsupported), written before it is read.
 *   gather_poses: out (n_clips, num_frames, 3, 137) in the element type = src[starts[c] + i] with rows 0 and 1 (and row 2 if
 *     scale_confidence) multiplied by scalar converted to the element type.
 *   pcm_to_mono_f32: fmt 0 uint8 ((v - 128) / 128), 1 int16 (/ 2^15), 2 int32 (/ 2^31), 3 float32; interleaved frames
 *     [first, n_samples) -> out, the channels (at most 8) averaged in float32.
 *   resample_f32: y[j] = float32(sum_q taps[k0 + up*q] * x[t/up - q]), t = (j + n_pre_remove)*down, k0 = t % up, products and sums
 *     in float64 in ascending q, x zero outside [0, n_in).  sdt_clip_resample_lds_bytes: the launch's LDS (negative: unsupported
 *     filter length / ratio).
 *   gather_audio: out (n_clips, l_max) = audio[a0[c] : a1[c]] clamped to the track, zero after its end; lengths[c] the slice length.
 * No allocation; every pointer but scalar arguments is a device buffer; every index is checked against the sizes given.
 */
int64_t sdt_clip_workspace_bytes(int64_t n_frames);
int sdt_clip_frame_flags(int elem_bytes, const void* src, const void* present, int64_t n_frames, int32_t* keep, double* dist, int32_t* bad,
                         void* stream);
int sdt_clip_scan(const int32_t* keep, const double* dist, int64_t n_frames, int32_t* prefix, double* dist_kept, void* stream);
int sdt_clip_shoulder_means(const double* dist_kept, const int32_t* prefix, int64_t n_frames, int chunks, double* means, void* stream);
int64_t sdt_clip_window_candidates(int64_t n_frames, int start_frame, int num_frames, int step);
int sdt_clip_windows(const int32_t* prefix, int64_t n_frames, int start_frame, int num_frames, int step, void* workspace,
                     int64_t workspace_bytes, int32_t* starts, int64_t starts_capacity, int32_t* n_clips, void* stream);
int sdt_clip_gather_poses(int elem_bytes, const void* src, int64_t n_frames, const int32_t* starts, int64_t n_clips, int num_frames,
                          double scalar, int scale_confidence, void* out, int64_t out_elems, void* stream);
int sdt_clip_pcm_to_mono_f32(int fmt, const void* pcm, int64_t n_samples, int channels, int64_t first, float* out, int64_t out_elems,
                             void* stream);
int64_t sdt_clip_resample_lds_bytes(int n_taps, int up, int down);
int sdt_clip_resample_f32(const float* x, int64_t n_in, const double* taps, int n_taps, int up, int down, int64_t n_pre_remove, float* y,
                          int64_t n_out, void* stream);
int sdt_clip_gather_audio(const float* audio, int64_t n_audio, const int64_t* a0, const int64_t* a1, int64_t n_clips, int64_t l_max,
                          float* out, int64_t out_elems, int32_t* lengths, void* stream);

/*
 * Repair of short keypoint dropouts and spikes, an opt-in stage in front of sdt_clip_frame_flags (DESIGN.md section 26 is the contract).
 * Out of place: src (n_frames, 3, 137) and present are read, src_r (same shape and element type, another buffer) and present_r are
 * written.  Supported sizes: 1 <= n_frames <= 2^30 (as sdt_clip_workspace_bytes), 0 <= half <= 3, 1 <= max_gap <= 64, 1 <= num_frames
 * <= 2^24; outside them the size query is negative and the entry points return SDT_ERR_UNSUPPORTED before any launch.  Every float64
 * operation is rounded on its own, no atomics: the same bits on every call.  All 137 keypoints take part.
 *   valid: valid0[f, k] = present[f] and x, y finite and not (x <= 3 and y <= 3), compared in the element type.  With half >= 1 a valid0
 *     point is a spike iff, per coordinate over the m >= 3 valid0 points of frames f-half..f+half of its track (clipped to the video),
 *     |v - med| > kappa * (1.4826 * mad) + floor_px in x or in y, med = 0.5 * (s[(m-1)/2] + s[m/2]) of the ascending values, mad the
 *     same median of |s - med|, in float64.  valid = valid0 and not spike; valid and spike are (n_frames, 137) uint8.
 *   fill: an invalid point with valid frames a < f < b nearest on its track and b - a - 1 <= max_gap becomes
 *     xa + (xb - xa) * ((f - a) / (b - a)) in float64, rounded once to the element type (x and y), confidence 0, filled[f, k] = 1;
 *     every other element is copied.  repaired_per_frame[f] = filled keypoints of f among 0, 2..7, 15, 16, 25..136;
 *     present_r[f] = present[f] or that count is 121.
 *   clip_counts: repaired_per_clip[c] = sum of repaired_per_frame over [starts[c], starts[c] + num_frames), through an int64 prefix sum
 *     in workspace (sdt_clip_repair_workspace_bytes(n_frames) bytes, written before it is read).
 */
int64_t sdt_clip_repair_workspace_bytes(int64_t n_frames);
int sdt_clip_repair_valid(int elem_bytes, const void* src, const void* present, int64_t n_frames, int half, double kappa, double floor_px,
                          uint8_t* valid, uint8_t* spike, void* stream);
int sdt_clip_repair_fill(int elem_bytes, const void* src, const void* present, const uint8_t* valid, int64_t n_frames, int max_gap, void* src_r,
                         uint8_t* present_r, uint8_t* filled, int32_t* repaired_per_frame, void* stream);
int sdt_clip_repair_clip_counts(const int32_t* repaired_per_frame, int64_t n_frames, const int32_t* starts, int64_t n_clips, int num_frames,
                                void* workspace, int64_t workspace_bytes, int32_t* repaired_per_clip, void* stream);

/*
 * Retiming of keypoints recorded at fps_num / fps_den frames per second onto the 15 fps grid, an opt-in stage in front of the repair
 * stage (DESIGN.md section 27 is the contract).  Out of place: src (n_src, 3, 137) and present are read, src_t (n_out, 3, 137, same
 * element type, another buffer) is written.  With D = 15 * fps_den and g = gcd(fps_num, D): n_out = (n_src - 1) * D / fps_num + 1, and
 * output frame j has a = j * fps_num / D, r = j * fps_num % D (int64; no floating-point time) and reads row r / g of taps
 * (n_phases = D / g rows of n_taps float64, designed on the host): tap i weighs source frame a + 1 - n_taps / 2 + i; a tap of weight 0
 * takes part in nothing.  A source point is valid as in sdt_clip_repair_valid's valid0; a frame outside [0, n_src) is invalid.
 * Per output point, over the non-zero taps with a valid source point in ascending i, in float64, every operation rounded on its own:
 * num = sum h * v for x, y and the confidence, den = sum h; full = sum h over all non-zero taps of the row.  The point is valid iff
 * den > 0 and den >= min_support * full, and is then num / den rounded once to the element type, else (0, 0, 0).
 *   valid_t, taps_used (n_out, 137) uint8: the verdict and the number of taps that took part; present_t (n_out) uint8: a source frame
 *   under a non-zero tap has a file; nearest_src (n_out) int32 = min(a + (2 r >= D), n_src - 1); counts (3 int64) = invalid source
 *   points, source points with a non-finite x or y, invalid output points (integer block counts in workspace, summed by one workgroup).
 * Supported: 1 <= fps_num <= 2^20, 1 <= fps_den <= 2^16, 1 <= fps_num / fps_den <= 240, n_phases <= 16384, n_taps even in [2, 32],
 * n_src and n_out in [1, 2^30], min_support in (0, 1]; outside them the size query is negative and the entry point returns
 * SDT_ERR_UNSUPPORTED before any launch.  No atomics: the same bits on every call.
 */
int64_t sdt_clip_retime_workspace_bytes(int64_t n_src, int64_t fps_num, int64_t fps_den, int n_phases, int n_taps);
int sdt_clip_retime(int elem_bytes, const void* src, const void* present, int64_t n_src, int64_t fps_num, int64_t fps_den, const double* taps,
                    int n_phases, int n_taps, double min_support, int64_t n_out, void* src_t, uint8_t* present_t, uint8_t* valid_t,
                    uint8_t* taps_used, int32_t* nearest_src, int64_t* counts, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * Audio activity gate, an opt-in stage between the window search and the gathers (DESIGN.md section 28 is the contract; no counterpart in
 * the reference).  audio is the video's cut 16 kHz float32 track of n_samples; a hop is 160 samples, n_hops = n_samples / 160, the tail
 * is ignored.  float64 with every operation rounded on its own, no floating-point atomics, integers after the threshold: the same bits
 * on every call.
 *   energy: e[h] = sum over the hop of d^2, d[n] = x[n] - (31/32) x[n-1], x[-1] = 0.  Lane l of 64 adds samples l, l + 64, l + 128
 *     (below 160) of the hop in that order from +0.0, then the xor butterfly 32, 16, 8, 4, 2, 1.  flag (device int32; zeroed first) is set
 *     when an e[h] is not finite.
 *   mask: stats[0] = f = the energy of rank floor_pct * (n_hops - 1) / 100 in ascending order (an exact radix select on the bit patterns),
 *     stats[1] = thr = f * margin if that is greater than abs_floor, else abs_floor (the product rounded once);
 *     active_raw[h] = e[h] > thr (uint8).  n_hops = 0: stats = (0, 0).
 *   smooth: (a) every maximal run of active hops shorter than min_run_hops becomes inactive; then (b) every maximal run of inactive hops
 *     of length <= hang_hops with an active hop on both sides becomes active (runs that touch an end of the track are not filled).  0
 *     disables a rule.  active must not alias active_raw.
 *   windows: prefix (n_hops + 1 int32) = exclusive prefix sum of active.  For candidate window i (starts[i], ascending, with its audio
 *     span a0[i], a1[i] in samples; a1 is clipped to n_samples, a0 below 0 to 0): n_h = the hops with 160 h >= a0 and 160 (h + 1) <= a1,
 *     c = the active ones; counts_all (n_windows, 2 int32) = (c, n_h).  Kept iff n_h > 0 and 1000 c >= min_permille n_h (int64).
 *     starts_kept, index_kept (the i) and counts_kept (n_kept, 2) list the kept windows in ascending order (capacity n_windows each);
 *     n_kept (device int32) their number.
 * Supported: 0 <= n_samples <= 160 * 2^24 + 159, 0 <= n_windows <= 2^30, floor_pct in [0, 50], min_run_hops and hang_hops in [0, 1024],
 * min_permille in [1, 1000]; outside them sdt_clip_speech_workspace_bytes is negative and the entry points return SDT_ERR_UNSUPPORTED
 * before any launch.  workspace: sdt_clip_speech_workspace_bytes(n_samples, n_windows) bytes serve every entry point; written before
 * it is read.  No allocation; every index is checked against the sizes given.
 */
int64_t sdt_clip_speech_workspace_bytes(int64_t n_samples, int64_t n_windows);
int sdt_clip_speech_energy(const float* audio, int64_t n_samples, double* energy, int32_t* flag, void* stream);
int sdt_clip_speech_mask(const double* energy, int64_t n_hops, int floor_pct, double margin, double abs_floor, uint8_t* active_raw,
                         double* stats, void* workspace, int64_t workspace_bytes, void* stream);
int sdt_clip_speech_smooth(const uint8_t* active_raw, int64_t n_hops, int min_run_hops, int hang_hops, uint8_t* active, void* workspace,
                           int64_t workspace_bytes, void* stream);
int sdt_clip_speech_windows(const uint8_t* active, int64_t n_hops, int64_t n_samples, const int32_t* starts, const int64_t* a0,
                            const int64_t* a1, int64_t n_windows, int min_permille, int32_t* prefix, int32_t* counts_all,
                            int32_t* starts_kept, int32_t* index_kept, int32_t* counts_kept, int32_t* n_kept, void* workspace,
                            int64_t workspace_bytes, void* stream);

/*
 * Optimiser-side safeguards of the flat-buffer Adam (no counterpart in the reference): gradient-norm clipping as
 * torch.nn.utils.clip_grad_norm_(norm_type=2, error_if_nonfinite=False), a step that a non-finite gradient cannot poison, and an
 * exponential moving average of the parameters.  No atomics, no host read-back: hipGraph-capturable like the rest.
 *   grad_sumsq_f64: partial[0] = sum of the float64 squares of g[0..n) in ONE fixed order (csrc/optim_guard.hip states it;
 *     optim.sumsq_model is the same order in numpy, bit for bit); partial: sdt_grad_sumsq_partials() doubles, contents irrelevant.
 *     Non-finite exactly when an element of g is.  g 16-byte aligned.
 *   optim_guard_prep: partials = HOST array of n_buffers (1..4) device partial buffers, summed in argument order.  Writes the guard
 *     record, 32 device bytes {double norm; float scale; int32 skip; int64 skipped; int64 reserved} zero-initialised by the caller:
 *     norm = grad_scale * sqrt(sum); scale = (float)(grad_scale * coef), coef = min(max_norm / (norm + 1e-6), 1) in float64 (a NaN
 *     stays a NaN), coef = 1 when max_norm <= 0; skip = skip_nonfinite and norm is not finite; skipped += skip.
 *   adam_step_guarded_f32: sdt_adam_step_f32 with grad_scale read from the record.  skip set: nothing is written -- p, m, v, ema and
 *     state_dev keep their bits.  ema != NULL: ema = ema_decay * ema + (1 - ema_decay) * p_new in the same pass (ema_decay in (0, 1)).
 *   optim_guard_pass_elems: elements one grid pass of the launch as built covers (0: the sum of squares, 1: the guarded Adam step).
 */
int64_t sdt_grad_sumsq_partials(void);
int64_t sdt_optim_guard_pass_elems(int which);
int sdt_grad_sumsq_f64(const float* g, int64_t n, double* partial, void* stream);
int sdt_optim_guard_prep(const double* const* partials, int n_buffers, float grad_scale, double max_norm, int skip_nonfinite,
                         void* guard, void* stream);
int sdt_adam_step_guarded_f32(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1, float beta2,
                              float eps, float weight_decay, const void* guard, float* ema, float ema_decay, void* state_dev,
                              void* stream);

/*
 * Per-tensor histograms and moments of a flat fp32 buffer, one segmented pass (tensor_hist.py; DESIGN.md section 20 is the contract;
 * no counterpart in the reference, which calls SummaryWriter.add_histogram per parameter).  A segment is {offset, numel} in elements of
 * flat[0..n): offset a multiple of 4, offset + numel <= n (else SDT_ERR_ARG).  Supported sizes: 1 <= n_segments <= 65536
 * (sdt_tensor_hist_max_segments), numel < 2^32 per segment, at most 2^24 chunks of sdt_tensor_hist_chunk() elements in all; outside them
 * both entry points return SDT_ERR_UNSUPPORTED.  Elements outside every segment are never read into a result.
 *   plan (host only, no GPU): segments = HOST (n_segments, 2) int64 -> seg_plan HOST (n_segments, 3) {offset, numel, first chunk},
 *     chunk_plan HOST (chunk_rows, 2) {segment, chunk number}, *n_chunks = rows used.  seg_plan / chunk_plan may be NULL (size query).
 *   f32: seg_plan, chunk_plan = DEVICE copies of the plan; every row is checked again on the device against n_segments, n and n_chunks.
 *     edges = DEVICE n_edges = 1549 ascending float64 bucket edges (edges[774] == 0).  Every element is v = (float)(x * scale), widened
 *     to float64.  Zeroes and fills counts (n_segments, 1548) int64: bucket i = [edges[i], edges[i + 1]) by float64 compares, finite
 *     values beyond the table in the outermost bucket of their sign; tallies (n_segments, 3) int64 {finite, NaN, +-inf}; stats
 *     (n_segments, 4) float64 {min, max, sum, sum of squares} over the finite elements (none: +inf, -inf, +0, +0).  The sums have one
 *     fixed order (csrc/tensor_hist.hip states it; tensor_hist.model_histograms is the same order in numpy, bit for bit); the integer
 *     results use integer atomics and are exact.  partials: 4 * n_chunks doubles, contents irrelevant.  flat 16-byte aligned.
 */
int64_t sdt_tensor_hist_threads(void);
int64_t sdt_tensor_hist_chunk(void);
int64_t sdt_tensor_hist_buckets(void);
int64_t sdt_tensor_hist_max_segments(void);
int sdt_tensor_hist_plan(const int64_t* segments, int n_segments, int64_t n, int64_t* seg_plan, int64_t* chunk_plan, int64_t chunk_rows,
                         int64_t* n_chunks);
int sdt_tensor_hist_f32(const float* flat, int64_t n, const int64_t* seg_plan, int n_segments, const int64_t* chunk_plan, int64_t n_chunks,
                        const double* edges, int n_edges, float scale, int64_t* counts, int64_t* tallies, double* stats, double* partials,
                        void* stream);

/*
 * Per-clip validation metrics on final float64 poses (TEST.CLIP_METRICS; speechdrivestemplates_amd/clip_metrics.py; DESIGN.md section 22 is
 * the contract, clip_metrics.clip_metrics_model / epoch_model are the same operations in numpy).  pred / gt: (R, T, 2, K) float64, parts: K
 * bytes in {0, 1, 2} (body, face, hands); part index p = 0 is "all", p = 1 + byte.  Every multiply, add and subtract is rounded on its own
 * (csrc/exact_f64.h); no floating-point atomics.  No allocation; every pointer except ``alphas``, ``part_sizes`` and ``tables`` (host arrays,
 * read during the call) is a device buffer; every size is checked before the launch.
 *   A record is 40 words of 8 bytes: float64 [0,4) l2_sum[p], [4,8) speed_pred[p], [8,12) speed_gt[p], [12,16) vel_l2[p], [16,20) div_sum[p];
 *   int64 [20,36) pck_hit[a * 4 + p] (a >= A: 0), 36 seen, 37 copies, 38 nonfinite, 39 frames.
 *   rows: one record per row (div_sum 0, seen 1, copies 1) into rows (R x 40 words); work: R * T * 32 words, contents irrelevant.  Within a
 *     frame lane k holds keypoint k's term (0 outside the part) and the 128 lanes are combined by the xor butterfly 32, 16, 8, 4, 2, 1 inside
 *     each wave, then wave 0 + wave 1; the frames of a row are added in frame order.  K in [1, 128], T >= 1, A in [1, 4].
 *   diversity: row j * B + b is copy j of clip b, m in [2, 16]; lane k adds its pair terms in lexicographic (i, j) order, the butterfly
 *     combines the lanes; divwork: B * T * 4 float64 (per (clip, frame), summed over t in order by commit).
 *   commit: the m row records of clip b added in order j = 0..m-1, div_sum from divwork (NULL with m = 1), into row clip_index[b] of table,
 *     (N + 1) x 40 words: row N is the header, whose word 0 counts the indices outside [0, N) (they write nothing else).  Two entries of one
 *     call with the same index: either may win.
 *   epoch: tables are ranks (1..64) table pointers; clip n takes the record of the lowest rank with seen set, records with nonfinite set are
 *     left out and counted.  Columns are summed in chunks of 64 clips in index order, then the chunk partials in order.  work:
 *     ceil(N / 64) * 48 words.  out (40 words): float64 [0,4) L2[p], [4,20) PCK[a * 4 + p], [20,24) mean over the alphas of PCK[.][p],
 *     [24,28) sum speed_pred[p] / sum speed_gt[p], [28,32) vel_L2[p], [32,36) diversity[p]; int64 36 clips with a record, 37 of them left
 *     out as nonfinite, 38 index errors of all tables, 39 the number of (pair, frame) terms behind diversity.  A quotient whose divisor is 0
 *     is 0.0.  part_sizes: 4 int64 {K, body, face, hands}.
 *   sqrt: y[i] = sqrt(x[i]) as the kernels above compute it (the tests ask it whether this device's square root is correctly rounded).
 */
#define SDT_CLIP_METRICS_COLS 40
int sdt_clip_metrics_rows_f64(const double* pred, const double* gt, const uint8_t* parts, const double* alphas, int num_alphas, int R, int T,
                              int K, void* work, void* rows, void* stream);
int sdt_clip_metrics_diversity_f64(const double* pred, const uint8_t* parts, int B, int m, int T, int K, double* divwork, void* stream);
int sdt_clip_metrics_commit(const void* rows, const double* divwork, const int64_t* clip_index, int B, int m, int T, void* table, int64_t N,
                            void* stream);
int sdt_clip_metrics_epoch(const void* const* tables, int ranks, int64_t N, const int64_t* part_sizes, int num_alphas, void* work, void* out,
                           void* stream);
int sdt_clip_metrics_sqrt_f64(const double* x, int64_t n, double* y, void* stream);

/*
 * Whole-recording demo (DEMO.LONG_FORM; speechdrivestemplates_amd/long_demo.py; DESIGN.md section 23 is the contract, long_demo.stitch_model /
 * smooth_model / report_model are the same operations in numpy; no counterpart in the reference, which runs a demo as one sequence).
 * Layout, integers only: W frames per window, overlap O with 0 <= 2 O <= W, H = W - O, F >= W frames in all, N = 1 + ceil((F - W) / H)
 * windows starting at s_i = i H (i < N - 1) and s_{N-1} = F - W; at most three windows cover a frame and they are visited in ascending i.
 * K in [1, 128], W >= 2; any other size, or an N that does not match, returns SDT_ERR_ARG before any launch.  No allocation, no host
 * synchronisation, no atomics; every pointer except ``coeffs`` and ``part_sizes`` (host arrays, read during the call) is a device buffer.
 * Every multiply, add, subtract and divide is rounded on its own (csrc/exact_f64.h).
 *   gather: out (n, Lw) float32, out[i][j] = audio[offsets[i] + j], 0.0f where that index is outside [0, L).  offsets: n int64 on the device.
 *   stitch: windows (N, W, 2, K) float64 -> out (F, 2, K).  u_i(t) = min(t - s_i + 1, s_i + W - t), w_i(t) = min(u_i(t), max(O, 1)).  A frame
 *     that one window covers is that window's value bit for bit; otherwise (w_a x_a + w_b x_b [+ w_c x_c]) / (w_a + w_b [+ w_c]) with the
 *     products added in ascending window order starting from the first product, and the integer weight sum converted exactly.
 *   smooth: y(t) = sum over j = -m .. m of coeffs[j + m] * x(clamp(t + j, 0, F - 1)), j ascending, starting from the first product.  x, y:
 *     (F, 2, K) float64, F >= 1, m in [1, 8], y != x.
 *   report: parts = K bytes in {0, 1, 2} (body, face, hands), part index p = 0 is "all", p = 1 + byte; part_sizes = 4 int64 {K, body, face,
 *     hands}; smoothed may be NULL.  out = 40 words of 8 bytes: float64 [0,4) speed[p] and [4,8) jerk[p] of the stitched poses, [8,12) and
 *     [12,16) the same of the smoothed poses (0.0 without them), [16,20) seam[p]; int64 [20,24) / [24,28) / [28,32) the number of terms behind
 *     speed / jerk / seam per part, 32 nonfinite (a sum is not finite), 33 F, 34 N, 35 smoothed given, 36 the number of (frame, window pair)
 *     terms, 37..39 zero.  speed is the mean over (t < F - 1, k in p) of |x(t + 1) - x(t)|, jerk the mean over (t < F - 3, k in p) of
 *     |((x(t + 3) - 3 x(t + 2)) + 3 x(t + 1)) - x(t)|, seam the mean over the frames with two or more covering windows, their pairs i < j and
 *     k in p of |x_i(t) - x_j(t)|; a quotient whose divisor is 0 is 0.0.  Within a frame lane k holds keypoint k's term (0 outside the
 *     part; the pair terms of a keypoint are added in lexicographic (i, j) order first) and the 128 lanes are combined by the xor butterfly
 *     32, 16, 8, 4, 2, 1 inside each wave, then wave 0 + wave 1; the frames are added in chunks of 64 in ascending order, then the chunk
 *     partials in order.  work: sdt_long_report_workspace_bytes(F) bytes (-1 for an F outside [1, 2^24]), contents irrelevant.
 */
#define SDT_LONG_REPORT_COLS 40
int sdt_long_windows_gather_f32(const float* audio, int64_t L, const int64_t* offsets, int n, int Lw, float* out, void* stream);
int sdt_long_stitch_f64(const double* windows, int N, int W, int O, int F, int K, double* out, void* stream);
int sdt_long_smooth_f64(const double* x, int F, int K, const double* coeffs, int m, double* y, void* stream);
int64_t sdt_long_report_workspace_bytes(int F);
int sdt_long_report_f64(const double* windows, const double* stitched, const double* smoothed, const uint8_t* parts, const int64_t* part_sizes,
                        int N, int W, int O, int F, int K, void* work, void* out, void* stream);

/*
 * Speech-gesture synchrony (TEST.SYNC_METRICS; speechdrivestemplates_amd/sync_metrics.py; DESIGN.md section 24 is the contract, sync_metrics.
 * onsets_model / beats_model / match_model / sync_model / epoch_model are the same operations in numpy; no counterpart in the reference).
 * Times are integers in ticks of 1/300 s at 16000 samples/s and 15 frames/s: an audio hop of 160 samples is 3 ticks, a pose frame 20.  Every
 * multiply, add, subtract and divide is rounded on its own (csrc/exact_f64.h); no floating-point atomics, no allocation, no host
 * synchronisation; every pointer except ``tables`` (a host array, read during the call) is a device buffer; every size is checked before
 * the launch (K in [1, 128], tol in [1, 150], T in [1, 2^24], L in [0, 160 * 2^28]; otherwise SDT_ERR_ARG).
 *   onsets: audio (B, L) float32.  Nf = L / 160 frames, frame n covers samples [160 n, 160 n + 320), 0.0 at or past L.  e[n] = sqrt(sum x^2):
 *     lane l of a wave adds the squares of samples l, l + 64, .., l + 256 in that order (the first product starts the sum), then the xor
 *     butterfly 32 .. 1.  o[0] = 0, o[n] = e[n] - e[n-1] where that is > 0, else 0.  Frame 1 <= n <= Nf - 2 is a candidate if o[n] > o[n-1],
 *     o[n] >= o[n+1], o[n] > delta * mean (the sum of o over [n-15, n+15] clipped to the clip, ascending from +0.0, divided by the count) and
 *     o[n] > floor_frac * max e.  Candidates are accepted left to right; one fewer than 8 frames after the last accepted one is dropped.
 *     ticks (B, cap) int32: 3 n + 3 of the accepted frames, ascending; cap >= sdt_sync_onset_capacity(L) = Nf / 8 + 1.  info (B, 2) int64:
 *     the number of onsets, and 1 if an e[n] is not finite.  work: e (B, Nf) then o (B, Nf) float64.
 *   rows: poses (R, T, 2, K) float64, parts K bytes in {0, 1, 2}; part index p = 0 is "all", p = 1 + byte.  Row r belongs to clip r % B of
 *     ticks / info.  s_p[t] (t < T - 1) = sum over k in p of |x(t+1) - x(t)|, formed as sdt_clip_metrics_rows_f64 forms speed_pred.  t in
 *     [1, T - 3] is a beat of part p if s[t] > s[t-1], s[t] >= s[t+1] and s[t] > gamma * (sum of s in order from +0.0) / (T - 1); its tick is
 *     20 t + 10, d = min(distance to the nearest onset tick, 150) (150 without onsets).  A row record is SDT_SYNC_ROW_COLS words of 8 bytes:
 *     float64 [0,4) align[p] = sum of gauss[d] in beat order from +0.0 (gauss: 151 float64); int64 [4,8) beats[p], [8,12) hits[p] (d <= tol),
 *     [12,16) dsum[p], [16,20) covered[p] (onsets with a beat of part p within tol), 20 onsets, 21 nonfinite (a speed sum or an e[n] is not
 *     finite), 22 T, 23 zero.  work: s (R, T - 1, 4) float64, then the beat flags (R, 4, T) bytes.
 *   sdt_sync_workspace_bytes(B, L, R, T): bytes of the larger of the two work buffers (-1 for a size outside the ranges).
 *   commit: clip b's record = the sum over its m copies (rows j * B + b, j ascending) of the prediction's and the ground truth's row records
 *     (rows_gt may be NULL: zeros), into row clip_index[b] of table, (N + 1) x SDT_SYNC_COLS words; row N is the header, whose word 0 counts
 *     the indices outside [0, N).  A clip record: float64 [0,4) align_pred[p], [4,8) align_gt[p]; int64 [8,24) beats, hits, dsum, covered of
 *     the prediction (4 words each), [24,40) of the ground truth, 40 onsets (summed over the copies), 41 seen, 42 copies, 43 nonfinite, 44 T,
 *     45 Nf, 46..47 zero.
 *   epoch: as sdt_clip_metrics_epoch: the lowest rank with seen set gives clip n's record, nonfinite records are left out and counted,
 *     chunks of 64 clips in index order, then the chunk partials in order; work: ceil(N / 64) * SDT_SYNC_COLS words.  out is
 *     SDT_SYNC_OUT_COLS words: float64 pairs {all, hands} 0 precision = hits / beats, 2 precision_gt, 4 recall = covered / onsets, 6 recall_gt,
 *     8 offset_ms = dsum * (1000 / 300) / beats, 10 beat_align = align / beats, 12 beat_align_gt, 14 beats * 15 / sum(copies * T), 16 the
 *     same of the ground truth, 18 onsets * 100 / sum(copies * Nf), 19 zero; int64 20 clips with a record, 21 of them left out as nonfinite,
 *     22 index errors of all tables, 23 zero.  A quotient whose divisor is 0 is 0.0.
 */
#define SDT_SYNC_ROW_COLS 24
#define SDT_SYNC_COLS 48
#define SDT_SYNC_OUT_COLS 24
int64_t sdt_sync_onset_capacity(int64_t L);
int64_t sdt_sync_workspace_bytes(int B, int64_t L, int R, int T);
int sdt_sync_onsets_f64(const float* audio, int B, int64_t L, double delta, double floor_frac, void* work, int32_t* ticks, int64_t cap,
                        int64_t* info, void* stream);
int sdt_sync_rows_f64(const double* poses, const uint8_t* parts, int R, int T, int K, int B, const int32_t* ticks, int64_t cap,
                      const int64_t* info, const double* gauss, int tol, double gamma, void* work, void* rows, void* stream);
int sdt_sync_commit(const void* rows_pred, const void* rows_gt, const int64_t* clip_index, int B, int m, int T, int64_t L, void* table, int64_t N,
                    void* stream);
int sdt_sync_epoch(const void* const* tables, int ranks, int64_t N, void* work, void* out, void* stream);

/*
 * Audio augmentation inside the train step (TRAIN.AUGMENT; speechdrivestemplates_amd/augment.py; DESIGN.md section 25 is the contract, augment.
 * philox4x32 / sumsq_model / clip_params_model / audio_model / mel_mask_model are the same operations in numpy; no counterpart in the
 * reference).  Random words are Philox4x32-10 (multipliers D2511F53 / CD9E8D57, Weyl constants 9E3779B9 / BB67AE85) with the key (seed low
 * 32 bits, seed high 32 bits) and the counter (block j, purpose, clip_index[b] low 32 bits, step[0] low 32 bits): nothing depends on the
 * clip's row, on B or on the rank.  Purpose 0: block 0 gives the clip's parameters from its words w0 .. w3, blocks 1 .. nf the frequency
 * masks, blocks 5 .. 4 + nt the time masks.  Purpose 1: noise sample n takes block n >> 1, words 2 (n & 1) and 2 (n & 1) + 1.  No
 * transcendental function, no allocation, no host synchronisation, no atomics; clip_index (B,) and step (1,) are int64 device buffers read
 * by the kernels, so a captured graph follows them; every size is checked before the launch (B in [1, 65535], L in [1, 2^24]; otherwise
 * SDT_ERR_ARG).  Every float64 multiply, add and divide is rounded on its own (csrc/exact_f64.h).
 *   sumsq: audio (B, L) float32 -> ss (B,) float64, the sum of the squares (each exact in float64) in this order: chunk c covers samples
 *     [1024 c, 1024 c + 1024); thread t of 256 adds the squares of samples 1024 c + t + 256 k, k = 0 .. 3, from +0.0 (+0.0 at or past L);
 *     the xor butterfly 32, 16, 8, 4, 2, 1 inside each of the four waves; ((wave 0 + wave 1) + wave 2) + wave 3 is the chunk's partial.
 *     Then lane l adds the partials l, l + 64, .. from +0.0 and the same butterfly follows.  work: sdt_augment_workspace_bytes(B, L) bytes
 *     (-1 for a size outside the ranges), contents irrelevant.
 *   audio: out (B, L) float32, out != audio.  Per clip, from block 0: ig = w0 >> 24, g = gain_table[ig] (256 float32), negated when
 *     polarity and w3 & 1; is = w1 >> 24, a = snr_table[is] (256 float64); s = (w2 mod (2 max_shift + 1)) - max_shift; the noise is on iff
 *     (w3 >> 8) < noise_prob24 (0 .. 2^24); sigma = sqrt(ss[b] / L) * a with the noise on, else 0.0.  x_s[n] = audio[b][n - s] inside
 *     [0, L), else +0.0.  z[n] = (h0 + h1 + h2 + h3 - 131070) * 0x1.bb67ae86627e7p-16 over the four 16-bit halves of the sample's two words
 *     (the integer converts exactly).  out[b][n] = float32(float64(g) * (float64(x_s[n]) + sigma * z[n])) with the noise on and
 *     float32(float64(g) * float64(x_s[n])) with it off (no noise term is formed, so a -0.0 keeps its sign).  One read and one write of the
 *     audio; the elements before the first 16-byte boundary of an output row and the last L' mod 4 are written one by one, the rest by
 *     16-byte stores; no read or write outside a row.  rec (B, SDT_AUGMENT_REC_COLS) words of 8 bytes: int64 0 ig, 1 is, 2 s, 3 polarity,
 *     4 noise on, float64 5 sigma, 6 ss, int64 7 nonfinite (ss is not finite: a NaN or inf sits in that clip, and only that clip's output
 *     is affected), 8 .. 31 zero.
 *   mel mask: mel (B, M, F) float32, in place.  Mask i of a dimension of size D (M for a frequency band, F for a time span) and largest
 *     width w: width = w0 mod (w + 1), clipped to D; start = w1 mod (D - width + 1); the rectangle spans the whole other dimension and is
 *     set to +0.0; elements outside every rectangle are neither read nor written.  The moduli are biased by at most (w + 1) 2^-32 resp.
 *     D 2^-32.  rec words 8 + 2 i, 9 + 2 i: start, width of frequency mask i; 16 + 2 i, 17 + 2 i: of time mask i (0, 0 for i >= n);
 *     24 nf, 25 nt.  Words 0 .. 7 and 26 .. 31 are left as they are.
 */
#define SDT_AUGMENT_REC_COLS 32
int64_t sdt_augment_workspace_bytes(int B, int64_t L);
int sdt_augment_sumsq_f64(const float* audio, int B, int64_t L, void* work, double* ss, void* stream);
int sdt_augment_audio_f32(const float* audio, int B, int64_t L, const int64_t* clip_index, const int64_t* step, const double* ss, uint64_t seed,
                          int64_t max_shift, int64_t noise_prob24, int polarity, const float* gain_table, const double* snr_table, void* rec,
                          float* out, void* stream);
int sdt_augment_mel_mask_f32(float* mel, int B, int M, int F, const int64_t* clip_index, const int64_t* step, uint64_t seed, int nf, int wf, int nt,
                             int wt, void* rec, void* stream);

/*
 * Pose augmentation inside the train step (TRAIN.POSE_AUGMENT; speechdrivestemplates_amd/pose_augment.py; DESIGN.md section 30 is the
 * contract, pose_augment.params_model / pose_model are the same operations in numpy; no counterpart in the reference): a left/right mirror
 * about the neck, a per-clip uniform scale and a per-clip in-plane rotation about the neck.  One Philox4x32-10 block per clip (the generator of
 * the audio augmentation above): key (seed low 32 bits, seed high 32 bits), counter (0, purpose 2, clip_index[b] low 32 bits, step[0] low
 * 32 bits -- 0 with per_clip).  mirror = (w0 >> 8) < mirror_prob24 (0 .. 2^24); is = w1 >> 24, s = scale_table[is] (256 float64);
 * ir = w2 >> 24, (c, sn) = rot_table[2 ir], rot_table[2 ir + 1] (256 float64 pairs); w3 is unused.  No transcendental function, no
 * allocation, no host synchronisation, no atomics, no scratch; clip_index (B,) and step (1,) are int64 device buffers read by the kernels,
 * so a captured graph follows them.  perm is a HOST array of K int32, the mirror partner of each keypoint: it is checked to be a
 * permutation of 0 .. K - 1 (else SDT_ERR_ARG) and travels to the kernel by value.  Sizes: K in [1, 128], B in [1, 65535], T in [1, 2^24],
 * n_clips in [1, 2^40]; anything else returns SDT_ERR_UNSUPPORTED before any launch.  Out of place: poses_out != poses, score_out != score.
 *   poses, poses_out (B, T, 2, K) float32 (x row, y row per frame); score_or_null, score_out the same shape (score_out unused without a
 *   score); mean, std (B, 2 K) float64 (x then y).  For keypoint k with m = perm[k] under mirror and m = k without, per frame, in float64 on
 *   values converted exactly from float32, every multiply, add, subtract and divide rounded on its own (csrc/exact_f64.h):
 *     dx = n_x[m] std_x[m] + mean_x[m], dy likewise; dx = -dx under mirror;
 *     (rx, ry) = (s dx, s dy) when c == 1 and sn == 0 (no rotation: the coordinates stay apart), else
 *     (rx, ry) = (s (c dx - sn dy), s (sn dx + c dy));
 *     out_x[k] = float32((rx - mean_x[k]) / std_x[k]), out_y[k] likewise.
 *   A clip whose transformation is the identity (no mirror, s == 1, c == 1, sn == 0) gets its input's bits instead.  score_out[.][k] =
 *   score[.][m] as bits.  eff_index[b] = clip_index[b] + n_clips * mirror.  A non-finite input element reaches only the outputs of the
 *   keypoint k with perm[k] = its keypoint, in its frame: its own coordinate, and both with a rotation on.
 *   rec (B, SDT_POSE_AUGMENT_REC_COLS) words of 8 bytes: int64 0 mirror, 1 is, 2 ir, float64 3 s, 4 c, 5 sn, int64 6 the effective index,
 *   7 identity.  One launch of a thread per clip, one of a thread per (frame, keypoint) with plain dword accesses (rows of 2 K floats are not
 *   16-byte aligned).
 */
#define SDT_POSE_AUGMENT_REC_COLS 8
int sdt_pose_augment_f32(const float* poses, const float* score_or_null, const double* mean, const double* std, int B, int T, int K,
                         const int64_t* clip_index, const int64_t* step, int64_t n_clips, uint64_t seed, int64_t mirror_prob24, int per_clip,
                         const int32_t* perm, const double* scale_table, const double* rot_table, float* poses_out, float* score_out,
                         int64_t* eff_index, void* rec, void* stream);

/*
 * Motion histograms and Hellinger distances at validation (TEST.MOTION_DIST; speechdrivestemplates_amd/motion_dist.py; DESIGN.md section 31
 * is the contract, motion_dist.motion_dist_model / epoch_model are the same operations in numpy; no counterpart in the reference).  pred / gt:
 * (R, T, 2, K) float64, parts: K bytes in {0, 1, 2} (body, face, hands); part index p = 0 is "all", p = 1 + byte; source s = 0 is the
 * prediction, 1 the ground truth; order o = 0, 1, 2 is speed, acceleration, jerk.  Differences are successive, each subtraction rounded on its
 * own: d1(t) = x(t+1) - x(t), d2(t) = d1(t+1) - d1(t), d3(t) = d2(t+1) - d2(t), per coordinate; order o has T - 1 - o terms per keypoint.
 * q = dx * dx + dy * dy, every operation rounded on its own (csrc/exact_f64.h); no floating-point atomics, no allocation, no host
 * synchronisation; every pointer except ``tables`` (a host array, read during the call) is a device buffer; every size is checked before the
 * launch (K in [1, 128], T in [1, 65536], m in [1, 16], m * T * K < 2^31; otherwise SDT_ERR_ARG).
 *   edges: (3, 2, 31) float64: per order the 31 ascending inner edges (> 0, finite), then their squares e * e as the host rounded them.  The
 *     bin of a term is the number of squared edges <= q (0 .. 31): a q equal to a squared edge belongs to the upper bin, +inf to bin 31; a NaN
 *     is counted nowhere and sets nonfinite.
 *   A record is SDT_MOTION_DIST_COLS = 316 words of 8 bytes: float64 [0,24) mag_sum[12 s + 4 o + p], the sum of sqrt(q); [24,312) the 576
 *     counts as int32 pairs: count i = ((3 s + o) * 3 + part) * 32 + bin (part 0 body, 1 face, 2 hands) sits in word 24 + i / 2, in the low 32
 *     bits for an even i and the high 32 bits for an odd one; int64 312 seen, 313 copies, 314 nonfinite (a NaN term, or a float sum that is
 *     not finite), 315 frames.
 *   rows: one record per row (seen 1, copies 1) into rows (R x 316 words).  One workgroup of four waves per row, two per source, lane k of a
 *     pair holds keypoint k; within a frame the lanes' sqrt terms (+0.0 outside the part) go through the xor butterfly 32, 16, 8, 4, 2, 1
 *     inside each wave, then wave 0 + wave 1; the frame sums of an order are added in frame order from +0.0.
 *   commit: the m row records of clip b (rows j * B + b) added in order j = 0..m-1 into row clip_index[b] of table, (N + 1) x 316 words: row
 *     N is the header, whose word 0 counts the indices outside [0, N) (they write nothing else).
 *   epoch: tables are ranks (1..64) table pointers; clip n takes the record of the lowest rank with seen set, records with nonfinite set are
 *     left out and counted.  Counts are summed exactly, float sums in chunks of 64 clips in index order, then the chunk partials in order;
 *     "all" is the sum of the three parts.  work: sdt_motion_dist_epoch_work_words(N) = ceil(N / 64) * 896 words.  For counts a_b, b_b with
 *     totals na, nb: BC = sum over b in order from +0.0 of sqrt((a_b / na) * (b_b / nb)), H = sqrt(max(1 - BC, +0.0)); both 0.0 if na or nb
 *     is 0.  out (SDT_MOTION_DIST_OUT_COLS = 64 words), index r = 4 o + p: float64 [0,12) H[r] and [12,24) BC[r] of the prediction against
 *     the ground truth, [24,36) H_floor[r] and [36,48) BC_floor[r] of the ground truth of the clips with an even index against that of the
 *     clips with an odd index, [48,60) ratio[r] = sum mag_sum_pred / sum mag_sum_gt (0.0 for a divisor of 0); int64 60 clips with a record,
 *     61 of them left out as nonfinite, 62 index errors of all tables, 63 zero.  hist: (2, 3, 4, 32) int64, the merged histograms
 *     [s][o][p][bin] with "all" filled in.
 *   The square root is the one sdt_clip_metrics_sqrt_f64 probes.
 */
#define SDT_MOTION_DIST_COLS 316
#define SDT_MOTION_DIST_OUT_COLS 64
int sdt_motion_dist_rows_f64(const double* pred, const double* gt, const uint8_t* parts, const double* edges, int R, int T, int K, void* rows,
                             void* stream);
int sdt_motion_dist_commit(const void* rows, const int64_t* clip_index, int B, int m, int T, int K, void* table, int64_t N, void* stream);
int64_t sdt_motion_dist_epoch_work_words(int64_t N);
int sdt_motion_dist_epoch(const void* const* tables, int ranks, int64_t N, void* work, void* out, void* hist, void* stream);

/*
 * Fitting template codes to clips with the generator held fixed (TEST.FIT_CODE; speechdrivestemplates_amd/code_fit.py; DESIGN.md section 32 is
 * the contract, code_fit.loss_model / step_model / set_model / pick_model are the same operations in numpy; no counterpart in the reference).
 * Everything of an iteration that is not the Conv1d chain or the head.  No floating-point atomics, no allocation, no host synchronisation;
 * every operation is rounded on its own except the three fused multiply-adds of the Adam update, which are the ones adam_kernel is compiled
 * to; every pointer is a device buffer; a clip reads and writes its own rows only.  Sizes are checked before the launch (SDT_ERR_ARG).
 *   loss: pred, gt (B, n) fp32.  loss[b] = (sum |double(pred) - double(gt)|) / double(n) in float64, NaN when the sum is not finite;
 *     dpred = sign(pred - gt) * float(1.0 / double(n)), sign(0) = 0, a NaN difference gives NaN.  One workgroup of 256 threads per clip:
 *     thread t adds the elements t, t + 256, ... in that order from +0.0; wave butterfly xor 32, 16, 8, 4, 2, 1; (w0 + w1) + (w2 + w3).
 *   step (mode 0), one wave per clip, D <= 256, in this order:
 *     1. loss[b] < best_loss[b] (never for a NaN): best_code[b] = code[b] -- the code that produced this loss -- and best_loss[b] = loss[b];
 *     2. g[d] = float(sum over t ascending from +0.0 of double(dh[b, t, C + d])), dh (B, T, C + D) fp32;
 *     3. lambda > 0: g[d] = float(double(g[d]) + ((lambda * (double(code[d]) - mu[d])) * ivar[d]) / double(D)), mu and ivar (D) float64;
 *     4. loss[b] and every g[d] of the clip finite: s = counter[0] + 1, bc1 = float(1 - pow(double(beta1), s)),
 *        bc2s = float(sqrt(1 - pow(double(beta2), s))), step_size = lr_dev[0] / bc1, and per element in fp32
 *          m = fma(m, beta1, (1 - beta1) * g);  v = fma(v, beta2, ((1 - beta2) * g) * g);
 *          code = fma(-step_size, m / (sqrt(v) / bc2s + eps), code)
 *        (sdt_adam_step_f32's update with weight_decay 0 and grad_scale 1, bit for bit on a buffer of a multiple of 4 elements);
 *        otherwise code, m and v keep their bits and nonfinite[b] = 1 (int32, never cleared here);
 *     5. h[b, t, C + d] = code[d] for every t: the chain's input buffer (B, T, C + D); its first C channels are not touched;
 *     6. history[counter[0], b] = loss[b] where counter[0] < history_rows, history (history_rows, B) float64;
 *     then counter[0] += 1 (a second launch on the same stream).  mode 1: 1 and 6 only, the counter stays (the loss of the last code).
 *   set: h[b, t, C + d] = codes[b, d], codes (B, D) fp32.
 *   pick: cand_loss (M, B) float64.  index[b] (int32) = the lowest j with the smallest finite cand_loss[j, b], -1 when the clip has none;
 *     best[b] = that loss (NaN for -1); with cands (M, D) fp32 and code_out (B, D) both given, code_out[b] = cands[max(index[b], 0)].
 */
int sdt_code_fit_loss_f32(const float* pred, const float* gt, int B, int64_t n, double* loss, float* dpred, void* stream);
int sdt_code_fit_step_f32(const float* dh, const double* loss, float* code, float* m, float* v, float* best_code, double* best_loss,
                          int64_t* counter, const float* lr_dev, const double* mu, const double* ivar, double lambda, float beta1, float beta2,
                          float eps, float* h, int B, int T, int C, int D, double* history, int64_t history_rows, int32_t* nonfinite, int mode,
                          void* stream);
int sdt_code_fit_set_f32(const float* codes, float* h, int B, int T, int C, int D, void* stream);
int sdt_code_fit_pick_f32(const double* cand_loss, int M, int B, const float* cands, int D, int32_t* index, double* best, float* code_out,
                          void* stream);

/*
 * Precision / recall and density / coverage between the pose-encoder features of the real and of the generated clips (TEST.PRDC;
 * speechdrivestemplates_amd/prdc.py; DESIGN.md section 33 is the contract, prdc.prdc_model / commit_model / gather_model are the same
 * operations in numpy; no counterpart in the reference).  Rows are float64 vectors of D columns, float32 features widened exactly.
 * d2(x, y) = the sum over c = 0 .. D-1 in that order from +0.0 of (x_c - y_c)^2, every subtract, multiply and add rounded on its own
 * (csrc/exact_f64.h): symmetric to the bit.  The radius of a row in its set = the k-th smallest d2 to the OTHER rows of the set (self left
 * out by position, so duplicates at d2 = 0 count), +inf in a set of at most k rows.  No square root, no floating-point atomics, no
 * allocation, no host synchronisation; every pointer except ``tables`` (a host array, read during the call) is a device buffer.  Sizes are
 * checked before any launch: rows (and clips x copies) 1 .. 2^20 per set, D 1 .. 64, k 1 .. 16, copies 1 .. 16, slices 1 .. 4096; anything
 * else returns SDT_ERR_UNSUPPORTED (a null pointer or a workspace that is too small SDT_ERR_ARG).
 *   A record is sdt_prdc_cols(D, m) = SDT_PRDC_HEADER_WORDS + D (1 + m) words of 8 bytes: int64 0 copies m (0 = no step has committed the
 *     clip: the seen word), 1 nonfinite (a NaN or an infinity among the clip's features); float64 [2, 2 + D) the ground truth of copy 0, mu then
 *     logvar (D = 2 Dh); [2 + D (1 + j), 2 + D (2 + j)) the prediction of copy j.  A table is (N + 1) records: row N is the header, whose word 0
 *     counts the clip indices outside [0, N) (they write nothing else).
 *   commit: mu_pred, logvar_pred, mu_gt, logvar_gt (m B, Dh) float32, copy j of clip b in row j B + b -> row clip_index[b] of table.
 *   gather: tables are ranks (1..64) table pointers; clip n takes the record of the lowest rank with copies != 0; records with nonfinite set
 *     are left out of both sets and counted.  Live clip number p (its position among the live clips in index order, an exclusive prefix over
 *     the live flags) gives row p of real (its ground truth) and rows p m + j of gen (its predictions), the leading dim_used columns of each,
 *     pitch dim_used; real_clip / gen_clip / gen_copy map a row back.  With floor_pass the ground truth of live clip p gives row p / 2 of real
 *     for an even p and row p / 2 of gen for an odd p (gen_copy 0).  real holds N rows, gen N m; work 2 N words.  counts (8 int64): 0 rows of
 *     real, 1 rows of gen, 2 clips with a record, 3 of them left out as nonfinite, 4 index errors of all tables, 5 live clips, 6, 7 zero.
 *   The all-pairs stages read their row counts from device words (count, qcount, scount: at most cap rows are ever touched), so no stage
 *   waits for the host.  One thread owns a query row, the other set streams through LDS in tiles of 32 rows, the streamed range is split
 *   into ``slices`` equal stretches (gridDim.y; sdt_prdc_slices proposes a number) whose partial results a second launch merges: the
 *   results do not depend on the number of slices.
 *   knn: radius[i] of every row of x (count rows of D) as defined above.  part: slices x cap x 16 words.
 *   cross: for every row i of q: ball_count[i] = the number of rows s of sx with d2(q_i, sx_s) <= s_radius[s]; nearest_d2[i] = the smallest
 *     d2(q_i, sx_s) (+inf for an empty sx) and nearest[i] = the lowest s that has it (-1).  part: slices x qcap x 3 words.
 *   reduce: counts as gather leaves them (words 0 .. 4 are read); r_real the radii of real; gen_balls of cross(gen, real, r_real); real_balls
 *     and real_nearest_d2 of cross(real, gen, r_gen).  covered[i] = real_nearest_d2[i] <= r_real[i], recalled[i] = real_balls[i] > 0.  out
 *     (SDT_PRDC_OUT_WORDS = 16): float64 0 precision = #{j : gen_balls[j] > 0} / Ng, 1 recall = #recalled / Nr, 2 density = sum_j gen_balls[j]
 *     / (k Ng), 3 coverage = #covered / Nr, each one division of two exactly converted integers, each the NaN 0x7ff8000000000000 when err != 0;
 *     int64 4 .. 7 the four numerators, 8 Nr, 9 Ng, 10 k, 11 err (SDT_PRDC_ERR_REAL_ROWS: Nr <= k, SDT_PRDC_ERR_GEN_ROWS: Ng <= k),
 *     12 clips with a record, 13 left out as nonfinite, 14 index errors, 15 zero.
 */
#define SDT_PRDC_HEADER_WORDS 2
#define SDT_PRDC_OUT_WORDS 16
#define SDT_PRDC_ERR_REAL_ROWS 1
#define SDT_PRDC_ERR_GEN_ROWS 2
int64_t sdt_prdc_cols(int D, int m);
int sdt_prdc_commit(const float* mu_pred, const float* logvar_pred, const float* mu_gt, const float* logvar_gt, const int64_t* clip_index, int B,
                    int m, int Dh, void* table, int64_t N, void* stream);
int sdt_prdc_gather(const void* const* tables, int ranks, int64_t N, int D, int m, int dim_used, int floor_pass, void* work, double* real,
                    double* gen, int64_t* real_clip, int64_t* gen_clip, int64_t* gen_copy, int64_t* counts, void* stream);
int64_t sdt_prdc_slices(int64_t queries, int64_t streamed);
int sdt_prdc_knn(const double* x, const int64_t* count, int64_t cap, int D, int k, int slices, void* part, int64_t part_words, double* radius,
                 void* stream);
int sdt_prdc_cross(const double* q, const int64_t* qcount, int64_t qcap, const double* sx, const int64_t* scount, int64_t scap,
                   const double* s_radius, int D, int slices, void* part, int64_t part_words, int64_t* ball_count, int64_t* nearest,
                   double* nearest_d2, void* stream);
int sdt_prdc_reduce(const int64_t* counts, int64_t real_cap, int64_t gen_cap, int k, const double* r_real, const int64_t* gen_balls,
                    const int64_t* real_balls, const double* real_nearest_d2, int64_t* covered, int64_t* recalled, int64_t* out, void* stream);

/*
 * Bootstrap over the clips of a record table (TEST.BOOTSTRAP; speechdrivestemplates_amd/bootstrap.py; DESIGN.md section 34 is the contract,
 * bootstrap.stages_model is the same operations in numpy).  Float words are float64 carried in 8-byte words, every operation rounded on its
 * own (csrc/exact_f64.h); integer words are added exactly; no floating-point atomics.  No allocation; every pointer except ``tables_a``,
 * ``tables_b`` and ``part_sizes`` (host arrays, read during the call) is a device buffer; every size is checked before the launch.
 *   sdt_clip_metrics_replicate_dense: the live clips of the clip-metrics tables (sdt_clip_metrics_epoch's ``tables``: per clip the record of
 *     the lowest rank with seen set; live = there is one and its nonfinite word is 0 -- with ranks_b > 0 in BOTH sets), in clip order, as
 *     dense rows of 39 words: the record's words [0, 36) (20 float sums, 16 hit counts), then copies * frames, copies * (frames - 1),
 *     copies * (copies - 1) / 2 * frames.  dense_a (dense_b): N x 39 words, the first n filled; n_out[0] = n.  point_a (point_b): 39 words,
 *     the sums of the set's live rows in the order of the epoch stage: chunks of 64 clips OF THE TABLE in index order, then the chunk
 *     partials in order (with one set these are the totals sdt_clip_metrics_epoch divides).  work: ceil(N / 64) * 80 words.  With
 *     ranks_b == 0 the three pointers of the second set are NULL.
 *   sdt_bootstrap_sums: generic.  dense: n rows of ``words`` (1 .. 64) words, the first ``float_words`` float64, the rest int64.  Draw i
 *     (0 .. n - 1) of replicate r (0 .. replicates - 1) is row (uint64(w) * n) >> 32, w = word i & 3 of Philox4x32-10 with the counter
 *     (i >> 2, 3, r, 0) and the key (seed low word, seed high word).  sums[r] (``words`` words) adds the n drawn rows in chunks of 64 draws
 *     in draw order, then the chunk partials in order.  work: replicates * ceil(n / 64) * words words.  n < 2^31, replicates <= 65535.
 *   sdt_clip_metrics_replicate_values: the final divisions of sdt_clip_metrics_epoch on each of ``rows`` sum rows of 39 words: values
 *     (rows x 36 float64, the words [0, 36) of the epoch vector) and pair_frames (rows int64, the (pair, frame) terms behind diversity).
 *   sdt_bootstrap_diff_f64: d[i] = a[i] - b[i].
 *   sdt_bootstrap_intervals_f64: values is (replicates, cols) float64; lohi (cols x 2) takes per column the order statistics at ranks
 *     ``rank`` and replicates - 1 - rank (0 <= 2 rank < replicates) in the order of csrc/radix_select.h's order_key, by eight digit passes:
 *     each is one of the inputs.  counts: NULL, or cols x 3 int64 = per column the number of values < 0, > 0, == 0.
 */
#define SDT_BOOTSTRAP_CLIP_WORDS 39
#define SDT_BOOTSTRAP_CLIP_VALUES 36
#define SDT_BOOTSTRAP_DENSE_WORK 80
int sdt_clip_metrics_replicate_dense(const void* const* tables_a, int ranks_a, const void* const* tables_b, int ranks_b, int64_t N, void* work,
                                     void* dense_a, void* dense_b, void* point_a, void* point_b, int64_t* n_out, void* stream);
int sdt_bootstrap_sums(const void* dense, int64_t n, int words, int float_words, int replicates, uint64_t seed, void* work, void* sums,
                       void* stream);
int sdt_clip_metrics_replicate_values(const void* sums, int64_t rows, const int64_t* part_sizes, int num_alphas, void* values,
                                      void* pair_frames, void* stream);
int sdt_bootstrap_diff_f64(const double* a, const double* b, int64_t n, double* d, void* stream);
int sdt_bootstrap_intervals_f64(const double* values, int64_t replicates, int cols, int64_t rank, double* lohi, int64_t* counts, void* stream);

/*
 * The audio band under the rendered pictures (SYS.AUDIO_STRIP; speechdrivestemplates_amd/audio_strip.py; DESIGN.md section 35 is the contract,
 * audio_strip.envelope_model / raster_model / compose_model are the same operations in numpy).  Every decision is integer arithmetic, a
 * comparison or one IEEE operation rounded on its own; minima and maxima are taken on an integer order key (-0 below +0); a non-finite sample is
 * selected away, never compared; the only atomics are integer ones.  No allocation; every pointer except ``colours``, ``background`` and
 * ``playhead`` (host arrays of BGR bytes, read during the call) is a device buffer; every size is checked before the launch.
 *   sdt_strip_envelope_f32: audio (L,) float32; bounds (Nc + 1,) int64 ascending, the columns' start samples.  Column c covers the samples
 *     [max(bounds[c], 0), min(bounds[c + 1], L)): env[2 c], env[2 c + 1] = the min and max of its finite samples (0 without one), flags[c] =
 *     SDT_STRIP_EMPTY (no sample), SDT_STRIP_NONFINITE (a NaN or an infinity among them) or SDT_STRIP_OK.  stats[0] = the bits of max |x| over
 *     the finite samples of the whole recording (a float32 in the low word, 0 without one), stats[1] = the number of non-finite samples.
 *   sdt_strip_raster_u8: the band (S, Nc, 3) uint8 BGR from the envelope, the power mel (n_mels, F) float32, colormap (256, 3) uint8 BGR,
 *     factors (255,) float32 ascending and three lists of int32 ticks of 1/300 s (n = 0: an absent list).  From the top: a waveform lane of
 *     Sw = 3 S / 8 rows, SDT_STRIP_MARK_LANES mark lanes of SDT_STRIP_MARK_ROWS rows, a mel lane of Sm rows (the rest).
 *     Waveform: sample x sits in row clamp(floor((1 - x g) (Sw - 1) / 2 + 0.5), 0, Sw - 1), g = 1 / max(peak, 2^-15), float64, each operation
 *     rounded on its own; an OK column has colours[1] from the row of its max to the row of its min, colours[0] elsewhere; a NONFINITE column
 *     is colours[2] over the lane; an EMPTY one colours[0].  Marks: tick k >= 0 is at sample k * 16000 / 300 and colours, in lane q,
 *     colours[3 + q] in the column that holds that sample and the SDT_STRIP_TICK_WIDTH - 1 columns after it; ticks outside
 *     [bounds[0], bounds[Nc]) are ignored.  Mel: pixel (y, c) takes frame min(max((bounds[c] + bounds[c + 1]) >> 1, 0) / 160, F - 1) and bin
 *     n_mels (Sm - 1 - y) / Sm; its colour is colormap[the number of i with p >= fl32(ref * factors[i])], ref = the largest finite power of
 *     the mel, at least +0 (work[0], never read back); a non-finite power is colours[2]; an EMPTY column is colours[0].  work: 8 bytes.
 *   sdt_strip_compose_u8: out (n, H + S, W, 3): rows [0, H) of image i are those of frames (n, H, W, 3); row H + y is row y of the band,
 *     columns [c0[i], c0[i] + W), ``background`` where that leaves [0, Nc); ``playhead`` over columns [ph[i] - c0[i], + SDT_STRIP_PLAYHEAD_WIDTH)
 *     unless ph[i] < 0.  16 bytes per lane when W * 3 and both base addresses are multiples of 16 (sdt_strip_compose_vectorised returns 1),
 *     else a byte per lane.
 */
#define SDT_STRIP_EMPTY 0
#define SDT_STRIP_NONFINITE 1
#define SDT_STRIP_OK 2
#define SDT_STRIP_MARK_LANES 3
#define SDT_STRIP_MARK_ROWS 8
#define SDT_STRIP_TICK_WIDTH 2
#define SDT_STRIP_PLAYHEAD_WIDTH 2
#define SDT_STRIP_COLOURS 6
#define SDT_STRIP_MIN_HEIGHT 64
#define SDT_STRIP_MAX_HEIGHT 1024
#define SDT_STRIP_MAX_COLUMNS (1 << 24)
int sdt_strip_envelope_f32(const float* audio, int64_t L, const int64_t* bounds, int Nc, float* env, int32_t* flags, int64_t* stats,
                           void* stream);
int sdt_strip_raster_u8(const float* env, const int32_t* flags, const int64_t* stats, const int64_t* bounds, int Nc, const float* mel, int n_mels,
                        int64_t F, const uint8_t* colormap, const float* factors, const int32_t* ticks0, int n0, const int32_t* ticks1, int n1,
                        const int32_t* ticks2, int n2, const uint8_t* colours, int S, void* work, uint8_t* band, void* stream);
int sdt_strip_compose_u8(const uint8_t* frames, int64_t n, int H, int W, const uint8_t* band, int S, int Nc, const int32_t* c0, const int32_t* ph,
                         const uint8_t* background, const uint8_t* playhead, uint8_t* out, int64_t out_bytes, void* stream);
int sdt_strip_compose_vectorised(const void* frames, int W, const void* out);

#ifdef __cplusplus
}
#endif
#endif /* SDT_HIP_H */
