"""The fp32 Conv2d kernels -- the default arithmetic, what the headline is measured on -- swept over edge geometries against float64 through the
public entry points ops.conv_forward, ops.ConvStatsFn, ops.conv_input_grad (no holder, IN holder, BN holder) and ops.conv_weight_grad on fp32
tensors, with the kernel that serves every launch PINNED per case (EXPECT / EXPECT_MFMA; `python tests/test_f32_conv_sweep_gpu.py --plans` prints
the tables from the host planner, no GPU needed).  Modelled on test_bf16_conv_sweep_gpu.py, whose hand-picked geometries it keeps.

Kernel families an fp32 launch can reach (speechdrivestemplates_amd/ops.py, csrc/convsk.hip, csrc/convbf.hip, csrc/conv.hip):
  forward / dx   convbf2_kernel<float, 128, 128 | 256, 64>   split-fp32: three bf16 planes per operand, six MFMAs (ops.F32_SPLIT, default)
                 convsk_kernel<128, 128 | 128, 64>           fp32 MFMA (ops.F32_SPLIT = False, SYS.CONV_F32_SPLIT: False; and wherever the split
                                                             plan is refused for its tile count but the two-per-CU plan is wanted and fits)
                 sdt_conv_taps_f32 / sdt_conv_taps_splitk_f32 + reduce / sdt_conv_taps_multi_f32 / sdt_conv_taps_stats_f32   the 64 x 64 fall-back
  dW             convx3_dw_kernel<bm, bn> (split), convsk_dw_kernel<bm, bn> (fp32 MFMA), sdt_conv_dw_det_f32 (fall-back)

Operands: seeded randn ROUNDED TO fp32, the full 24-bit mantissa (the mid and low planes of the split carry data); the reference is F.conv2d and
its autograd in float64 on those same values.  Holder inputs (y, mean, rstd, gamma, beta) are fp32-representable and every float64
pre-activation is clear of the LeakyReLU kink by KINK = 1e-4 (asserted; no element is excluded from any comparison).

Flush cadence of the split kernel (csrc/convbf.hip, the K loop of convbf2_kernel<float>): the fp32 accumulators are added to `tot` and cleared
every CH = SK_CHUNK = 8 K steps (csrc/convsk.h; UNR = 2 divides it), a K step being 128 bytes = 32 fp32 channels of one tap, counted from the
first step a workgroup RUNS of a tile (nsteps = F.b - F.a: a tile cut between two workgroups' ranges runs two shorter loops).  The cadence-* cases
have taps * Cin / 32 = 7, 9 and 17 steps per tile (7 x 1, 3 x 3 and 17 x 1 taps on 32 channels) on exactly G = 256 tiles, so every range is one
whole tile and every workgroup runs ONE loop of 7, 9 or 17 steps: shorter than one chunk, one step past one chunk, one step past two (asserted
from the plan's own tables by test_table_covers_the_planner; other cases meet the boundaries only by the way their ranges happen to fall).

Bars: those of the random sweeps in test_ops_gpu.py -- rel-max 4e-6 forward and dx, 8e-6 dW, 4e-6 forward and backward sums (the sums and the
sums of squares each against their own maximum).  Where 4x the error of fp32 torch on the CPU against float64 on the very inputs of a check is
larger, that is the tolerance (FP32_REF_ERR; `python tests/test_f32_conv_sweep_gpu.py` prints the entries; nothing a kernel produced enters a
tolerance).  test_cpu_fp32_stays_below_a_quarter_of_the_bars asserts the rest; test_bars_discriminate (host only) shows what these bars reject.

Power-of-two scaling (test_power_of_two_scaling): x 2^a, w 2^b, gy 2^c give y, dx, dW BIT-IDENTICAL to the unscaled run times 2^(a+b), 2^(b+c),
2^(a+c) -- derived, not measured: the three-plane split, the bf16 x bf16 products, fp32 accumulation, the fp32 MFMA and the fall-back's FMAs are
all exact under a power-of-two scale while nothing is subnormal (operands have |value| in [2^-10, 2^4]).  A kernel that thresholds, flushes or
drops a low plane by magnitude fails it.

What the table cannot reach under the size cap (5e9 multiply-adds, 8192 output pixels per case):
  * a FORWARD launch on convbf2_kernel<float, 256, 64> with Cout = 64 or 192: the split plan wants 2 T >= 256 tiles of 256 rows, i.e. more than
    10 000 output pixels (Cout = 320 reaches the form with five column tiles; the input gradients of the ho-wo-1-* cases reach it with Cin = 64);
  * an INPUT GRADIENT on convsk_kernel<128, 64>: at any size -- ops._sk_wanted gives the two-per-CU fp32 kernel only the input gradients with
    Cin % 128 == 0 (STREAMK_MIN_COUT), which take 128 x 128 tiles; the form serves forward launches only (asserted in the table test);
  * BN grouping at 31 / 32 / 33 rows IN ALL on a stream-K input gradient: B Hi Wi = 33 rows are one tile, and no plan has S >= 4 G K steps on one
    tile (the planner refuses Cin = 128 and 256 alike); under BN the threshold is only met from far above (every stream-K case) and on the
    fall-back (stat64-bn-63 / 64 / 65).  IN grouping is what the stat-in-* / stat-dx-* cases put at 31 / 32 / 33;
  * the 32-row threshold of the FORWARD statistics on the stream-K kernels: ops.conv_stats_fusable asks sdt_conv_taps_stats_supported, which
    wants 64 rows per group whichever kernel would serve the launch, so ConvStatsFn is never called between 32 and 63 rows per group; the
    stat-31/32/33 cases pin that answer ("no") and approach the threshold from both sides where it is live: the dx parity classes."""
import collections
import os
import random
import sys
import zlib

import pytest
import torch
import torch.nn.functional as F

from test_bf16_conv_sweep_gpu import HAND, KERNELS_RANDOM, MAX_MACS, MAX_PIXELS, SLOPE, bwd_sums, dims, fwd_sums, holder_modes, out_size, unreachable  # noqa: F401
from test_edge_shapes_gpu import DEV, EPS, KINK, _off_kink, check, f32, ops, rel_err  # noqa: F401  (ops: the fixture)

TOL_Y, TOL_DX, TOL_DW, TOL_SUMS, TOL_BSUMS = 4e-6, 4e-6, 8e-6, 4e-6, 4e-6
CADENCE = 8  # K steps (of 32 fp32 channels) between two flushes of the split kernel's accumulators

# (tag, B, Hi, Wi, Cin, Cout, kh, kw, s, p)
EXTRA = [
    # ---- Cin = 32 (mod 64): a K step is 32 channels; 1 x 1: one K step per tap and 32 channels
    ("cin32-k1", 8, 32, 32, 32, 2048, 1, 1, 1, 0),          # ONE K step per tile; 16 column tiles
    ("cin96-k1", 8, 32, 32, 96, 768, 1, 1, 1, 0),           # three K steps per tile
    ("cin160-k1", 8, 32, 32, 160, 512, 1, 1, 1, 0),         # five
    ("cin32-k3", 7, 30, 39, 32, 256, 3, 3, 1, 1),           # M = 8190
    ("cin96-k3", 5, 31, 37, 96, 384, 3, 3, 1, 1),
    ("cin160-k3", 3, 25, 43, 160, 64, 3, 3, 1, 1),
    ("cin32-k4s2", 8, 64, 64, 32, 256, 4, 4, 2, 1),
    ("cin96-k4s2", 6, 63, 71, 96, 384, 4, 4, 2, 1),
    ("cin160-k4s2", 5, 40, 66, 160, 320, 4, 4, 2, 1),
    # ---- every fp32 tile form under both settings of ops.F32_SPLIT (Cout = 64 / 192: 128 x 64 on the fp32-MFMA kernel, refused by the split
    # kernel's forward plan under the cap -- see the docstring; 320: 256 x 64 / 128 x 64; 384: 128 x 128, three column tiles)
    ("cout64", 8, 32, 32, 128, 64, 3, 3, 1, 1),
    ("cout192", 7, 33, 35, 128, 192, 3, 3, 1, 1),
    ("cout320", 6, 33, 40, 128, 320, 3, 3, 1, 1),
    ("cout384", 6, 31, 40, 128, 384, 3, 3, 1, 1),
    ("dw-64x64-b", 4, 36, 34, 64, 192, 3, 3, 1, 1),         # a third 64 x 64 weight-gradient tile: Cout and taps * Cin both odd multiples of 64
    # ---- K loops around the split kernel's flush cadence (CADENCE = 8 steps): 7, 9 and 17 steps per tile
    # (Cout = 512 on M = 8192: 64 x 4 = 256 tiles of 128 x 128 = G, every workgroup's range is ONE whole tile -- the flush is counted from the first
    # step a workgroup runs of a tile, so a tile cut between ranges would run shorter loops; segment_lengths() reads the lengths off the plan)
    ("cadence-7", 8, 38, 32, 32, 512, 7, 1, 1, 0),
    ("cadence-9", 8, 34, 34, 32, 512, 3, 3, 1, 0),
    ("cadence-17", 8, 48, 32, 32, 512, 17, 1, 1, 0),
    # ---- rows per statistics group at 31 / 32 / 33 on a stream-K plan (IN: rows per clip; BN: all rows; dx classes of a stride-1 layer = Hi Wi)
    ("stat-in-31", 200, 31, 1, 128, 384, 3, 3, 1, 1),
    ("stat-in-32", 200, 4, 8, 128, 384, 3, 3, 1, 1),
    ("stat-in-33", 200, 3, 11, 128, 384, 3, 3, 1, 1),
    ("stat-dx-31", 160, 2, 62, 128, 384, 2, 2, 2, 0),       # stride 2: four / two parity classes of 31, 32, 33 rows per clip
    ("stat-dx-32", 160, 8, 16, 128, 384, 2, 2, 2, 0),
    ("stat-dx-33", 160, 6, 22, 128, 384, 2, 2, 2, 0),
    # ---- ... and at 63 / 64 / 65 where the planner refuses (Cout = 96): sdt_conv_taps_stats_f32 and sdt_conv_taps_multi_f32 decide
    ("stat64-in-63", 100, 7, 9, 96, 96, 3, 3, 1, 1),
    ("stat64-in-64", 100, 8, 8, 96, 96, 3, 3, 1, 1),
    ("stat64-in-65", 100, 5, 13, 96, 96, 3, 3, 1, 1),
    ("stat64-bn-63", 3, 3, 7, 64, 96, 1, 1, 1, 0),          # BN: 63 / 64 / 65 rows in all (1 x 1: too few K steps to split, the hint is 1)
    ("stat64-bn-64", 2, 4, 8, 64, 96, 1, 1, 1, 0),
    ("stat64-bn-65", 5, 1, 13, 64, 96, 1, 1, 1, 0),
    # ---- channel counts on either side of each divisibility rule: the scalar loader (Cin % 32 != 0: no fused statistics, no stream-K), Cout % 64
    # (no stream-K forward / dW), Cin % 64 (no stream-K dW), Cout % 32 (dx: the scalar loader), Cout % 4 / Cin % 4 (dW fall-back without float4)
    ("cin3", 4, 20, 33, 3, 64, 3, 3, 1, 1),
    ("cin24", 4, 20, 33, 24, 64, 3, 3, 1, 1),
    ("cin48", 4, 20, 33, 48, 128, 4, 4, 2, 1),
    ("cout96", 4, 24, 40, 128, 96, 3, 3, 1, 1),
    ("cout48", 4, 24, 40, 64, 48, 3, 3, 1, 1),
    ("cout6", 4, 20, 33, 64, 6, 3, 3, 1, 1),
    # ---- dx_pack is None: a parity class without taps (1 x 1, stride 2: three of four classes are zero-filled on the host), more than 4 classes
    ("no-pack-k1s2", 6, 21, 37, 128, 128, 1, 1, 2, 0),
    ("no-pack-k2s3", 4, 20, 32, 64, 128, 2, 2, 3, 0),
    # ---- sdt_conv_taps_splitk_hint > 1 on a 2-D launch: fewer than 192 tiles of 64 x 64 and >= 8 K steps, refused by the planner (Cout = 96)
    ("splitk-2d", 2, 9, 17, 128, 96, 3, 3, 1, 1),
]

def _random_cases(n, seed):
    """the bf16 sweep's seeded fill with Cin widened to {32, 64, 96, 128, 160, 192, 256}"""
    rng, out = random.Random(seed), []
    while len(out) < n:
        Cin, Cout = rng.choice([32, 64, 96, 128, 160, 192, 256]), rng.choice([64, 128, 192, 256, 320, 384])
        kh, kw = rng.choice(KERNELS_RANDOM)
        s = rng.choice([1, 2])
        p = rng.randrange(0, min(kh, kw))
        B = rng.randrange(1, 9)
        pix = int(200 * (MAX_PIXELS / 200.0) ** rng.random()) // B
        Ho = max(1, min(pix, int(round(pix ** 0.5 * 2.0 ** rng.uniform(-1.5, 1.5)))))
        Wo = max(1, pix // Ho)
        Hi, Wi = (Ho - 1) * s + kh - 2 * p + rng.randrange(0, s), (Wo - 1) * s + kw - 2 * p + rng.randrange(0, s)
        if Hi < 1 or Wi < 1 or B * Ho * Wo > MAX_PIXELS or B * Ho * Wo * Cout * kh * kw * Cin > MAX_MACS:
            continue
        if out_size(Hi, kh, s, p) != Ho or out_size(Wi, kw, s, p) != Wo:
            continue
        out.append(("random-%d" % len(out), B, Hi, Wi, Cin, Cout, kh, kw, s, p))
    return out


CASES = HAND + EXTRA + _random_cases(8, 20261019)
CASE = {c[0]: c for c in CASES}
# run under ops.F32_SPLIT = False (the fp32-MFMA kernels) as well; chosen so that the two settings route differently
BOTH = ("k2s2", "k4s2p1-even", "cap-c256", "cap-c320", "cap-c384", "cap-cin192", "cap-cin128", "dw-128x128", "dw-64x64", "dw-64x128", "k3s2p1",
        "k3x5s2", "cout192", "cout320", "cout384", "dw-64x64-b", "cin96-k3")
# weight gradient called twice, then onto a pre-filled .grad: (tag, F32_SPLIT) -- one case per dW kernel and tile form
ACCUMULATE = (("dw-128x128", True), ("k3s2p1", True), ("dw-64x128", True), ("dw-64x64", True), ("dw-128x128", False), ("dw-64x64", False),
              ("cout96", True), ("cin3", True))
# power-of-two scaling: (tag, F32_SPLIT) -- one case per forward / dx / dW kernel family
SCALED = (("k4s2p1-even", True), ("cap-c320", True), ("k3x5s2", True), ("dw-128x128", False), ("cout96", True), ("no-pack-k1s2", True), ("cin3", True))
SCALES = ((12, -7, 3), (40, -40, 0), (-30, 20, 10))

Served = collections.namedtuple("Served", "fwd dx dw stats")
# Which kernel serves each case: forward, input gradient (x number of parity classes in the launch; k: split-K factor of the fall-back), weight
# gradient, and where the statistics fuse ("fwd IN BN | dx IN BN": ConvStatsFn under that grouping / the holder of that grouping is filled).
# Printed by `python tests/test_f32_conv_sweep_gpu.py --plans`; test_table_covers_the_planner asserts the planner still answers this, the GPU
# test that the launches got it.
EXPECT = {
    "one-row":         Served('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 1
    "sub-wave":        Served('sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x1 k=16', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 40
    "one-128-tile":    Served('sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x1 k=16', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 128
    "k3s2p1-small":    Served('sdt_conv_taps_splitk_f32 k=4', 'sdt_conv_taps_multi_f32 x4 k=2', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 60
    "tile-plus-one":   Served('sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x1 k=15', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 129
    "one-256-tile":    Served('sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x1 k=16', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 256
    "257-rows":        Served('sdt_conv_taps_splitk_f32 k=16', 'convsk_kernel<128, 128> x1', 'sdt_conv_dw_det_f32', 'fwd - | dx IN'),  # M = 257
    "clips-per-tile":  Served('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=11', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 756
    "k1s1":            Served('convbf2_kernel<float, 256, 64>', 'convbf2_kernel<float, 128, 128> x1', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx IN BN'),  # M = 8177
    "k1s2":            Served('convbf2_kernel<float, 256, 64>', 'sdt_conv_taps_splitk_f32 per class (1 of 4) k=1', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx -'),  # M = 8177
    "k2s2":            Served('convbf2_kernel<float, 128, 128>', 'convbf2_kernel<float, 128, 128> x4', 'convx3_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),  # M = 8192
    "k3s2p1":          Served('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=5', 'convx3_dw_kernel<128, 64>', 'fwd - | dx -'),  # M = 2560
    "k4s2p1-odd":      Served('sdt_conv_taps_splitk_f32 k=11', 'sdt_conv_taps_multi_f32 x4 k=4', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 1600
    "k4s2p1-even":     Served('convbf2_kernel<float, 128, 128>', 'convbf2_kernel<float, 256, 64> x4', 'convx3_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),  # M = 8192
    "k6x3":            Served('sdt_conv_taps_splitk_f32 k=16', 'convsk_kernel<128, 128> x1', 'sdt_conv_dw_det_f32', 'fwd - | dx IN BN'),  # M = 512
    "wo-1":            Served('sdt_conv_taps_splitk_f32 k=16', 'convsk_kernel<128, 128> x1', 'sdt_conv_dw_det_f32', 'fwd - | dx BN'),  # M = 700
    "ho-wo-1-c256":    Served('convsk_kernel<128, 64>', 'convbf2_kernel<float, 128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd - | dx BN'),  # M = 3640
    "ho-wo-1-c128":    Served('convsk_kernel<128, 64>', 'convbf2_kernel<float, 128, 128> x1', 'sdt_conv_dw_det_f32', 'fwd - | dx BN'),  # M = 3640
    "pad-k-1":         Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd - | dx IN BN'),  # M = 2816
    "k3x5s2":          Served('convsk_kernel<128, 128>', 'convbf2_kernel<float, 256, 64> x4', 'convx3_dw_kernel<128, 64>', 'fwd - | dx IN BN'),  # M = 2907
    "two-classes":     Served('sdt_conv_taps_splitk_f32 k=4', 'sdt_conv_taps_multi_f32 x2 k=3', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 2800
    "cap-c256":        Served('convbf2_kernel<float, 128, 128>', 'sdt_conv_taps_multi_f32 x1 k=4', 'convx3_dw_kernel<128, 64>', 'fwd IN BN | dx -'),  # M = 8177
    "cap-c320":        Served('convbf2_kernel<float, 256, 64>', 'sdt_conv_taps_multi_f32 x1 k=5', 'convx3_dw_kernel<64, 64>', 'fwd IN BN | dx -'),  # M = 6475
    "cap-c384":        Served('convbf2_kernel<float, 128, 128>', 'sdt_conv_taps_multi_f32 x4 k=7', 'convx3_dw_kernel<128, 128>', 'fwd IN BN | dx -'),  # M = 5418
    "cap-cin192":      Served('convsk_kernel<128, 64>', 'convbf2_kernel<float, 256, 64> x4', 'convx3_dw_kernel<64, 128>', 'fwd - | dx IN BN'),  # M = 8192
    "cap-cin128":      Served('convsk_kernel<128, 128>', 'convbf2_kernel<float, 128, 128> x4', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx IN BN'),  # M = 8192
    "dw-128x128":      Served('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<128, 128>', 'fwd - | dx IN BN'),  # M = 1566
    "dw-64x64":        Served('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=11', 'convx3_dw_kernel<64, 64>', 'fwd - | dx -'),  # M = 969
    "dw-64x128":       Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd - | dx IN BN'),  # M = 1150
    "cin32-k1":        Served('convbf2_kernel<float, 128, 128>', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx -'),  # M = 8192
    "cin96-k1":        Served('convbf2_kernel<float, 128, 128>', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx IN BN'),  # M = 8192
    "cin160-k1":       Served('convbf2_kernel<float, 128, 128>', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx IN BN'),  # M = 8192
    "cin32-k3":        Served('convbf2_kernel<float, 128, 128>', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx -'),  # M = 8190
    "cin96-k3":        Served('convbf2_kernel<float, 128, 128>', 'sdt_conv_taps_multi_f32 x1 k=3', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx -'),  # M = 5735
    "cin160-k3":       Served('sdt_conv_taps_splitk_f32 k=11', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 3225
    "cin32-k4s2":      Served('convbf2_kernel<float, 128, 128>', 'sdt_conv_taps_multi_f32 x4 k=4', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx -'),  # M = 8192
    "cin96-k4s2":      Served('convbf2_kernel<float, 128, 128>', 'sdt_conv_taps_multi_f32 x4 k=1', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx IN BN'),  # M = 6510
    "cin160-k4s2":     Served('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x4 k=4', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx -'),  # M = 3300
    "cout64":          Served('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd - | dx IN BN'),  # M = 8192
    "cout192":         Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd IN BN | dx IN BN'),  # M = 8085
    "cout320":         Served('convbf2_kernel<float, 256, 64>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd IN BN | dx IN BN'),  # M = 7920
    "cout384":         Served('convbf2_kernel<float, 128, 128>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),  # M = 7440
    "dw-64x64-b":      Served('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=7', 'convx3_dw_kernel<64, 64>', 'fwd IN BN | dx -'),  # M = 4896
    "cadence-7":       Served('convbf2_kernel<float, 128, 128>', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx -'),  # M = 8192
    "cadence-9":       Served('convbf2_kernel<float, 128, 128>', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx -'),  # M = 8192
    "cadence-17":      Served('convbf2_kernel<float, 128, 128>', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx IN BN'),  # M = 8192
    "stat-in-31":      Served('convbf2_kernel<float, 128, 128>', 'sdt_conv_taps_multi_f32 x1 k=1', 'convx3_dw_kernel<128, 128>', 'fwd BN | dx BN'),  # M = 6200
    "stat-in-32":      Served('convbf2_kernel<float, 128, 128>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<128, 128>', 'fwd BN | dx IN BN'),  # M = 6400
    "stat-in-33":      Served('convbf2_kernel<float, 128, 128>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<128, 128>', 'fwd BN | dx IN BN'),  # M = 6600
    "stat-dx-31":      Served('sdt_conv_taps_f32', 'convbf2_kernel<float, 128, 128> x4', 'sdt_conv_dw_det_f32', 'fwd BN:sdt_conv_taps_stats_f32 | dx BN'),  # M = 4960
    "stat-dx-32":      Served('sdt_conv_taps_f32', 'convbf2_kernel<float, 128, 128> x4', 'sdt_conv_dw_det_f32', 'fwd BN:sdt_conv_taps_stats_f32 | dx IN BN'),  # M = 5120
    "stat-dx-33":      Served('sdt_conv_taps_f32', 'convbf2_kernel<float, 128, 128> x4', 'sdt_conv_dw_det_f32', 'fwd BN:sdt_conv_taps_stats_f32 | dx IN BN'),  # M = 5280
    "stat64-in-63":    Served('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd BN:sdt_conv_taps_stats_f32 | dx BN'),  # M = 6300
    "stat64-in-64":    Served('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx IN BN'),  # M = 6400
    "stat64-in-65":    Served('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx IN BN'),  # M = 6500
    "stat64-bn-63":    Served('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 63
    "stat64-bn-64":    Served('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd BN:sdt_conv_taps_stats_f32 | dx BN'),  # M = 64
    "stat64-bn-65":    Served('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd BN:sdt_conv_taps_stats_f32 | dx BN'),  # M = 65
    "cin3":            Served('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 2640
    "cin24":           Served('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 2640
    "cin48":           Served('sdt_conv_taps_splitk_f32 k=6', 'sdt_conv_taps_multi_f32 x4 k=4', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 640
    "cout96":          Served('sdt_conv_taps_splitk_f32 k=5', 'sdt_conv_taps_multi_f32 x1 k=5', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 3840
    "cout48":          Served('sdt_conv_taps_splitk_f32 k=4', 'sdt_conv_taps_multi_f32 x1 k=3', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 3840
    "cout6":           Served('sdt_conv_taps_splitk_f32 k=4', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 2640
    "no-pack-k1s2":    Served('sdt_conv_taps_f32', 'sdt_conv_taps_splitk_f32 per class (1 of 4) k=1', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'),  # M = 1254
    "no-pack-k2s3":    Served('sdt_conv_taps_splitk_f32 k=2', 'sdt_conv_taps_splitk_f32 per class (4 of 9) k=1', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 308
    "splitk-2d":       Served('sdt_conv_taps_splitk_f32 k=9', 'sdt_conv_taps_multi_f32 x1 k=6', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 306
    "random-0":        Served('sdt_conv_taps_splitk_f32 k=5', 'sdt_conv_taps_multi_f32 x1 k=6', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 520
    "random-1":        Served('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x4 k=7', 'convx3_dw_kernel<64, 128>', 'fwd - | dx -'),  # M = 1575
    "random-2":        Served('sdt_conv_taps_splitk_f32 k=2', 'sdt_conv_taps_multi_f32 x1 k=8', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 210
    "random-3":        Served('sdt_conv_taps_splitk_f32 k=8', 'sdt_conv_taps_multi_f32 x4 k=1', 'sdt_conv_dw_det_f32', 'fwd - | dx BN'),  # M = 168
    "random-4":        Served('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=6', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 1890
    "random-5":        Served('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 4935
    "random-6":        Served('sdt_conv_taps_splitk_f32 k=8', 'sdt_conv_taps_multi_f32 x4 k=12', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),  # M = 646
    "random-7":        Served('sdt_conv_taps_splitk_f32 k=10', 'sdt_conv_taps_multi_f32 x4 k=1', 'sdt_conv_dw_det_f32', 'fwd - | dx IN BN'),  # M = 1224
}
# the BOTH cases with ops.F32_SPLIT = False
EXPECT_MFMA = {
    "k2s2":            Served('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=1', 'convsk_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),  # M = 8192
    "k4s2p1-even":     Served('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=4', 'convsk_dw_kernel<128, 128>', 'fwd IN BN | dx -'),  # M = 8192
    "cap-c256":        Served('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x1 k=4', 'convsk_dw_kernel<128, 64>', 'fwd IN BN | dx -'),  # M = 8177
    "cap-c320":        Served('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=5', 'convsk_dw_kernel<64, 64>', 'fwd IN BN | dx -'),  # M = 6475
    "cap-c384":        Served('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=7', 'convsk_dw_kernel<128, 128>', 'fwd IN BN | dx -'),  # M = 5418
    "cap-cin192":      Served('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x4 k=1', 'convsk_dw_kernel<64, 128>', 'fwd - | dx IN BN'),  # M = 8192
    "cap-cin128":      Served('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=1', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx IN BN'),  # M = 8192
    "dw-128x128":      Served('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<128, 128>', 'fwd - | dx IN BN'),  # M = 1566
    "dw-64x64":        Served('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=11', 'convsk_dw_kernel<64, 64>', 'fwd - | dx -'),  # M = 969
    "dw-64x128":       Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<64, 128>', 'fwd - | dx IN BN'),  # M = 1150
    "k3s2p1":          Served('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=5', 'convsk_dw_kernel<128, 64>', 'fwd - | dx -'),  # M = 2560
    "k3x5s2":          Served('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=4', 'convsk_dw_kernel<128, 64>', 'fwd - | dx -'),  # M = 2907
    "cout192":         Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<64, 128>', 'fwd IN BN | dx IN BN'),  # M = 8085
    "cout320":         Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<64, 128>', 'fwd IN BN | dx IN BN'),  # M = 7920
    "cout384":         Served('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),  # M = 7440
    "dw-64x64-b":      Served('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=7', 'convsk_dw_kernel<64, 64>', 'fwd IN BN | dx -'),  # M = 4896
    "cin96-k3":        Served('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x1 k=3', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx -'),  # M = 5735
}


def modes(c):
    B = c[1]
    return [("IN", B)] + ([("BN", 1)] if B > 1 else [])


def _dx_route(ops, c, dev):
    """(name, kind, pack, k) of the input-gradient launch as ops.conv_input_grad routes it"""
    from speechdrivestemplates_amd import _lib
    lib = _lib.load()
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    pack = ops.dx_pack(B, Hi, Wi, Cin, Cout, kh, kw, s, p, False)
    if pack is None:
        live = [g for g, _ in ops.dx_geoms(B, Hi, Wi, Cin, Cout, kh, kw, s, p)]
        k = max(ops._splitk_hint(lib, g) for g in live) if all(g is not None for g in live) else 1
        return "sdt_conv_taps_splitk_f32 per class (%d of %d) k=%d" % (sum(g is not None for g in live), len(live), k), "classes", None, k
    plan = ops._sk_plan(pack[0], pack[1], -1, 1, dev)
    if plan is not None:
        return "%s x%d" % (ops._sk_name(plan), pack[1]), "sk", pack, 1
    k = max(ops._splitk_hint(lib, g) for g in pack[2])
    return "sdt_conv_taps_multi_f32 x%d k=%d" % (pack[1], k), "multi", pack, k


def dx_fuses(ops, c, groups, dev):
    """the routing's own predicate (ops.conv_input_grad): >= 32 rows per group and class on a stream-K plan, >= 64 on an unsplit vector-path
    launch of sdt_conv_taps_multi_f32 (the dY channels a multiple of 32), never on the per-class launches"""
    B, Hi, Wi, Cin, Cout = c[1:6]
    _name, kind, pack, k = _dx_route(ops, c, dev)
    if kind == "classes":
        return False
    rows = [(g.B * g.Ho * g.Wo if groups == 1 else g.Ho * g.Wo) for g in pack[2]]
    if kind == "sk":
        return all(r >= 32 for r in rows)
    return k == 1 and Cout % 32 == 0 and B * Hi * Wi * Cin * 4 < 2 ** 31 - 4 and all(r >= 64 for r in rows)


def fwd_fuses(ops, c, groups):
    """ops.conv_stats_fusable restated on the geometry (host code; the library answers): Cin % 32 == 0, >= 64 rows per group, no split-K"""
    from speechdrivestemplates_amd import _lib
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    m = B * Ho * Wo
    return bool(m % groups == 0 and _lib.load().sdt_conv_taps_stats_supported(ops.fwd_geom(B, Hi, Wi, Cin, Cout, kh, kw, s, p), m // groups))


def served(ops, c, dev):
    """What serves the forward, the dx and the dW launch of a case on ``dev`` and where the statistics fuse (host code; the plans are the cached ones)"""
    from speechdrivestemplates_amd import _lib
    lib = _lib.load()
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    g = ops.fwd_geom(B, Hi, Wi, Cin, Cout, kh, kw, s, p)
    plan = ops._sk_plan(g, 1, 0, 1, dev, forward=True) if ops.USE_STREAMK else None
    if plan is not None:
        fwd = ops._sk_name(plan)
    else:
        k = ops._splitk_hint(lib, g)
        fwd = "sdt_conv_taps_splitk_f32 k=%d" % k if k > 1 else "sdt_conv_taps_f32"
    fs = []
    for mode, groups in modes(c):
        if fwd_fuses(ops, c, groups):  # ConvStatsFn: the stream-K plan with this grouping, else the 64 x 64 statistics kernel
            sp = ops._sk_plan(g, 1, B * Ho * Wo // groups, 1, dev, forward=True)
            assert (sp is None) == (plan is None), "the forward kernel depends on the statistics grouping"
            fs.append(mode if sp is not None else mode + ":sdt_conv_taps_stats_f32")
    dx = _dx_route(ops, c, dev)[0]
    dplan = ops._sk_dw_plan(g, dev)
    if dplan is None:
        dw = "sdt_conv_dw_det_f32"
    else:
        dw = "%s<%d, %d>" % ("convx3_dw_kernel" if (dplan.host[3] >> 26) & 1 else "convsk_dw_kernel", dplan.host[1], dplan.host[2])
    bs = [mode for mode, groups in holder_modes(c) if dx_fuses(ops, c, groups, dev)]
    return Served(fwd, dx, dw, "fwd %s | dx %s" % (" ".join(fs) or "-", " ".join(bs) or "-"))


Data = collections.namedtuple("Data", "x w gy y dx dw")


def _randn32(shape, g, scale=1.0):
    return f32(torch.randn(*shape, generator=g, dtype=torch.float64) * scale)


def reference(c, dtype=torch.float64, data=None):
    """fp32-representable operands with the full 24-bit mantissa (seeded by the tag) and conv2d + autograd in ``dtype`` on them; channels-last
    x, gy, y, dx"""
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    if data is None:
        g = torch.Generator().manual_seed(zlib.crc32(c[0].encode()))
        x = _randn32((B, Hi, Wi, Cin), g)
        w = _randn32((Cout, Cin, kh, kw), g, (2.0 / (Cin * kh * kw)) ** 0.5)
        gy = _randn32((B, Ho, Wo, Cout), g)
    else:
        x, w, gy = data.x, data.w, data.gy
    xr = x.to(dtype).permute(0, 3, 1, 2).requires_grad_(True)
    wr = w.to(dtype).clone().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, s, p)
    yr.backward(gy.to(dtype).permute(0, 3, 1, 2))
    return Data(x, w, gy, yr.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), wr.grad)


def bias_of(c):
    return _randn32((c[5],), torch.Generator().manual_seed(zlib.crc32((c[0] + " bias").encode())))


def _moments(y3):
    """fp32-representable mean and rstd per (group, channel) of y3 (G, R, C): what the holder hands to the kernel"""
    mean = f32(y3.mean(1, keepdim=True))
    rstd = f32(1.0 / torch.sqrt(y3.var(1, unbiased=False, keepdim=True) + EPS))
    return mean, rstd


def below(c, mode, groups):
    """The block below: its stored fp32 output, its statistics and (BN) affine parameters, every float64 pre-activation clear of the kink"""
    B, Hi, Wi, Cin = c[1:5]
    g = torch.Generator().manual_seed(zlib.crc32((c[0] + mode).encode()))
    y3 = _randn32((groups, B * Hi * Wi // groups, Cin), g)
    gamma = beta = None
    if mode == "BN":
        gamma = f32(1.0 + 0.1 * torch.randn(Cin, generator=g, dtype=torch.float64))
        beta = f32(0.1 * torch.randn(Cin, generator=g, dtype=torch.float64))

    def pre(y):
        mean, rstd = _moments(y)
        u = (y - mean) * rstd
        return [u if gamma is None else u * gamma + beta]

    y3 = _off_kink(y3, pre)
    mean, rstd = _moments(y3)
    assert torch.equal(y3, f32(y3)) and float(pre(y3)[0].abs().min()) >= KINK
    return dict(y=y3, mean=mean, rstd=rstd, gamma=gamma, beta=beta)


# Measured on the CPU (`python tests/test_f32_conv_sweep_gpu.py`): rel-max-err of the same torch formula in fp32 against float64 on the very
# inputs of the named quantity (the fp32 side on ONE thread, so that the figure does not depend on how many the machine has), listed where 4x that error exceeds 0.8 of the stated tolerance (tolerance used: the larger of the stated one and 4x
# the figure; the entries between 0.8 and 1 change nothing -- they are listed so that a CPU whose BLAS sums in another order does not move a check
# across the line of test_cpu_fp32_stays_below_a_quarter_of_the_bars).  Long plain fp32 sums on the CPU: 2000 - 4600 terms per output.
FP32_REF_ERR = {
    "cadence-7 dx": 2.13e-06, "cadence-7 IN bwd sum g": 9.98e-07, "cadence-7 IN bwd sum g yhat": 1.12e-06, "cadence-7 BN bwd sum g": 9.79e-07,
    "cadence-7 BN bwd sum g yhat": 1.19e-06, "cadence-9 dx": 1.16e-06, "cadence-9 BN bwd sum g": 8.52e-07, "cadence-9 BN bwd sum g yhat": 9.07e-07,
    "cadence-17 y": 1.04e-06, "cadence-17 dx": 4.58e-06, "cadence-17 y+bias": 9.19e-07, "cadence-17 IN bwd sum g": 1.10e-06,
    "cadence-17 IN bwd sum g yhat": 1.03e-06, "cadence-17 BN bwd sum g yhat": 8.74e-07,
    "one-128-tile y": 2.25e-06, "one-128-tile dx": 8.02e-07, "one-128-tile y+bias": 1.74e-06, "one-128-tile IN sum": 9.35e-07,
    "one-128-tile IN sumsq": 9.16e-07, "one-128-tile BN sum": 8.48e-07, "one-128-tile BN sumsq": 8.57e-07, "tile-plus-one y": 2.13e-06,
    "tile-plus-one y+bias": 1.96e-06, "tile-plus-one IN sum": 1.35e-06, "tile-plus-one IN sumsq": 1.20e-06, "tile-plus-one BN sum": 1.09e-06,
    "tile-plus-one BN sumsq": 9.48e-07, "one-256-tile y": 2.43e-06, "one-256-tile dx": 1.03e-06, "one-256-tile y+bias": 2.25e-06,
    "one-256-tile IN sum": 1.32e-06, "257-rows y": 2.31e-06, "257-rows y+bias": 1.94e-06, "257-rows IN sum": 1.28e-06, "clips-per-tile y": 1.93e-06,
    "clips-per-tile dx": 2.24e-06, "clips-per-tile y+bias": 1.56e-06, "clips-per-tile IN sum": 9.15e-07, "clips-per-tile BN sum": 1.06e-06,
    "clips-per-tile IN bwd sum g": 9.24e-07, "clips-per-tile IN bwd sum g yhat": 1.16e-06, "clips-per-tile BN bwd sum g": 9.96e-07,
    "k1s1 dx": 8.05e-07, "k1s2 y": 9.50e-07, "k1s2 dx": 8.81e-07, "k1s2 dW": 3.69e-06, "k2s2 y": 1.54e-06, "k2s2 dW": 3.32e-06,
    "k2s2 y+bias": 1.25e-06, "k3s2p1 y": 1.70e-06, "k3s2p1 dx": 8.31e-07, "k3s2p1 dW": 1.97e-06, "k3s2p1 y+bias": 1.46e-06, "k3s2p1 BN sum": 8.61e-07,
    "k4s2p1-odd y": 3.17e-06, "k4s2p1-odd dx": 9.03e-07, "k4s2p1-odd dW": 2.01e-06, "k4s2p1-odd y+bias": 2.54e-06, "k4s2p1-odd IN sum": 9.63e-07,
    "k4s2p1-odd BN sum": 1.35e-06, "k4s2p1-even y": 1.45e-06, "k4s2p1-even dW": 3.07e-06, "k4s2p1-even y+bias": 1.27e-06, "k6x3 y": 2.47e-06,
    "k6x3 y+bias": 2.03e-06, "k6x3 IN sum": 1.33e-06, "k6x3 IN sumsq": 9.01e-07, "k6x3 BN sum": 1.16e-06, "wo-1 y": 1.68e-06, "wo-1 dx": 1.01e-06,
    "wo-1 y+bias": 1.55e-06, "wo-1 IN sum": 1.05e-06, "wo-1 IN sumsq": 2.09e-06, "wo-1 BN sum": 8.95e-07, "ho-wo-1-c256 y": 2.93e-06,
    "ho-wo-1-c256 dW": 2.47e-06, "ho-wo-1-c256 y+bias": 2.26e-06, "ho-wo-1-c256 IN sum": 2.93e-06, "ho-wo-1-c256 IN sumsq": 4.05e-06,
    "ho-wo-1-c256 BN sum": 9.10e-07, "ho-wo-1-c128 y": 2.10e-06, "ho-wo-1-c128 dW": 2.63e-06, "ho-wo-1-c128 y+bias": 1.78e-06,
    "ho-wo-1-c128 IN sum": 2.10e-06, "ho-wo-1-c128 IN sumsq": 3.25e-06, "ho-wo-1-c128 BN sum": 9.72e-07, "pad-k-1 dx": 1.82e-06,
    "pad-k-1 dW": 2.38e-06, "pad-k-1 IN bwd sum g yhat": 8.53e-07, "pad-k-1 BN bwd sum g yhat": 8.60e-07, "k3x5s2 y": 2.73e-06, "k3x5s2 dW": 2.47e-06,
    "k3x5s2 y+bias": 2.39e-06, "k3x5s2 BN sum": 1.06e-06, "two-classes y": 9.98e-07, "two-classes dW": 1.98e-06, "two-classes y+bias": 8.41e-07,
    "cap-c256 y": 1.22e-06, "cap-c256 dx": 8.28e-07, "cap-c256 y+bias": 1.01e-06, "cap-c320 y": 1.17e-06, "cap-c320 dx": 8.73e-07,
    "cap-c320 y+bias": 9.91e-07, "cap-c320 IN bwd sum g yhat": 8.46e-07, "cap-c320 BN bwd sum g yhat": 8.51e-07, "cap-c384 y": 1.24e-06,
    "cap-c384 dx": 9.46e-07, "cap-c384 dW": 3.18e-06, "cap-c384 y+bias": 1.11e-06, "cap-cin192 y": 2.13e-06, "cap-cin192 dW": 3.10e-06,
    "cap-cin192 y+bias": 1.94e-06, "cap-cin192 IN sum": 1.06e-06, "cap-cin192 BN sum": 1.04e-06, "cap-cin128 y": 1.49e-06, "cap-cin128 dx": 1.01e-06,
    "cap-cin128 dW": 3.31e-06, "cap-cin128 y+bias": 1.37e-06, "dw-128x128 y": 2.72e-06, "dw-128x128 dx": 1.19e-06, "dw-128x128 y+bias": 1.90e-06,
    "dw-128x128 IN sum": 1.59e-06, "dw-128x128 BN sum": 8.75e-07, "dw-64x64 y": 1.78e-06, "dw-64x64 dx": 2.19e-06, "dw-64x64 y+bias": 1.40e-06,
    "dw-64x64 BN sum": 1.04e-06, "dw-64x64 IN bwd sum g": 8.85e-07, "dw-64x64 IN bwd sum g yhat": 8.99e-07, "dw-64x64 BN bwd sum g yhat": 1.20e-06,
    "dw-64x128 y": 3.05e-06, "dw-64x128 y+bias": 2.52e-06, "dw-64x128 IN sum": 1.47e-06, "dw-64x128 BN sum": 1.39e-06, "cin32-k3 dx": 1.74e-06,
    "cin32-k3 IN bwd sum g": 1.03e-06, "cin32-k3 IN bwd sum g yhat": 1.10e-06, "cin32-k3 BN bwd sum g": 1.05e-06,
    "cin32-k3 BN bwd sum g yhat": 8.90e-07, "cin96-k3 y": 1.49e-06, "cin96-k3 dx": 1.90e-06, "cin96-k3 y+bias": 1.20e-06,
    "cin96-k3 IN bwd sum g": 1.01e-06, "cin96-k3 IN bwd sum g yhat": 9.63e-07, "cin96-k3 BN bwd sum g": 1.13e-06,
    "cin96-k3 BN bwd sum g yhat": 8.98e-07, "cin160-k3 y": 1.42e-06, "cin160-k3 dx": 9.25e-07, "cin160-k3 y+bias": 1.18e-06,
    "cin160-k3 IN sum": 9.00e-07, "cin32-k4s2 y": 1.04e-06, "cin32-k4s2 dW": 3.26e-06, "cin32-k4s2 y+bias": 8.96e-07, "cin96-k4s2 y": 1.57e-06,
    "cin96-k4s2 dx": 1.87e-06, "cin96-k4s2 dW": 3.49e-06, "cin96-k4s2 y+bias": 1.37e-06, "cin96-k4s2 IN sum": 8.13e-07, "cin96-k4s2 BN sum": 8.03e-07,
    "cin96-k4s2 BN bwd sum g": 9.22e-07, "cin160-k4s2 y": 1.95e-06, "cin160-k4s2 dx": 9.60e-07, "cin160-k4s2 dW": 2.35e-06,
    "cin160-k4s2 y+bias": 1.61e-06, "cin160-k4s2 IN sum": 9.15e-07, "cout64 y": 1.33e-06, "cout64 dx": 1.06e-06, "cout64 y+bias": 1.28e-06,
    "cout192 y": 1.42e-06, "cout192 dx": 1.89e-06, "cout192 y+bias": 1.06e-06, "cout192 BN bwd sum g": 9.52e-07, "cout320 y": 1.51e-06,
    "cout320 dx": 2.13e-06, "cout320 y+bias": 1.32e-06, "cout320 IN bwd sum g": 9.26e-07, "cout320 IN bwd sum g yhat": 1.28e-06,
    "cout320 BN bwd sum g": 1.29e-06, "cout320 BN bwd sum g yhat": 1.19e-06, "cout384 y": 1.31e-06, "cout384 dx": 2.51e-06,
    "cout384 y+bias": 1.02e-06, "cout384 IN bwd sum g": 8.94e-07, "cout384 IN bwd sum g yhat": 1.09e-06, "cout384 BN bwd sum g": 1.13e-06,
    "cout384 BN bwd sum g yhat": 8.99e-07, "dw-64x64-b y": 1.24e-06, "dw-64x64-b dx": 1.52e-06, "dw-64x64-b y+bias": 1.01e-06,
    "dw-64x64-b IN bwd sum g": 9.21e-07, "dw-64x64-b IN bwd sum g yhat": 8.37e-07,
   
   
    "stat-in-31 y": 9.15e-07, "stat-in-31 dx": 1.77e-06, "stat-in-31 dW": 2.75e-06,
    "stat-in-31 IN bwd sum g yhat": 9.73e-07, "stat-in-32 y": 1.40e-06, "stat-in-32 dx": 1.83e-06, "stat-in-32 y+bias": 1.15e-06,
    "stat-in-32 IN sumsq": 8.46e-07, "stat-in-32 IN bwd sum g": 1.08e-06, "stat-in-32 IN bwd sum g yhat": 1.53e-06,
    "stat-in-32 BN bwd sum g": 8.92e-07, "stat-in-32 BN bwd sum g yhat": 1.50e-06, "stat-in-33 y": 1.34e-06, "stat-in-33 dx": 2.29e-06,
    "stat-in-33 y+bias": 1.03e-06, "stat-in-33 IN sumsq": 9.17e-07, "stat-in-33 IN bwd sum g": 9.88e-07, "stat-in-33 IN bwd sum g yhat": 1.20e-06,
    "stat-in-33 BN bwd sum g": 9.87e-07, "stat-in-33 BN bwd sum g yhat": 8.42e-07, "stat-dx-31 y": 9.37e-07, "stat-dx-31 dx": 1.10e-06,
    "stat-dx-31 dW": 2.57e-06, "stat-dx-31 y+bias": 8.88e-07, "stat-dx-32 y": 1.17e-06, "stat-dx-32 dx": 9.17e-07, "stat-dx-32 dW": 2.53e-06,
    "stat-dx-32 y+bias": 1.01e-06, "stat-dx-33 y": 1.05e-06, "stat-dx-33 dx": 1.19e-06, "stat-dx-33 dW": 2.66e-06, "stat-dx-33 y+bias": 8.52e-07,
    "stat64-in-63 y": 1.37e-06, "stat64-in-63 dx": 1.13e-06, "stat64-in-63 y+bias": 1.13e-06, "stat64-in-64 y": 1.42e-06, "stat64-in-64 dx": 1.10e-06,
    "stat64-in-64 y+bias": 1.28e-06, "stat64-in-65 y": 1.33e-06, "stat64-in-65 dx": 1.10e-06, "stat64-in-65 y+bias": 1.18e-06, "cin48 y": 1.03e-06,
    "cin48 dx": 9.11e-07, "cin48 y+bias": 8.17e-07, "cout96 y": 1.64e-06, "cout96 dx": 1.19e-06, "cout96 y+bias": 1.39e-06, "cout48 y": 8.57e-07,
    "cout48 dx": 8.49e-07, "cout48 y+bias": 8.28e-07, "splitk-2d y": 1.06e-06, "splitk-2d dx": 9.23e-07, "splitk-2d y+bias": 8.40e-07,
    "splitk-2d BN sum": 8.21e-07, "random-0 dx": 9.20e-07, "random-1 y": 2.37e-06, "random-1 dx": 1.85e-06, "random-1 dW": 1.73e-06,
    "random-1 y+bias": 2.16e-06, "random-1 IN sum": 1.01e-06, "random-1 BN sum": 1.22e-06, "random-1 IN bwd sum g": 8.74e-07,
    "random-1 BN bwd sum g": 8.60e-07, "random-2 dx": 1.09e-06, "random-3 y": 9.46e-07, "random-4 y": 2.29e-06, "random-4 dx": 1.16e-06,
    "random-4 dW": 2.03e-06, "random-4 y+bias": 1.95e-06, "random-4 BN sum": 1.14e-06, "random-5 dx": 1.63e-06, "random-5 dW": 2.38e-06,
    "random-6 y": 2.23e-06, "random-6 dx": 1.40e-06, "random-6 y+bias": 1.87e-06, "random-6 IN sum": 1.08e-06, "random-6 BN sum": 1.13e-06,
    "random-7 y": 1.33e-06, "random-7 y+bias": 1.02e-06,
}


def tol_for(key, stated):
    e32 = FP32_REF_ERR.get(key)
    return stated if e32 is None else max(stated, 4.0 * e32)


def cpu_fp32_rows(c):
    """(key, fp32-torch-vs-float64 error, stated tolerance) of every check of a case"""
    tag = c[0]
    d64 = reference(c)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # ONE thread: plain sums in the library's own fixed order (a threaded dW splits its reduction by the thread count)
    try:
        return _cpu_fp32_rows(c, tag, d64, reference(c, torch.float32, d64))
    finally:
        torch.set_num_threads(threads)


def _cpu_fp32_rows(c, tag, d64, d32):
    rows = [(tag + " y", rel_err(d32.y, d64.y), TOL_Y), (tag + " dx", rel_err(d32.dx, d64.dx), TOL_DX), (tag + " dW", rel_err(d32.dw, d64.dw), TOL_DW)]
    b = bias_of(c)
    rows.append((tag + " y+bias", rel_err(d32.y + b.float(), d64.y + b), TOL_Y))
    for mode, groups in modes(c):
        for q, a, r in zip(("sum", "sumsq"), fwd_sums(d32.y, groups), fwd_sums(d64.y, groups)):
            rows.append(("%s %s %s" % (tag, mode, q), rel_err(a, r), TOL_SUMS))
    for mode, groups in holder_modes(c):
        bl = below(c, mode, groups)
        for q, a, r in zip(("sum g", "sum g yhat"), bwd_sums(bl, d32.dx, torch.float32), bwd_sums(bl, d64.dx)):
            rows.append(("%s %s bwd %s" % (tag, mode, q), rel_err(a, r), TOL_BSUMS))
    return rows


@pytest.fixture()
def routed(ops):  # noqa: F811
    prev = ops.F32_SPLIT
    yield ops
    ops.F32_SPLIT = prev
    ops.clear_plans()


def _holder(ops, c, bl, groups):
    B, Hi, Wi, Cin = c[1:5]
    h = ops.NormBwdHolder()
    h.y = bl["y"].reshape(B, Hi, Wi, Cin).float().to(DEV)
    h.mean, h.rstd = bl["mean"].reshape(-1).float().to(DEV), bl["rstd"].reshape(-1).float().to(DEV)
    if bl["gamma"] is not None:
        h.gamma, h.beta = bl["gamma"].float().to(DEV), bl["beta"].float().to(DEV)
    h.groups, h.slope = groups, SLOPE
    return h


def _poison(*shapes):
    """NaN-filled tensors of the sizes the op allocates with torch.empty (the output; for an input gradient the transposed weights before it, which
    share the allocator's pool from 1 MB up and could otherwise take the output's NaN block), allocated together and freed: an unwritten row
    cannot hide behind stale zeros"""
    ts = [torch.full(shape, float("nan"), device=DEV) for shape in shapes]
    del ts


def _param(ops, w):
    return torch.nn.Parameter(ops.to_weight_layout(w.float()).to(DEV))


def run_case(ops, c, d, belows, expect, label, split):
    tag = c[0]
    dev = torch.device(DEV, torch.cuda.current_device())
    got = served(ops, c, dev)
    assert got == expect, "%s%s: served by %r, the table says %r" % (tag, label, got, expect)
    name = tag + label
    errs = {}
    run_forward(ops, c, d, name, errs)
    run_backward(ops, c, d, belows, expect, name, errs, (tag, split) in ACCUMULATE)
    assert not ops.streamk_error_codes(), name
    print("  case %-24s fwd %-36s dX %-52s dW %-30s %-28s | %s" % (name, expect.fwd, expect.dx, expect.dw, expect.stats,
                                                                   "  ".join("%s %.2e" % kv for kv in errs.items())))


def _note(errs, key, e):
    errs[key] = max(errs.get(key, 0.0), e)


def run_forward(ops, c, d, name, errs, tol=None):
    """the forward half of a case: y without and with a bias, ConvStatsFn under every grouping conv_stats_fusable accepts"""
    tag, tol = c[0], tol or tol_for  # (tol: another module's table of measured fp32 reference errors)
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    xd = d.x.float().to(DEV)
    wd = _param(ops, d.w)

    def note(key, e):
        _note(errs, key, e)

    # ---- forward without and with a bias, twice
    bias = bias_of(c)
    _poison((B, Ho, Wo, Cout))
    y0 = ops.conv_forward(xd, wd, None, s, p)
    _poison((B, Ho, Wo, Cout))
    y1 = ops.conv_forward(xd, wd, None, s, p)
    _poison((B, Ho, Wo, Cout))
    yb = ops.conv_forward(xd, wd, bias.float().to(DEV), s, p)
    torch.cuda.synchronize()
    note("y", rel_err(y0, d.y))
    check(name + " y", y0, d.y, tol(tag + " y", TOL_Y))
    check(name + " y+bias", yb, d.y + bias, tol(tag + " y+bias", TOL_Y))
    assert torch.equal(y0, y1), "%s: the second forward run differs from the first" % name
    # ---- forward with the statistics epilogue, under each grouping for which conv_stats_fusable says yes
    for mode, groups in modes(c):
        want = fwd_fuses(ops, c, groups)
        assert bool(ops.conv_stats_fusable(xd, wd, s, p, groups)) == want, "%s: conv_stats_fusable(%s) is not %r" % (name, mode, want)
        if not want:
            continue
        runs = []
        for _rep in range(2):
            _poison((B, Ho, Wo, Cout))
            with torch.no_grad():
                runs.append(ops.ConvStatsFn.apply(xd, wd, s, p, groups, None))
        torch.cuda.synchronize()
        (ys, sums), (ys1, sums1) = runs
        note("y", rel_err(ys, d.y))
        check("%s y (%s statistics)" % (name, mode), ys, d.y, tol(tag + " y", TOL_Y))
        assert torch.equal(ys, ys1) and torch.equal(sums, sums1), "%s: the second %s statistics run differs from the first" % (name, mode)
        sums = sums.view(groups, Cout, 2)
        for k, (q, ref) in enumerate(zip(("sum", "sumsq"), fwd_sums(d.y, groups))):
            note(mode + " " + q, rel_err(sums[..., k], ref))
            check("%s %s %s" % (name, mode, q), sums[..., k], ref, tol("%s %s %s" % (tag, mode, q), TOL_SUMS))


def run_backward(ops, c, d, belows, expect, name, errs, accumulate, tol=None):
    """the backward half of a case (callable alone: tests/test_reserved_conv_sweep_gpu.py runs it under a reserve): dx under three holders, the
    backward sums where ``expect.stats`` says they fuse, dW; ``accumulate``: a second dW call and a call onto a pre-filled .grad as well"""
    tag, tol = c[0], tol or tol_for  # (tol: another module's table of measured fp32 reference errors)
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    dev = torch.device(DEV, torch.cuda.current_device())
    xd, gyd = d.x.float().to(DEV), d.gy.float().to(DEV)
    wd = _param(ops, d.w)

    def note(key, e):
        _note(errs, key, e)

    # ---- input gradient: no holder, IN holder, BN holder; twice each
    dead = unreachable(c)
    for mode, groups in [(None, 0)] + holder_modes(c):  # (one row per group: every pre-activation sits ON the kink -- no holder there)
        runs = []
        for _rep in range(2):
            h = None if mode is None else _holder(ops, c, belows[mode], groups)
            _poison((Cin, kh * kw, Cout), (B, Hi, Wi, Cin))
            runs.append((ops.conv_input_grad(gyd, wd, (B, Hi, Wi, Cin), s, p, h), h))
        torch.cuda.synchronize()
        (dxd, h), (dxd1, h1) = runs
        what = "%s dx%s" % (name, "" if mode is None else " (%s holder)" % mode)
        note("dx", rel_err(dxd, d.dx))
        check(what, dxd, d.dx, tol(tag + " dx", TOL_DX))
        assert torch.equal(dxd, dxd1), "%s: the second run differs from the first" % what
        if bool(dead.any()):
            z = dxd[:, dead.to(DEV)]
            assert bool((z == 0).all()) and not bool(torch.signbit(z).any()), "%s: unreachable input pixels are not exactly +0" % what
        if h is not None:
            fused = dx_fuses(ops, c, groups, dev)
            assert (h.sums is not None) == fused, "%s: backward statistics %s" % (what, "missing" if fused else "accumulated where the routing says no")
            assert fused == (mode in expect.stats.split("| dx ")[1].split())
            if fused:
                assert torch.equal(h.sums, h1.sums), "%s: the second run's statistics differ from the first's" % what
                bs = h.sums.view(groups, Cin, 2)
                for k, (q, ref) in enumerate(zip(("sum g", "sum g yhat"), bwd_sums(belows[mode], d.dx))):
                    note("%s %s" % (mode, q), rel_err(bs[..., k], ref))
                    check("%s %s bwd %s" % (name, mode, q), bs[..., k], ref, tol("%s %s bwd %s" % (tag, mode, q), TOL_BSUMS))
    # ---- weight gradient into a fresh .grad, twice; for one case per kernel also a second call and a call onto a pre-filled .grad
    tol_dw = tol(tag + " dW", TOL_DW)
    ops.conv_weight_grad(xd, gyd, wd, s, p)
    wd1 = _param(ops, d.w)
    ops.conv_weight_grad(xd, gyd, wd1, s, p)
    torch.cuda.synchronize()
    note("dW", rel_err(wd.grad, d.dw))
    check(name + " dW", wd.grad, d.dw, tol_dw)
    assert torch.equal(wd.grad, wd1.grad), "%s: the second dW run differs from the first" % name
    if accumulate:
        ops.conv_weight_grad(xd, gyd, wd, s, p)
        check(name + " dW, second call adds", wd.grad, 2.0 * d.dw, tol_dw)
        fill = (((torch.arange(d.dw.numel(), dtype=torch.float64) * 7919) % 13 - 6.0) * 0.125 * float(d.dw.abs().max())).reshape(d.dw.shape)
        wd.grad = ops.to_weight_layout(fill.float()).to(DEV)
        assert wd.grad.stride() == wd.stride()
        ops.conv_weight_grad(xd, gyd, wd, s, p)
        torch.cuda.synchronize()
        check(name + " dW onto a pre-filled .grad", wd.grad, fill.float().double() + d.dw, tol_dw)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_f32_conv_sweep(routed, tag):
    """Every case under the production routing (ops.F32_SPLIT = True), the BOTH cases on the fp32-MFMA kernels as well: y without and with a bias,
    forward sums, dx (three holders), backward sums, dW against float64 on the same operands; second runs bit-identical; unreachable input pixels
    exactly +0; the kernel that served each launch is the table's; the error word stays clear."""
    ops, c = routed, CASE[tag]
    d = reference(c)
    belows = {mode: below(c, mode, groups) for mode, groups in holder_modes(c)}
    ops.F32_SPLIT = True
    ops.clear_plans()
    run_case(ops, c, d, belows, EXPECT[tag], "", True)
    if tag in BOTH:
        ops.F32_SPLIT = False
        ops.clear_plans()
        assert EXPECT_MFMA[tag] != EXPECT[tag]
        run_case(ops, c, d, belows, EXPECT_MFMA[tag], " [fp32 MFMA]", False)


def _clamped(t):
    """|value| into [2^-10, 2^4], fp32-representable"""
    return f32(torch.where(t < 0, -1.0, 1.0) * t.abs().clamp(2.0 ** -10, 2.0 ** 4))


@pytest.mark.gpu
@pytest.mark.parametrize("tag,split", SCALED, ids=["%s-%s" % (t, "split" if sp else "mfma") for t, sp in SCALED])
def test_power_of_two_scaling(routed, tag, split):
    """x 2^a, w 2^b, gy 2^c: y, dx and dW are bit-identical to the unscaled run times 2^(a+b), 2^(b+c), 2^(a+c) (see the docstring: derived)."""
    ops, c = routed, CASE[tag]
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    ops.F32_SPLIT = split
    ops.clear_plans()
    dev = torch.device(DEV, torch.cuda.current_device())
    assert served(ops, c, dev) == (EXPECT if split else EXPECT_MFMA)[tag]
    g = torch.Generator().manual_seed(zlib.crc32((tag + " scaled").encode()))
    x = _clamped(torch.randn(B, Hi, Wi, Cin, generator=g, dtype=torch.float64))
    w = _clamped(torch.randn(Cout, Cin, kh, kw, generator=g, dtype=torch.float64) * (2.0 / (Cin * kh * kw)) ** 0.5)
    gy = _clamped(torch.randn(B, Ho, Wo, Cout, generator=g, dtype=torch.float64))

    def run(a, b, cc):
        xd, gyd = (x * 2.0 ** a).float().to(DEV), (gy * 2.0 ** cc).float().to(DEV)
        wd = _param(ops, w * 2.0 ** b)
        assert torch.equal(xd.double().cpu(), x * 2.0 ** a) and torch.equal(wd.detach().double().cpu(), w * 2.0 ** b)  # the scaled operands are exact
        y = ops.conv_forward(xd, wd, None, s, p)
        dx = ops.conv_input_grad(gyd, wd, (B, Hi, Wi, Cin), s, p)
        ops.conv_weight_grad(xd, gyd, wd, s, p)
        torch.cuda.synchronize()
        return y, dx, wd.grad

    y0, dx0, dw0 = run(0, 0, 0)
    for a, b, cc in SCALES:
        y1, dx1, dw1 = run(a, b, cc)
        for q, t0, t1, e in (("y", y0, y1, a + b), ("dx", dx0, dx1, b + cc), ("dW", dw0, dw1, a + cc)):
            assert torch.equal(t1, t0 * 2.0 ** e), "%s %s under (a, b, c) = %r: %d of %d elements are not the unscaled ones times 2^%d" % (
                tag, q, (a, b, cc), int((t1 != t0 * 2.0 ** e).sum()), t0.numel(), e)
    assert not ops.streamk_error_codes()


# =============================================================================================================================
# host only: the table against the planner, the CPU fp32 error against the bars, and what the bars reject
# =============================================================================================================================
def segment_lengths(plan):
    """K steps of every (range, tile) segment of a stream-K plan, from its own tables (csrc/convsk.hip plan_build: P[3] & 0xffff = G ranges,
    P[6] = T tiles, P[7] = S steps, P[12] = offset of tilecum[T + 1]; range r runs the steps [r S / G, (r + 1) S / G)): the loop lengths the
    kernel's flush counter sees"""
    P = plan.host
    G, T, S = P[3] & 0xffff, P[6], P[7]
    cum = P[P[12]:P[12] + T + 1]
    assert cum[0] == 0 and cum[T] == S
    out, tile = collections.Counter(), 0
    for r in range(G):
        a, b = r * S // G, (r + 1) * S // G
        while a < b:
            while cum[tile + 1] <= a:
                tile += 1
            e = min(b, cum[tile + 1])
            out[e - a] += 1
            a = e
    return out


def _plans_now(split, tags):
    from speechdrivestemplates_amd import ops as o
    cpu = torch.device("cpu")
    prev = o.F32_SPLIT
    try:
        o.F32_SPLIT = split
        o.clear_plans()
        return {t: served(o, CASE[t], cpu) for t in tags}
    finally:
        o.F32_SPLIT = prev
        o.clear_plans()


def _form(name):
    return name.split(" x")[0].split(" k=")[0].split(" per class")[0]


FWD_DX_FORMS = ("convbf2_kernel<float, 128, 128>", "convbf2_kernel<float, 256, 64>", "convsk_kernel<128, 128>", "convsk_kernel<128, 64>")


def test_table_covers_the_planner():
    """Every case is routed as EXPECT / EXPECT_MFMA say (sdt_convsk_supported_t, sdt_convsk_plan_build_t, sdt_convsk_dw_supported_t,
    sdt_conv_taps_splitk_hint and sdt_conv_taps_stats_supported through ops, plans kept on the host), and the tables hold every kernel family and
    tile form: each forward / dx form in at least four cases, each dW form in at least three."""
    from speechdrivestemplates_amd import ops as o
    now, now_mfma = _plans_now(True, [c[0] for c in CASES]), _plans_now(False, list(BOTH))
    assert now == EXPECT, {t: (now[t], EXPECT.get(t)) for t in now if now[t] != EXPECT.get(t)}
    assert now_mfma == EXPECT_MFMA, {t: (now_mfma[t], EXPECT_MFMA.get(t)) for t in now_mfma if now_mfma[t] != EXPECT_MFMA.get(t)}
    for c in CASES:
        B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
        assert B * Ho * Wo <= MAX_PIXELS and B * Ho * Wo * Cout * kh * kw * Cin <= MAX_MACS and kh * kw <= 20, c
    assert set(HAND) <= set(CASES) and len(BOTH) >= 8
    both = list(EXPECT.values()) + list(EXPECT_MFMA.values())
    count = collections.Counter()
    for e in both:
        for form in {_form(e.fwd), _form(e.dx)}:
            count[form] += 1
    for form in FWD_DX_FORMS + ("sdt_conv_taps_f32", "sdt_conv_taps_splitk_f32", "sdt_conv_taps_multi_f32"):
        assert count[form] >= 4, (form, count)
    for form in FWD_DX_FORMS:  # ... as a forward AND as an input-gradient launch (but ops._sk_wanted keeps convsk_kernel<128, 64> for forwards)
        assert any(_form(e.fwd) == form for e in both) and (form == "convsk_kernel<128, 64>" or any(_form(e.dx) == form for e in both)), form
    assert not any(_form(e.dx) == "convsk_kernel<128, 64>" for e in both)
    assert any(_form(e.fwd) == "sdt_conv_taps_splitk_f32" for e in both)                       # the hint > 1 on a 2-D launch
    assert any(e.dx.startswith("sdt_conv_taps_splitk_f32 per class") for e in both)            # dx_pack is None
    assert sum(1 for e in both if ":sdt_conv_taps_stats_f32" in e.stats) >= 4                  # sdt_conv_taps_stats_f32
    assert sum(1 for e in both if e.dx.startswith("sdt_conv_taps_multi_f32") and not e.stats.endswith("dx -")) >= 4  # ... with fused backward statistics
    assert sum(1 for e in both if e.dx.startswith("sdt_conv_taps_multi_f32") and e.stats.endswith("dx -")) >= 4      # ... and without
    dws = collections.Counter(e.dw for e in both)
    for kernel in ("convx3_dw_kernel", "convsk_dw_kernel"):
        for tile in ("<128, 128>", "<128, 64>", "<64, 128>", "<64, 64>"):
            assert dws[kernel + tile] >= 3, (kernel + tile, dws)
    assert dws["sdt_conv_dw_det_f32"] >= 3
    assert {EXPECT[t].dw if sp else EXPECT_MFMA[t].dw for t, sp in ACCUMULATE} >= {
        "convx3_dw_kernel<128, 128>", "convx3_dw_kernel<128, 64>", "convx3_dw_kernel<64, 128>", "convx3_dw_kernel<64, 64>", "convsk_dw_kernel<128, 128>",
        "convsk_dw_kernel<64, 64>", "sdt_conv_dw_det_f32"}
    for t in BOTH:  # the two settings route differently
        assert EXPECT[t] != EXPECT_MFMA[t] and "convbf2" not in "".join(EXPECT_MFMA[t][:3]) and "convx3" not in EXPECT_MFMA[t].dw, t
    assert {int(e.dx.rsplit(" x", 1)[1].split()[0]) for e in both if " x" in e.dx} == {1, 2, 4}
    assert {c[4] for c in CASES} >= {3, 24, 32, 48, 64, 96, 128, 160, 192, 256} and {c[5] for c in CASES} >= {6, 48, 64, 96, 128, 192, 256, 320, 384}
    # power-of-two scaling: one case per kernel family
    fam = set()
    for t, sp in SCALED:
        e = (EXPECT if sp else EXPECT_MFMA)[t]
        fam |= {"fwd " + _form(e.fwd).split("<")[0], "dx " + _form(e.dx).split("<")[0], "dW " + e.dw.split("<")[0]}
    assert fam >= {"fwd convbf2_kernel", "fwd convsk_kernel", "fwd sdt_conv_taps_f32", "fwd sdt_conv_taps_splitk_f32", "dx convbf2_kernel", "dx convsk_kernel",
                   "dx sdt_conv_taps_multi_f32", "dx sdt_conv_taps_splitk_f32", "dW convx3_dw_kernel", "dW convsk_dw_kernel", "dW sdt_conv_dw_det_f32"}, fam
    # the flush cadence: 7, 9 and 17 K steps per tile on the split kernel
    # ... and every workgroup runs ONE loop of exactly that length: each range of the plan is one whole tile
    prev = o.F32_SPLIT
    try:
        o.F32_SPLIT = True
        o.clear_plans()
        for t, steps in (("cadence-7", CADENCE - 1), ("cadence-9", CADENCE + 1), ("cadence-17", 2 * CADENCE + 1)):
            B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(CASE[t])
            assert kh * kw * Cin // 32 == steps and EXPECT[t].fwd == "convbf2_kernel<float, 128, 128>", t
            g = o.fwd_geom(B, Hi, Wi, Cin, Cout, kh, kw, s, p)
            for rpg in (0, Ho * Wo, B * Ho * Wo):  # conv_forward, ConvStatsFn under IN and under BN
                plan = o._sk_plan(g, 1, rpg, 1, torch.device("cpu"), forward=True)
                assert o._sk_name(plan) == EXPECT[t].fwd and segment_lengths(plan) == {steps: 256}, (t, rpg, segment_lengths(plan))
    finally:
        o.F32_SPLIT = prev
        o.clear_plans()
    # the statistics thresholds from both sides: 31 / 32 / 33 rows per group and class on a stream-K dx plan, 63 / 64 / 65 on the fall-back kernels
    cpu = torch.device("cpu")
    for t in ("stat-in", "stat-dx"):
        assert [dx_fuses(o, CASE["%s-%d" % (t, r)], CASE["%s-%d" % (t, r)][1], cpu) for r in (31, 32, 33)] == [False, True, True], t
    assert all(EXPECT["stat-dx-%d" % r].dx.startswith("convbf2_kernel<float") for r in (31, 32, 33))
    assert all(EXPECT["stat-in-%d" % r].dx.startswith("convsk_kernel") for r in (32, 33))  # (31 x 1 images: too few live taps for a plan; wo-1 has
    assert EXPECT["wo-1"].dx.startswith("convsk_kernel") and not dx_fuses(o, CASE["wo-1"], CASE["wo-1"][1], cpu)  # 27 rows per class on this kernel)
    for t, grp in (("stat64-in", "IN"), ("stat64-bn", "BN")):
        es = [EXPECT["%s-%d" % (t, r)] for r in (63, 64, 65)]
        assert all(e.fwd == "sdt_conv_taps_f32" and e.dx.startswith("sdt_conv_taps_multi_f32") for e in es), t
        assert [grp + ":sdt_conv_taps_stats_f32" in e.stats.split(" | ")[0] for e in es] == [False, True, True], t
        assert [grp in e.stats.split("| dx ")[1].split() for e in es] == [False, True, True], t
    # refusals for the channel counts, asserted on the host before any launch: no stream-K plan of any kind
    for t in ("cin3", "cin24", "cin48", "cout96", "cout48", "cout6"):
        e = EXPECT[t]
        assert e.fwd.startswith("sdt_conv_taps") and e.dx.startswith("sdt_conv_taps") and e.dw == "sdt_conv_dw_det_f32", (t, e)
    for t in ("cin3", "cin24", "cin48"):  # the scalar loader: no fused forward statistics either
        assert EXPECT[t].stats.startswith("fwd - |"), t


def test_cpu_fp32_stays_below_a_quarter_of_the_bars():
    """fp32 torch on the CPU against float64 on the inputs of every check: below a quarter of the stated bar, or listed in FP32_REF_ERR with the
    figure measured here."""
    seen = set()
    for c in CASES:
        for key, e, stated in cpu_fp32_rows(c):
            seen.add(key)
            if key in FP32_REF_ERR:  # the listed figure is this measurement (another CPU / BLAS may sum in another order: within a factor 1.5)
                assert FP32_REF_ERR[key] / 1.5 <= e <= 1.5 * FP32_REF_ERR[key] and 4.0 * FP32_REF_ERR[key] > 0.8 * stated, (key, e, FP32_REF_ERR[key])
            else:
                assert 4.0 * e <= stated, "%s: fp32 torch on the CPU errs by %.2e, more than a quarter of %.1e: list it in FP32_REF_ERR" % (key, e, stated)
    assert set(FP32_REF_ERR) <= seen, set(FP32_REF_ERR) - seen


def _planes(t):
    """the three bf16 planes of fp32-representable values (round to nearest even, as the loader splits)"""
    h = t.float().bfloat16().double()
    m = (t - h).float().bfloat16().double()
    lo = (t - h - m).float().bfloat16().double()
    return h, m, lo


def test_bars_discriminate():
    """On the float64 references of a strided case and of an IN case with several clips per tile: fp32 torch passes every bar; a dropped tap, a
    dropped 32-channel K step, a last row left at zero, a row credited to the next clip's statistics, a parity class of dx left at zero, the last
    dW columns left at zero each fail theirs.  A split that keeps only the three largest of the six plane products (hh, hm, mh: the bf16x3
    arithmetic) fails the y and the dx bar, narrowly (4.3e-6 and 5.0e-6 against 4e-6), while all six pass at a quarter; on dW it reaches 4.6e-6 / 5.7e-6,
    INSIDE the 8e-6 the random sweeps state for dW -- that bar alone would not notice it (asserted here as "more than half of the bar")."""
    for tag in ("k3s2p1-small", "clips-per-tile"):
        c = CASE[tag]
        B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
        d = reference(c)
        d32 = reference(c, torch.float32, d)
        assert rel_err(d32.y, d.y) < TOL_Y and rel_err(d32.dx, d.dx) < TOL_DX and rel_err(d32.dw, d.dw) < TOL_DW
        sm, sq = fwd_sums(d.y, B)
        assert rel_err(sm.float(), sm) < TOL_SUMS and rel_err(sq.float(), sq) < TOL_SUMS
        # one tap dropped; one 32-channel K step dropped
        w_tap = d.w.clone()
        w_tap[:, :, kh - 1, kw - 1] = 0
        x_k = d.x.clone()
        x_k[..., Cin - 32:] = 0
        for mut in (d._replace(w=w_tap), d._replace(x=x_k)):
            assert rel_err(reference(c, data=mut).y, d.y) > TOL_Y
        assert rel_err(reference(c, data=d._replace(w=w_tap)).dx, d.dx) > TOL_DX
        gy_k = d.gy.clone()
        gy_k[..., Cout - 32:] = 0  # (the K steps of dx run over Cout)
        assert rel_err(reference(c, data=d._replace(gy=gy_k)).dx, d.dx) > TOL_DX
        gy_row = d.gy.clone()
        gy_row[-1, -1, -1 - (B * Ho * Wo - 1) % 32:] = 0  # dW: the last, partly filled 32-row K step dropped
        assert rel_err(reference(c, data=d._replace(gy=gy_row)).dw, d.dw) > TOL_DW
        # the last row of the M tail left at zero
        y0 = d.y.clone()
        y0[-1, -1, -1] = 0
        assert rel_err(y0, d.y) > TOL_Y
        # the last row of a clip's plane credited to the next clip's statistics
        last = d.y[0, -1, -1]
        for ref, row in ((sm, last), (sq, last * last)):
            moved = ref.clone()
            moved[0] -= row
            moved[1] += row
            assert rel_err(moved, ref) > TOL_SUMS, tag
        # the last 32 columns of the (tap, channel) axis of dW left at zero
        dw0 = d.dw.clone()
        dw0[:, Cin - 32:, kh - 1, kw - 1] = 0
        assert rel_err(dw0, d.dw) > TOL_DW
        if s == 2:  # one parity class of dx left at zero
            for py in range(2):
                for px in range(2):
                    dx0 = d.dx.clone()
                    dx0[:, py::2, px::2] = 0
                    assert rel_err(dx0, d.dx) > TOL_DX
        # backward statistics: a row credited to the next clip
        bl = below(c, "IN", B)
        g0, g1 = bwd_sums(bl, d.dx)
        assert rel_err(g0.float(), g0) < TOL_BSUMS and rel_err(g1.float(), g1) < TOL_BSUMS
        one = dict(bl, y=bl["y"][:, -1:], mean=bl["mean"], rstd=bl["rstd"])
        r0, r1 = bwd_sums(one, d.dx.reshape(B, Hi * Wi, Cin)[:, -1:])
        for ref, row in ((g0, r0), (g1, r1)):
            moved = ref.clone()
            moved[0] -= row[0]
            moved[1] += row[0]
            assert rel_err(moved, ref) > TOL_BSUMS
        # the split: all six products (hh, hm, mh, hl, lh, mm) pass; the three largest alone (hh, hm, mh: bf16x3) fail
        conv = lambda a, b: F.conv2d(a.permute(0, 3, 1, 2), b, None, s, p).permute(0, 2, 3, 1)  # noqa: E731
        (xh, xm, xl), (wh, wm, wl) = _planes(d.x), _planes(d.w)
        three = conv(xh, wh) + conv(xh, wm) + conv(xm, wh)
        six = three + conv(xh, wl) + conv(xl, wh) + conv(xm, wm)
        assert rel_err(six, d.y) < TOL_Y / 4 and rel_err(three, d.y) > TOL_Y, (tag, rel_err(six, d.y), rel_err(three, d.y))
        (gh, gm, gl) = _planes(d.gy)
        dconv = lambda a, b: _dx_of(c, a, b)  # noqa: E731
        three = dconv(gh, wh) + dconv(gh, wm) + dconv(gm, wh)
        six = three + dconv(gh, wl) + dconv(gl, wh) + dconv(gm, wm)
        assert rel_err(six, d.dx) < TOL_DX / 4 and rel_err(three, d.dx) > TOL_DX, (tag, rel_err(six, d.dx), rel_err(three, d.dx))
        wconv = lambda a, b: _dw_of(c, a, b)  # noqa: E731
        three = wconv(xh, gh) + wconv(xh, gm) + wconv(xm, gh)
        six = three + wconv(xh, gl) + wconv(xl, gh) + wconv(xm, gm)
        print("  %s: three of six products: dW rel-max-err %.2e (bar %.1e)" % (tag, rel_err(three, d.dw), TOL_DW))
        assert rel_err(six, d.dw) < TOL_DW / 4 and rel_err(three, d.dw) > TOL_DW / 2, (tag, rel_err(six, d.dw), rel_err(three, d.dw))


def _dx_of(c, gy, w):
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    return torch.nn.grad.conv2d_input((B, Cin, Hi, Wi), w, gy.permute(0, 3, 1, 2), s, p).permute(0, 2, 3, 1)


def _dw_of(c, x, gy):
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    return torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (Cout, Cin, kh, kw), gy.permute(0, 3, 1, 2), s, p)


# =============================================================================================================================
# `python tests/test_f32_conv_sweep_gpu.py` prints the FP32_REF_ERR entries (fp32 torch on the CPU against float64), `--plans` the tables
# =============================================================================================================================
def _measure_fp32_ref_err():
    for c in CASES:
        rows = cpu_fp32_rows(c)
        print("# %-16s worst fp32-vs-float64 / stated tolerance: %.2f" % (c[0], max(e / t for _k, e, t in rows)), flush=True)
        for key, e, t in rows:
            if 4.0 * e > 0.8 * t:
                print('    "%s": %.2e,' % (key, e), flush=True)


def _print_plans():
    for name, split, tags in (("EXPECT", True, [c[0] for c in CASES]), ("EXPECT_MFMA", False, list(BOTH))):
        now = _plans_now(split, tags)
        print("%s = {" % name)
        for t in tags:
            e = now[t]
            B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(CASE[t])
            print("    %-18s Served(%r, %r, %r, %r),  # M = %d" % ('"%s":' % t, e.fwd, e.dx, e.dw, e.stats, B * Ho * Wo))
        print("}")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _print_plans() if "--plans" in sys.argv else _measure_fp32_ref_err()
