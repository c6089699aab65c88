"""The bf16-storage Conv2d kernels (csrc/convbf.hip convbf2_kernel<bf16>: 256-row tiles, one workgroup per CU; the 128-row stream-K kernel
behind sdt_convsk_bf16; convbf_dw_kernel behind sdt_convsk_dw_bf16) swept over edge geometries against float64, through the public entry
points ops.ConvStatsFn, ops.conv_input_grad (with and without a NormBwdHolder) and ops.conv_weight_grad on bf16 tensors.

Operands are bf16-representable (x, gy, master weights), the reference is F.conv2d and its autograd in float64 on those same values: products
are exact in fp32, what remains is the fp32 accumulation and, for y / dx, ONE rounding to bf16.

Bars.  bf16 outputs (y, dx), per element (check_bf16 of test_edge_shapes_bf16_gpu.py):  |got - ref| <= 2^-8 |ref| + tol max|ref|, tol = 1e-5,
the fp32 accumulation tolerance test_bf16_gpu.py states for same-operand fp32 quantities.  fp32 outputs: rel-max 2e-5 (dW, forward sums; the
sums and the sums of squares each against their own maximum), 1e-4 (backward sums) as in test_bf16_gpu.py.  Where 4x the error of fp32 torch on
the CPU against float64 on the very inputs of a check is larger, that is the tolerance (FP32_REF_ERR; `python tests/test_bf16_conv_sweep_gpu.py`
prints the entries; nothing a kernel produced enters a tolerance).  test_bars_discriminate (host only) shows what these bars reject.

What the planner accepts (csrc/convsk.hip).  A forward / input-gradient launch needs S >= G K steps (G = 512 ranges on the 128-row kernel, and
4 G with G = 256 plus T >= 128 tiles on the 256-row kernel), a weight gradient cdiv(M, 64) >= 4 (512 / T) K steps: launches of one or two
tiles -- one row, fewer rows than a wave's 64, exactly one 128-row tile -- are REFUSED, the fp32 kernels take them and return fp32.  The table
keeps those geometries: EXPECT pins the refusal (a case cannot move to another kernel unnoticed) and the fall-back is held to the fp32 bar.
ConvStatsFn is only reached where conv_stats_fusable says so (>= 32 rows per statistics group: a 32-row accumulator block then holds at most
two groups); each case runs under every grouping that qualifies (IN: groups = B, BN: groups = 1).  The input gradient runs without a holder
and with an IN and a BN one (the BN one with affine parameters); below 32 rows per group and class the launch does not fuse the statistics.

Size cap per case: 5e9 multiply-adds, 8192 output pixels (B Ho Wo).  The 256 x 256 and 256 x 128 tiles of the 256-row kernel need more than
65280 rows in one launch: only an input gradient gets there under the cap (Ho = Wo = 1, many clips: 18 input pixels per output pixel)."""
import collections
import os
import random
import sys
import zlib

import pytest
import torch
import torch.nn.functional as F

from test_edge_shapes_bf16_gpu import BF, HALF_STEP, bf16_ratio, bf16r, check_bf16, off_kink_bf16, ops  # noqa: F401  (ops: the fixture)
from test_edge_shapes_gpu import DEV, EPS, KINK, check, rel_err

SLOPE = 0.2
TOL_BF16, TOL_DW, TOL_SUMS, TOL_BSUMS = 1e-5, 2e-5, 2e-5, 1e-4
MAX_MACS, MAX_PIXELS = 5e9, 8192

# (tag, B, Hi, Wi, Cin, Cout, kh, kw, s, p)
HAND = [
    # ---- rows the planner refuses (S < G): every launch falls back to the fp32 kernels
    ("one-row", 1, 1, 1, 64, 64, 1, 1, 1, 0),               # M = 1: one row; Ho = Wo = 1; B = 1
    ("sub-wave", 1, 5, 8, 256, 320, 3, 3, 1, 1),            # M = 40 < 64: fewer rows than one wave's share; M < 64 (the dW K step)
    ("one-128-tile", 2, 11, 11, 256, 320, 4, 4, 1, 0),      # M = 128: exactly one 128-row tile (S = 320 < 512: refused)
    ("k3s2p1-small", 2, 9, 11, 64, 64, 3, 3, 2, 1),         # M = 60: parity classes with 2x2, 2x1, 1x2, 1x1 taps through the fall-back
    # ---- row tails on the 128-row kernel
    ("tile-plus-one", 3, 4, 46, 256, 320, 4, 4, 1, 0),      # M = 129: one tile plus one row; M odd; Ho = 1; IN: 43 rows per clip, three clips in a tile
    ("one-256-tile", 1, 19, 19, 256, 320, 4, 4, 1, 0),      # M = 256: exactly one 256-row tile (two 128-row tiles, no tail); B = 1
    ("257-rows", 1, 4, 260, 256, 320, 4, 4, 1, 0),          # M = 257 (prime): a 256-row tile plus one row; Ho = 1; B = 1
    ("clips-per-tile", 12, 7, 9, 256, 320, 3, 3, 1, 1),     # IN with Ho Wo = 63 < a tile, no multiple of 32: a group ends inside a wave's rows
    # ---- taps and stride
    ("k1s1", 13, 17, 37, 256, 320, 1, 1, 1, 0),             # (1,1) s1 p0: four K steps per tile; M = 8177 odd
    ("k1s2", 13, 33, 73, 256, 320, 1, 1, 2, 0),             # (1,1) s2 p0: three of four input pixels unreachable (exactly +0)
    ("k2s2", 8, 65, 64, 256, 256, 2, 2, 2, 0),              # (2,2) s2 p0, Hi odd (last input row unreachable), Wi even; one tap per parity class
    ("k3s2p1", 8, 31, 40, 192, 256, 3, 3, 2, 1),            # (3,3) s2 p1: classes of 1 / 2 / 2 / 4 taps; taps * Cin = 9 x 192: 64-wide dW columns
    ("k4s2p1-odd", 5, 33, 41, 256, 128, 4, 4, 2, 1),        # (4,4) s2 p1 on odd Hi and Wi
    ("k4s2p1-even", 8, 64, 64, 64, 256, 4, 4, 2, 1),        # (4,4) s2 p1 on even Hi and Wi; M = 8192: whole tiles only
    ("k6x3", 4, 6, 130, 256, 256, 6, 3, 1, 0),              # (6,3) s1 p0 on Hi = 6: Ho = 1 (a kernel as tall as the input, like L7)
    ("wo-1", 100, 9, 3, 256, 192, 3, 3, 1, 0),              # Wo = 1; IN has 7 rows per clip (BN only forward); dX classes of 27 rows: IN not fused
    ("ho-wo-1-c256", 3640, 6, 3, 256, 64, 6, 3, 1, 0),      # Ho = Wo = 1; dX: 65520 rows x 256 channels: the 256 x 256 tile
    ("ho-wo-1-c128", 3640, 6, 3, 128, 64, 6, 3, 1, 0),      # Ho = Wo = 1; dX: the 256 x 128 tile
    ("pad-k-1", 4, 20, 30, 256, 192, 3, 3, 1, 2),           # pad = k - 1: the output is larger than the input
    ("k3x5s2", 9, 33, 40, 192, 128, 3, 5, 2, 1),            # non-square kernel with stride 2: classes of 2 / 3 / 4 / 6 taps
    ("two-classes", 4, 1, 1401, 256, 384, 1, 2, 2, 0),      # Hi = 1 under stride 2: two parity classes; Wi odd: the last column unreachable
    # ---- close to the size cap: the 256-row kernel's forward launches (T >= 128 tiles)
    ("cap-c256", 13, 19, 39, 64, 256, 3, 3, 1, 0),          # Cout = 256, few rows: the 128 x 128 rule; taps * Cin = 9 x 64
    ("cap-c320", 5, 39, 37, 64, 320, 3, 3, 1, 0),           # Cout = 320: 256 x 64 tiles, five column tiles; dW 64 x 64
    ("cap-c384", 3, 86, 84, 64, 384, 4, 4, 2, 1),           # Cout = 384: 128 x 128, three column tiles
    ("cap-cin192", 8, 64, 64, 192, 64, 4, 4, 2, 1),         # dX on 256 x 64 tiles with three column tiles; Cout = 64
    ("cap-cin128", 8, 63, 63, 128, 128, 3, 3, 2, 1),        # dX under the 128 x 128 rule, classes of different size (odd Hi, Wi)
    # ---- weight-gradient tile forms at mid size
    ("dw-128x128", 2, 28, 30, 256, 384, 4, 4, 1, 1),
    ("dw-64x64", 3, 17, 19, 192, 320, 3, 3, 1, 1),
    ("dw-64x128", 2, 30, 25, 256, 192, 6, 3, 1, 0),
]
KERNELS_RANDOM = [(1, 1), (2, 2), (3, 3), (4, 4), (6, 3), (3, 5), (1, 3), (5, 2), (2, 4)]


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def _random_cases(n, seed):
    """the seeded fill: channels, kernel, stride and pad uniform, 200 .. 8192 output pixels log-uniform, inside the size cap"""
    rng, out = random.Random(seed), []
    while len(out) < n:
        Cin, Cout = rng.choice([64, 128, 192, 256]), rng.choice([64, 128, 192, 256, 320, 384])
        kh, kw = rng.choice(KERNELS_RANDOM)
        s = rng.choice([1, 2])
        p = rng.randrange(0, min(kh, kw))
        B = rng.randrange(1, 9)
        pix = int(200 * (MAX_PIXELS / 200.0) ** rng.random()) // B
        Ho = max(1, min(pix, int(round(pix ** 0.5 * 2.0 ** rng.uniform(-1.5, 1.5)))))
        Wo = max(1, pix // Ho)
        Hi, Wi = (Ho - 1) * s + kh - 2 * p + rng.randrange(0, s), (Wo - 1) * s + kw - 2 * p + rng.randrange(0, s)
        if Hi < 1 or Wi < 1 or p >= Hi + p or B * Ho * Wo > MAX_PIXELS or B * Ho * Wo * Cout * kh * kw * Cin > MAX_MACS:
            continue
        if out_size(Hi, kh, s, p) != Ho or out_size(Wi, kw, s, p) != Wo:
            continue
        if -(-B * Ho * Wo // 128) * (Cout // 64) * kh * kw * (Cin // 64) < 1024:  # too few K steps for any persistent launch: the hand-picked
            continue                                                              # refusals above cover that side of the planner
        out.append(("random-%d" % len(out), B, Hi, Wi, Cin, Cout, kh, kw, s, p))
    return out


CASES = HAND + _random_cases(10, 20261019)
CASE = {c[0]: c for c in CASES}
# planned on the 256-row kernel by default; run under the 128-row kernel's plan as well (ops.BF16_SHAPED = False)
BOTH = ("k2s2", "k4s2p1-even", "cap-c256", "cap-c320", "cap-c384", "cap-cin192", "cap-cin128")
# weight gradient called twice, then onto a pre-filled .grad: one case per tile form
ACCUMULATE = ("dw-128x128", "k3s2p1", "dw-64x128", "dw-64x64")
# geometries the planner refuses for their channels: (tag, B, Hi, Wi, Cin, Cout, kh, kw, s, p)
REFUSED = [("cin-32", 3, 12, 20, 32, 128, 3, 3, 1, 1), ("cout-96", 3, 12, 20, 128, 96, 3, 3, 1, 1), ("cin-32-s2", 2, 17, 21, 32, 64, 4, 4, 2, 1)]

Served = collections.namedtuple("Served", "fwd dx dw")
# Which kernel serves each case (printed by `python tests/test_bf16_conv_sweep_gpu.py --plans` from the host planner; None: refused, the fp32
# kernels take the launch).  test_table_covers_the_planner asserts the planner still answers this, the GPU test that the launches got it.
EXPECT = {
    "one-row":         Served(None, None, None),  # M = 1
    "sub-wave":        Served(None, None, None),  # M = 40
    "one-128-tile":    Served(None, None, None),  # M = 128
    "k3s2p1-small":    Served(None, None, None),  # M = 60
    "tile-plus-one":   Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', None),  # M = 129
    "one-256-tile":    Served('convsk_kernel<128, 64>', None, None),  # M = 256
    "257-rows":        Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', None),  # M = 257
    "clips-per-tile":  Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', None),  # M = 756
    "k1s1":            Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', None),  # M = 8177
    "k1s2":            Served('convsk_kernel<128, 64>', None, None),  # M = 8177
    "k2s2":            Served('convbf2_kernel<128, 128>', 'convbf2_kernel<128, 128> x4', 'convbf_dw_kernel<128, 128>'),  # M = 8192
    "k3s2p1":          Served('convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x4', 'convbf_dw_kernel<128, 64>'),  # M = 2560
    "k4s2p1-odd":      Served('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x4', None),  # M = 1600
    "k4s2p1-even":     Served('convbf2_kernel<128, 128>', 'convbf2_kernel<256, 64> x4', 'convbf_dw_kernel<128, 128>'),  # M = 8192
    "k6x3":            Served('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', None),  # M = 512
    "wo-1":            Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', None),  # M = 700
    "ho-wo-1-c256":    Served('convsk_kernel<128, 64>', 'convbf2_kernel<256, 256> x1', 'convbf_dw_kernel<64, 128>'),  # M = 3640
    "ho-wo-1-c128":    Served('convsk_kernel<128, 64>', 'convbf2_kernel<256, 128> x1', None),  # M = 3640
    "pad-k-1":         Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convbf_dw_kernel<64, 128>'),  # M = 2816
    "k3x5s2":          Served('convsk_kernel<128, 128>', 'convbf2_kernel<256, 64> x4', 'convbf_dw_kernel<128, 64>'),  # M = 2907
    "two-classes":     Served('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x2', None),  # M = 2800
    "cap-c256":        Served('convbf2_kernel<128, 128>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<128, 64>'),  # M = 8177
    "cap-c320":        Served('convbf2_kernel<256, 64>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<64, 64>'),  # M = 6475
    "cap-c384":        Served('convbf2_kernel<128, 128>', 'convsk_kernel<128, 64> x4', 'convbf_dw_kernel<128, 128>'),  # M = 5418
    "cap-cin192":      Served('convsk_kernel<128, 64>', 'convbf2_kernel<256, 64> x4', 'convbf_dw_kernel<64, 128>'),  # M = 8192
    "cap-cin128":      Served('convsk_kernel<128, 128>', 'convbf2_kernel<128, 128> x4', None),  # M = 8192
    "dw-128x128":      Served('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', 'convbf_dw_kernel<128, 128>'),  # M = 1566
    "dw-64x64":        Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<64, 64>'),  # M = 969
    "dw-64x128":       Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convbf_dw_kernel<64, 128>'),  # M = 1150
    "random-0":        Served('convsk_kernel<128, 128>', None, None),  # M = 816
    "random-1":        Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<64, 128>'),  # M = 4760
    "random-2":        Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x4', 'convbf_dw_kernel<64, 128>'),  # M = 4752
    "random-3":        Served('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', None),  # M = 1496
    "random-4":        Served('convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x1', None),  # M = 1890
    "random-5":        Served('convbf2_kernel<128, 128>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<128, 64>'),  # M = 6232
    "random-6":        Served('convsk_kernel<128, 64>', 'convbf2_kernel<128, 128> x4', 'convbf_dw_kernel<64, 128>'),  # M = 5512
    "random-7":        Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x4', 'convbf_dw_kernel<64, 64>'),  # M = 2392
    "random-8":        Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convbf_dw_kernel<64, 128>'),  # M = 3360
    "random-9":        Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convbf_dw_kernel<64, 128>'),  # M = 1815
}
# the BOTH cases with ops.BF16_SHAPED = False
EXPECT_128 = {
    "k2s2":            Served('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x4', 'convbf_dw_kernel<128, 128>'),  # M = 8192
    "k4s2p1-even":     Served('convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x4', 'convbf_dw_kernel<128, 128>'),  # M = 8192
    "cap-c256":        Served('convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<128, 64>'),  # M = 8177
    "cap-c320":        Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<64, 64>'),  # M = 6475
    "cap-c384":        Served('convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x4', 'convbf_dw_kernel<128, 128>'),  # M = 5418
    "cap-cin192":      Served('convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x4', 'convbf_dw_kernel<64, 128>'),  # M = 8192
    "cap-cin128":      Served('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x4', None),  # M = 8192
}


def dims(c):
    tag, B, Hi, Wi, Cin, Cout, kh, kw, s, p = c
    Ho, Wo = out_size(Hi, kh, s, p), out_size(Wi, kw, s, p)
    return B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo


def fwd_modes(c):
    """the statistics groupings under which the forward launch exists (>= 32 rows per group)"""
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    return ([("IN", B)] if Ho * Wo >= 32 else []) + ([("BN", 1)] if B > 1 and B * Ho * Wo >= 32 else [])


def holder_modes(c):
    B, Hi, Wi = c[1:4]
    return ([("IN", B)] if Hi * Wi >= 2 else []) + ([("BN", 1)] if B > 1 else [])


def dx_fuses(ops, c, groups):
    """_conv_input_grad_bf16 accumulates the backward statistics when every parity class has >= 32 rows per group"""
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    pack = ops.dx_pack(B, Hi, Wi, Cin, Cout, kh, kw, s, p, False)
    return pack is not None and all((g.B * g.Ho * g.Wo if groups == 1 else g.Ho * g.Wo) >= 32 for g in pack[2])


def served(ops, c, dev):
    """(forward, dX, dW) kernel names from the plans ops routes the case's launches to on ``dev`` (host code; the plans are the cached ones)"""
    from speechdrivestemplates_amd import _lib
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    g = ops.fwd_geom(B, Hi, Wi, Cin, Cout, kh, kw, s, p)
    fwd = None
    for _mode, groups in fwd_modes(c):
        plan = ops._sk_plan(g, 1, B * Ho * Wo // groups, 1, dev, forward=True, dtype=_lib.BF16)
        name = None if plan is None else ops._sk_name(plan)
        assert fwd in (None, name), "the forward kernel depends on the statistics grouping"
        fwd = name
    dx = None
    pack = ops.dx_pack(B, Hi, Wi, Cin, Cout, kh, kw, s, p, False)
    if pack is not None:
        plan = ops._sk_plan(pack[0], pack[1], -1, 1, dev, dtype=_lib.BF16)
        dx = None if plan is None else "%s x%d" % (ops._sk_name(plan), pack[1])
    plan = ops._sk_dw_plan(g, dev, _lib.BF16)
    dw = None if plan is None else "convbf_dw_kernel<%d, %d>" % (plan.host[1], plan.host[2])
    return Served(fwd, dx, dw)


Data = collections.namedtuple("Data", "x w gy y dx dw")


def reference(c, dtype=torch.float64, data=None):
    """bf16-representable operands (seeded by the tag) and conv2d + autograd in ``dtype`` on them; channels-last x, gy, y, dx"""
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    if data is None:
        g = torch.Generator().manual_seed(zlib.crc32(c[0].encode()))
        x = bf16r(torch.randn(B, Hi, Wi, Cin, generator=g, dtype=torch.float64))
        w = bf16r(torch.randn(Cout, Cin, kh, kw, generator=g, dtype=torch.float64) * (2.0 / (Cin * kh * kw)) ** 0.5)
        gy = bf16r(torch.randn(B, Ho, Wo, Cout, generator=g, dtype=torch.float64))
    else:
        x, w, gy = data.x, data.w, data.gy
    xr = x.to(dtype).permute(0, 3, 1, 2).requires_grad_(True)
    wr = w.to(dtype).clone().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, s, p)
    yr.backward(gy.to(dtype).permute(0, 3, 1, 2))
    return Data(x, w, gy, yr.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), wr.grad)


def fwd_sums(y, groups):
    """(groups, Cout) sum y and sum y^2 of a channels-last output, in y's own precision"""
    yg = y.reshape(groups, -1, y.shape[-1])
    return yg.sum(1), (yg * yg).sum(1)


def _moments(y3):
    """fp32-representable mean and rstd per (group, channel) of y3 (G, R, C): what the holder hands to the kernel"""
    mean = y3.mean(1, keepdim=True).float().double()
    rstd = (1.0 / torch.sqrt(y3.var(1, unbiased=False, keepdim=True) + EPS)).float().double()
    return mean, rstd


def below(c, mode, groups):
    """The block below: its stored bf16 output, its statistics and (BN) affine parameters, with every float64 pre-activation clear of the kink"""
    B, Hi, Wi, Cin = c[1:5]
    g = torch.Generator().manual_seed(zlib.crc32((c[0] + mode).encode()))
    # mean 1.5, deviation 1: an element on the kink then has |y| ~ 1.5 and leaves it by ONE bf16 step (with mean 0 it would be tiny itself, its
    # steps with it, and off_kink_bf16 would need ten rounds of doubling)
    y3 = bf16r(1.5 + torch.randn(groups, B * Hi * Wi // groups, Cin, generator=g, dtype=torch.float64))
    gamma = beta = None
    if mode == "BN":
        gamma = (1.0 + 0.1 * torch.randn(Cin, generator=g, dtype=torch.float64)).float().double()
        beta = (0.1 * torch.randn(Cin, generator=g, dtype=torch.float64)).float().double()

    def pre(y):
        mean, rstd = _moments(y)
        u = (y - mean) * rstd
        return [u if gamma is None else u * gamma + beta]

    y3 = off_kink_bf16(y3, pre)
    mean, rstd = _moments(y3)
    assert torch.equal(y3, bf16r(y3)) and float(pre(y3)[0].abs().min()) >= KINK
    return dict(y=y3, mean=mean, rstd=rstd, gamma=gamma, beta=beta)


def bwd_sums(bl, dx, dtype=torch.float64):
    """(groups, Cin) sum g and sum g yhat with g = dx act'(yhat gamma + beta), in ``dtype``"""
    y, mean, rstd = bl["y"].to(dtype), bl["mean"].to(dtype), bl["rstd"].to(dtype)
    yh = (y - mean) * rstd
    u = yh if bl["gamma"] is None else yh * bl["gamma"].to(dtype) + bl["beta"].to(dtype)
    gg = dx.to(dtype).reshape(y.shape) * torch.where(u > 0, 1.0, SLOPE).to(dtype)
    return gg.sum(1), (gg * yh).sum(1)


def unreachable(c):
    """mask (Hi, Wi) of the input pixels no output pixel reads: their gradient is exactly +0"""
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    hit = torch.zeros(Hi + 2 * p + kh, Wi + 2 * p + kw, dtype=torch.bool)
    for i in range(kh):
        for j in range(kw):
            hit[i:i + (Ho - 1) * s + 1:s, j:j + (Wo - 1) * s + 1:s] = True
    return ~hit[p:p + Hi, p:p + Wi]


# Measured on the CPU (`python tests/test_bf16_conv_sweep_gpu.py`): rel-max-err of the same torch formula in fp32 against float64 on the very
# inputs of the named quantity, listed where 4x that error exceeds the stated tolerance (tolerance used: 4x the figure).
FP32_REF_ERR = {  # (empty: the worst case, ho-wo-1-c256, reaches 0.22 of its stated tolerance)
}


def tol_for(key, stated):
    e32 = FP32_REF_ERR.get(key)
    return stated if e32 is None else max(stated, 4.0 * e32)


@pytest.fixture()
def routed(ops):  # noqa: F811
    prev = ops.BF16_SHAPED
    yield ops
    ops.BF16_SHAPED = prev
    ops.clear_plans()


def _holder(ops, c, bl, groups):
    B, Hi, Wi, Cin = c[1:5]
    h = ops.NormBwdHolder()
    h.y = bl["y"].reshape(B, Hi, Wi, Cin).to(BF).to(DEV)
    h.mean, h.rstd = bl["mean"].reshape(-1).float().to(DEV), bl["rstd"].reshape(-1).float().to(DEV)
    if bl["gamma"] is not None:
        h.gamma, h.beta = bl["gamma"].float().to(DEV), bl["beta"].float().to(DEV)
    h.groups, h.slope = groups, SLOPE
    return h


def run_case(ops, c, d, belows, expect, label):
    tag = c[0]
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    dev = torch.device(DEV, torch.cuda.current_device())
    got = served(ops, c, dev)
    assert got == expect, "%s%s: served by %r, the table says %r" % (tag, label, got, expect)
    name = tag + label
    errs = {}
    run_forward(ops, c, d, expect, name, errs)
    run_backward(ops, c, d, belows, expect, name, errs, tag in ACCUMULATE)
    assert not ops.streamk_error_codes(), name
    print("  case %-22s fwd %-28s dX %-32s dW %-28s | %s" % (name, expect.fwd, expect.dx, expect.dw,
                                                             "  ".join("%s %.2e" % kv for kv in errs.items())))


def run_forward(ops, c, d, expect, name, errs):
    """the forward half of a case: ConvStatsFn under every grouping for which a bf16 forward launch exists"""
    tag = c[0]
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    xd = d.x.to(BF).to(DEV)
    wd = torch.nn.Parameter(ops.to_weight_layout(d.w.float()).to(DEV))

    def note(key, e):
        errs[key] = max(errs.get(key, 0.0), e)
        return e
    # ---- forward with the statistics epilogue
    live = [groups for _mode, groups in fwd_modes(c)] if expect.fwd is not None else []
    for groups in {B, 1} - set(live):
        assert not ops.conv_stats_fusable(xd, wd, s, p, groups), "%s: no bf16 forward launch exists for groups = %d" % (name, groups)
    if expect.fwd is not None:
        for mode, groups in fwd_modes(c):
            assert ops.conv_stats_fusable(xd, wd, s, p, groups)
            with torch.no_grad():
                yd, sums = ops.ConvStatsFn.apply(xd, wd, s, p, groups, None)
            torch.cuda.synchronize()
            note("y", bf16_ratio(yd, d.y, tol_for(tag + " y", TOL_BF16)))
            check_bf16("%s y (%s)" % (name, mode), yd, d.y, tol_for(tag + " y", TOL_BF16))
            sums = sums.view(groups, Cout, 2)
            for k, (q, ref) in enumerate(zip(("sum", "sumsq"), fwd_sums(d.y, groups))):
                key = "%s %s %s" % (tag, mode, q)
                note(mode + " " + q, rel_err(sums[..., k], ref))
                check("%s %s %s" % (name, mode, q), sums[..., k], ref, tol_for(key, TOL_SUMS))


def run_backward(ops, c, d, belows, expect, name, errs, accumulate, tol_for=tol_for):
    """the backward half of a case (callable alone: tests/test_reserved_conv_sweep_gpu.py runs it under a reserve, twice): dx under three
    holders, the backward sums, dW; ``accumulate``: a second dW call and a call onto a pre-filled .grad as well.  Returns every tensor a launch
    produced (dx and the statistics per holder, the first dW), for a caller that compares two runs bit for bit."""
    tag = c[0]
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    xd, gyd = d.x.to(BF).to(DEV), d.gy.to(BF).to(DEV)
    wd = torch.nn.Parameter(ops.to_weight_layout(d.w.float()).to(DEV))
    outs = []

    def note(key, e):
        errs[key] = max(errs.get(key, 0.0), e)
        return e
    # ---- input gradient: no holder, IN holder, BN holder
    dead = unreachable(c)
    for mode, groups in [(None, 0)] + holder_modes(c):
        h = None if mode is None else _holder(ops, c, belows[mode], groups)
        dxd = ops.conv_input_grad(gyd, wd, (B, Hi, Wi, Cin), s, p, h)
        torch.cuda.synchronize()
        what = "%s dx%s" % (name, "" if mode is None else " (%s holder)" % mode)
        outs += [dxd] + ([] if h is None or h.sums is None else [h.sums])
        if expect.dx is None:  # refused: the fp32 kernels took it, and no statistics were accumulated from the bf16 y
            assert dxd.dtype == torch.float32 and (h is None or h.sums is None)
            note("dx (fp32)", rel_err(dxd, d.dx))
            check(what, dxd, d.dx, tol_for(tag + " dx", TOL_BF16))
        else:
            note("dx", bf16_ratio(dxd, d.dx, tol_for(tag + " dx", TOL_BF16)))
            check_bf16(what, dxd, d.dx, tol_for(tag + " dx", TOL_BF16))
        if bool(dead.any()):
            z = dxd[:, dead.to(DEV)].float()
            assert bool((z == 0).all()) and not bool(torch.signbit(z).any()), "%s: unreachable input pixels are not exactly +0" % what
        if h is not None:
            fused = expect.dx is not None and dx_fuses(ops, c, groups)
            assert (h.sums is not None) == fused, "%s: backward statistics %s" % (what, "missing" if fused else "accumulated below 32 rows per group")
            if fused:
                bs = h.sums.view(groups, Cin, 2)
                for k, (q, ref) in enumerate(zip(("sum g", "sum g yhat"), bwd_sums(belows[mode], d.dx))):
                    note("%s %s" % (mode, q), rel_err(bs[..., k], ref))
                    check("%s %s bwd %s" % (name, mode, q), bs[..., k], ref, tol_for("%s %s bwd %s" % (tag, mode, q), TOL_BSUMS))
    # ---- weight gradient (accumulates into .grad)
    tol_dw = tol_for(tag + " dW", TOL_DW)
    ops.conv_weight_grad(xd, gyd, wd, s, p)
    torch.cuda.synchronize()
    note("dW", rel_err(wd.grad, d.dw))
    check(name + " dW", wd.grad, d.dw, tol_dw)
    outs.append(wd.grad.clone())
    if accumulate:
        assert expect.dw is not None
        ops.conv_weight_grad(xd, gyd, wd, s, p)
        check(name + " dW, second call adds", wd.grad, 2.0 * d.dw, tol_dw)
        fill = (((torch.arange(d.dw.numel(), dtype=torch.float64) * 7919) % 13 - 6.0) * 0.125 * float(d.dw.abs().max())).reshape(d.dw.shape)
        wd.grad = ops.to_weight_layout(fill.float()).to(DEV)
        assert wd.grad.stride() == wd.stride()
        ops.conv_weight_grad(xd, gyd, wd, s, p)
        torch.cuda.synchronize()
        check(name + " dW onto a pre-filled .grad", wd.grad, fill.float().double() + d.dw, tol_dw)
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_bf16_conv_sweep(routed, tag):
    """Every case under the production routing, the BOTH cases under the 128-row kernel's plan as well: y, forward sums, dx (three holders),
    backward sums, dW against float64 on the same operands; the kernel that served each launch is the table's; the error word stays clear."""
    ops, c = routed, CASE[tag]
    d = reference(c)
    belows = {mode: below(c, mode, groups) for mode, groups in holder_modes(c)}
    run_case(ops, c, d, belows, EXPECT[tag], "")
    if tag in BOTH:
        ops.BF16_SHAPED = False
        ops.clear_plans()
        assert EXPECT_128[tag] != EXPECT[tag]
        run_case(ops, c, d, belows, EXPECT_128[tag], " [128-row plan]")


@pytest.mark.gpu
@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_geometries_fall_back(ops, case):  # noqa: F811
    """Cin = 32 / Cout = 96: no bf16 plan of any kind.  conv_stats_fusable says no before any launch; conv_weight_grad and conv_input_grad on bf16
    tensors fall back to the fp32 kernels and meet the fp32 bars."""
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(case)
    assert served(ops, case, torch.device(DEV, torch.cuda.current_device())) == Served(None, None, None)
    d = reference(case)
    xd, gyd = d.x.to(BF).to(DEV), d.gy.to(BF).to(DEV)
    wd = torch.nn.Parameter(ops.to_weight_layout(d.w.float()).to(DEV))
    for groups in (B, 1):  # (host code: the answer comes from the planner, nothing is launched)
        assert not ops.conv_stats_fusable(xd, wd, s, p, groups)
    ops.conv_weight_grad(xd, gyd, wd, s, p)
    dxd = ops.conv_input_grad(gyd, wd, (B, Hi, Wi, Cin), s, p)
    torch.cuda.synchronize()
    assert wd.grad.dtype == torch.float32 and dxd.dtype == torch.float32
    check(case[0] + " dW (fp32 fall-back)", wd.grad, d.dw, TOL_DW)
    check(case[0] + " dx (fp32 fall-back)", dxd, d.dx, TOL_BF16)


# =============================================================================================================================
# host only: the table against the planner, and what the bars reject
# =============================================================================================================================
def _tile(name):
    return None if name is None else name[name.index("<"):name.index(">") + 1]


def test_table_covers_the_planner():
    """sdt_convsk_supported_t / sdt_convsk_plan_build_t / sdt_convsk_dw_supported_t through ops._sk_plan / ops._sk_dw_plan with the plan's own
    copy kept on the host: every case is routed as EXPECT says, and the table holds every kernel and tile form, every parity-class count, at
    least 8 forward / dX cases per kernel and 12 weight-gradient cases."""
    from speechdrivestemplates_amd import _lib, ops as o
    cpu = torch.device("cpu")
    prev = o.BF16_SHAPED
    try:
        o.BF16_SHAPED = True
        o.clear_plans()
        now = {c[0]: served(o, c, cpu) for c in CASES}
        o.BF16_SHAPED = False
        o.clear_plans()
        now128 = {t: served(o, CASE[t], cpu) for t in BOTH}
    finally:
        o.BF16_SHAPED = prev
        o.clear_plans()
    assert now == EXPECT, {t: (now[t], EXPECT.get(t)) for t in now if now[t] != EXPECT.get(t)}
    assert now128 == EXPECT_128, {t: (now128[t], EXPECT_128.get(t)) for t in now128 if now128[t] != EXPECT_128.get(t)}
    for c in CASES:
        B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
        assert B * Ho * Wo <= MAX_PIXELS and B * Ho * Wo * Cout * kh * kw * Cin <= MAX_MACS, c
    launches = [n for e in EXPECT.values() for n in (e.fwd, e.dx) if n is not None]
    forms = {n.split(" x")[0] for n in launches}
    # plan_shape: 256 x {256, 128, 64} and the 128 x 128 rule on the 256-row kernel; sk_tile_choice: 128 x {128, 64} on the 128-row kernel
    assert forms == {"convbf2_kernel<256, 256>", "convbf2_kernel<256, 128>", "convbf2_kernel<256, 64>", "convbf2_kernel<128, 128>",
                     "convsk_kernel<128, 128>", "convsk_kernel<128, 64>"}, forms
    for kernel in ("convbf2_kernel", "convsk_kernel"):
        n = sum(1 for e in EXPECT.values() if any(x is not None and x.startswith(kernel) for x in (e.fwd, e.dx)))
        assert n >= 8, (kernel, n)
        assert any(e.fwd is not None and e.fwd.startswith(kernel) for e in EXPECT.values()), kernel
    assert len(BOTH) >= 6
    for t in BOTH:  # the 256-row kernel by default, the 128-row kernel when it is switched off
        a, b = EXPECT[t], EXPECT_128[t]
        assert any(x is not None and x.startswith("convbf2") for x in (a.fwd, a.dx)) and all(x is None or x.startswith("convsk") for x in (b.fwd, b.dx))
    assert {int(e.dx.rsplit(" x", 1)[1]) for e in EXPECT.values() if e.dx is not None} == {1, 2, 4}
    dws = [e.dw for e in EXPECT.values() if e.dw is not None]
    assert len(dws) >= 12 and {_tile(n) for n in dws} == {"<128, 128>", "<128, 64>", "<64, 128>", "<64, 64>"}, dws
    assert {_tile(EXPECT[t].dw) for t in ACCUMULATE} == {"<128, 128>", "<128, 64>", "<64, 128>", "<64, 64>"}
    assert any(e == Served(None, None, None) for e in EXPECT.values())
    assert {c[4] for c in CASES} == {64, 128, 192, 256} and {c[5] for c in CASES} == {64, 128, 192, 256, 320, 384}
    # taps * Cin that is no multiple of the 128-wide dW column tile, on a planned weight gradient
    assert any(EXPECT[c[0]].dw is not None and (c[6] * c[7] * c[4]) % 128 == 64 for c in CASES)
    # statistics: IN with several clips per tile / rows per clip no multiple of 32; BN; below 32 rows per group (no fusion)
    assert any(EXPECT[c[0]].fwd is not None and 32 <= dims(c)[9] * dims(c)[10] < 128 and dims(c)[9] * dims(c)[10] % 32 for c in CASES)
    assert any(EXPECT[c[0]].fwd is not None and ("BN", 1) in fwd_modes(c) for c in CASES)
    assert any(EXPECT[c[0]].dx is not None and not dx_fuses(o, c, c[1]) and dx_fuses(o, c, 1) for c in CASES)
    # refused: channels, and a weight-gradient geometry that names one weight tap twice (no public entry point builds one)
    for c in REFUSED:
        assert served(o, c, cpu) == Served(None, None, None), c
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(CASE["dw-128x128"])
    good = o.fwd_geom(B, Hi, Wi, Cin, Cout, kh, kw, s, p)
    twice = _lib.ConvGeom.from_buffer_copy(good)
    lib = _lib.load()
    _lib.check(lib.sdt_convsk_set_wg_per_cu(2))
    assert lib.sdt_convsk_dw_supported_t(good, _lib.BF16) and lib.sdt_convsk_supported_t(good, 1, _lib.BF16)
    twice.wt[1] = twice.wt[0]
    assert not lib.sdt_convsk_dw_supported_t(twice, _lib.BF16)


def _trunc_bf16(t):
    return (t.float().view(torch.int32) & -65536).view(torch.float32).to(BF)


def test_bars_discriminate():
    """On the float64 references of a strided case and of an IN case with several clips per tile: the reference rounded to nearest even passes
    every bar; a dropped tap, a dropped 64-channel K step, a last row left at zero, a row credited to the next clip's statistics, a parity class
    of dx left at zero, the last 64 dW columns left at zero and truncation instead of rounding each fail theirs."""
    for tag in ("k3s2p1-small", "clips-per-tile"):
        c = CASE[tag]
        B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
        d = reference(c)
        assert bf16_ratio(d.y.float().to(BF), d.y, TOL_BF16) <= 1.0 and bf16_ratio(d.dx.float().to(BF), d.dx, TOL_BF16) <= 1.0
        assert rel_err(d.dw.float(), d.dw) < TOL_DW
        sm, sq = fwd_sums(d.y, B)
        assert rel_err(sm.float(), sm) < TOL_SUMS and rel_err(sq.float(), sq) < TOL_SUMS
        # truncation instead of rounding
        assert bf16_ratio(_trunc_bf16(d.y), d.y, TOL_BF16) > 1.0 and bf16_ratio(_trunc_bf16(d.dx), d.dx, TOL_BF16) > 1.0
        # one tap dropped; one 64-channel K step dropped
        w_tap = d.w.clone()
        w_tap[:, :, kh - 1, kw - 1] = 0
        x_k = d.x.clone()
        x_k[..., Cin - 64:] = 0
        for mut in (d._replace(w=w_tap), d._replace(x=x_k)):
            m = reference(c, data=mut)
            assert bf16_ratio(m.y.float().to(BF), d.y, TOL_BF16) > 1.0
        m = reference(c, data=d._replace(w=w_tap))
        assert bf16_ratio(m.dx.float().to(BF), d.dx, TOL_BF16) > 1.0
        gy_k = d.gy.clone()
        gy_k[..., Cout - 64:] = 0  # (the K steps of dx run over Cout)
        assert bf16_ratio(reference(c, data=d._replace(gy=gy_k)).dx.float().to(BF), d.dx, TOL_BF16) > 1.0
        gy_row = d.gy.clone()
        gy_row[-1, -1, -1 - (B * Ho * Wo - 1) % 64:] = 0  # dW: the last, partly filled 64-row K step dropped
        assert rel_err(reference(c, data=d._replace(gy=gy_row)).dw.float(), d.dw) > TOL_DW
        # the last row of the M tail left at zero
        y0 = d.y.float().to(BF).clone()
        y0[-1, -1, -1] = 0
        assert bf16_ratio(y0, d.y, TOL_BF16) > 1.0
        # the last row of a clip's plane credited to the next clip's statistics
        last = d.y[0, -1, -1]
        for k, (ref, row) in enumerate(((sm, last), (sq, last * last))):
            moved = ref.clone()
            moved[0] -= row
            moved[1] += row
            assert rel_err(moved, ref) > TOL_SUMS, (tag, k)
        # the last 64 columns of the (tap, channel) axis of dW left at zero
        dw0 = d.dw.float().clone()
        dw0[:, Cin - 64:, kh - 1, kw - 1] = 0
        assert rel_err(dw0, d.dw) > TOL_DW
        if s == 2:  # one parity class of dx left at zero
            for py in range(2):
                for px in range(2):
                    dx0 = d.dx.float().to(BF).clone()
                    dx0[:, py::2, px::2] = 0
                    assert bf16_ratio(dx0, d.dx, TOL_BF16) > 1.0
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


# =============================================================================================================================
# `python tests/test_bf16_conv_sweep_gpu.py` prints the FP32_REF_ERR entries (fp32 torch on the CPU against float64), `--plans` the EXPECT tables
# =============================================================================================================================
def _measure_fp32_ref_err():
    for c in CASES + REFUSED:
        tag, B = c[0], c[1]
        d64 = reference(c)
        d32 = reference(c, torch.float32, d64)
        rows = [(tag + " y", rel_err(d32.y, d64.y), TOL_BF16), (tag + " dx", rel_err(d32.dx, d64.dx), TOL_BF16),
                (tag + " dW", rel_err(d32.dw, d64.dw), TOL_DW)]
        for mode, groups in fwd_modes(c):
            for q, a, b in zip(("sum", "sumsq"), fwd_sums(d32.y, groups), fwd_sums(d64.y, groups)):
                rows.append(("%s %s %s" % (tag, mode, q), rel_err(a, b), TOL_SUMS))
        for mode, groups in holder_modes(c) if c in CASES else []:
            bl = below(c, mode, groups)
            for q, a, b in zip(("sum g", "sum g yhat"), bwd_sums(bl, d32.dx, torch.float32), bwd_sums(bl, d64.dx)):
                rows.append(("%s %s bwd %s" % (tag, mode, q), rel_err(a, b), TOL_BSUMS))
        print("# %-16s worst fp32-vs-float64 / stated tolerance: %.2f" % (tag, max(e / t for _k, e, t in rows)), flush=True)
        for key, e, t in rows:
            if 4.0 * e > t:
                print('    "%s": %.2e,' % (key, e), flush=True)


def _print_plans():
    from speechdrivestemplates_amd import ops as o
    cpu = torch.device("cpu")
    for name, shaped, tags in (("EXPECT", True, [c[0] for c in CASES]), ("EXPECT_128", False, list(BOTH))):
        o.BF16_SHAPED = shaped
        o.clear_plans()
        print("%s = {" % name)
        for t in tags:
            e = served(o, CASE[t], cpu)
            B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(CASE[t])
            print("    %-18s Served(%r, %r, %r),  # %r M = %d" % ('"%s":' % t, e.fwd, e.dx, e.dw, CASE[t][1:], B * Ho * Wo))
        print("}")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _print_plans() if "--plans" in sys.argv else _measure_fp32_ref_err()
