"""The Conv2d backward kernels under the persistent grids of a data-parallel run, swept against float64.

dp.GradReducer plans every backward convolution with ops.SK_RESERVED_SLOTS workgroup slots left free (csrc/convsk.hip sk_grid): the two-per-CU
kernels then run on 512 - r workgroups, the one-per-CU 8-wave kernels on (256 - r / 2) & ~7.  RESERVES: 32 = dp.RESERVED_SLOTS, 16 = what
dp.reserved_slots() answers under a 16-channel cap, 256 = the largest the library takes and what the 2-ranks-on-1-GPU tests set (with
ops.SK_RESERVED_SLOTS_FWD).  Every threshold of the planner is a function of that grid, so a reserve changes the cuts between ranges, the dW
chunking (nchunk = G / T, the Q of the ordered reduce) AND which kernel serves a layer.  The two sweeps this module is modelled on
(test_f32_conv_sweep_gpu.py, test_bf16_conv_sweep_gpu.py) run at reserve 0 only; their helpers, bars and backward halves are imported.

Modes: "split" (fp32 tensors, ops.F32_SPLIT = True: production), "mfma" (fp32 tensors, F32_SPLIT = False), "bf16" (bf16 storage, the bf16
sweep's geometries and bars).  EXPECT_RESERVED[(reserve, mode)][tag] pins what serves each selected case (`python
tests/test_reserved_conv_sweep_gpu.py --plans` prints the tables from the host planner, `--info` the grids, chunks and segments of the
hand-made cases, no argument the FP32_REF_ERR entries).

Cases per (reserve, mode): every case of the sweep whose Served differs from reserve 0, the fewest further ones (greedy, in table order) that
bring each reachable dX form and each dW form to three cases, and the hand-made NEW / NEW_BF geometries:
  seg-*      dX plans whose (range, tile) segments are exactly 1, CADENCE - 1, CADENCE, CADENCE + 1 and 2 CADENCE + 1 steps long, with a tile cut
             among three or more ranges: the 8-wave kernels at G = 240 and G = 128, the two-per-CU kernels at G = 480 and G = 256
  chunk-*    dW plans with nchunk on both sides of 8, 16 and 32 across the reserves, no multiple of the reduce's Q, idle workgroups
             (T nchunk < G) and K % nchunk != 0; Q = 1, 2, 4, 8 all met (with k3s2p1: T = 54)
  thr-*      refused at reserve 0, accepted at 16 or 32 (chunk-t15 for the three dW families, k3s2p1 / thr-sk / thr-bfsk for dX; k3s2p1 on bf16 tensors
             for the bf16 8-wave kernel, with thr-bf2-less), each with a
             neighbour a K step or a clip smaller that stays refused.

What a (reserve, mode) cannot reach (asserted in test_reserved_tables_cover_the_planner):
  * "mfma": convbf2_kernel<float, ...> serves nothing (that is the switch), convsk_kernel<128, 128> is the only dX form;
  * Q = 8 needs nchunk >= 32, i.e. K >= 256 steps of 32 rows (128 of 64): only M in (8160, 8192] under the 8192-pixel cap, with T = 15 at
    G = 480 -- chunk-t15 at reserve 32 and nowhere else.

Bars: the sweeps' own (fp32: dx 4e-6, dW 8e-6, backward sums 4e-6; bf16: those of the bf16 sweep); where 4x the error of fp32 torch on the CPU
against float64 on a check's own inputs is larger, that figure (FP32_REF_ERR below for the hand-made cases, the sweeps' tables for theirs).
Nothing a kernel produced enters a tolerance.  Results are NOT compared with the reserve-0 ones: the summation order differs by design."""
import collections
import os
import sys
import time

import pytest
import torch

import test_bf16_conv_sweep_gpu as H
import test_f32_conv_sweep_gpu as F
from test_bf16_conv_sweep_gpu import MAX_MACS, MAX_PIXELS, dims, holder_modes
from test_edge_shapes_gpu import DEV, check, ops, rel_err  # noqa: F401  (ops: the fixture)
from test_f32_conv_sweep_gpu import (CADENCE, TOL_BSUMS, TOL_DW, TOL_DX, TOL_SUMS, TOL_Y, _holder, _poison, below, reference, segment_lengths,  # noqa: F401
                                     served)

RESERVES = (16, 32, 256)
MODES = ("split", "mfma", "bf16")
SEG_NEED = {1, CADENCE - 1, CADENCE, CADENCE + 1, 2 * CADENCE + 1}

# (tag, B, Hi, Wi, Cin, Cout, kh, kw, s, p) -- fp32 tensors, both settings of F32_SPLIT
NEW = [
    ("seg-x3-g240", 5, 31, 35, 384, 320, 3, 1, 1, 0),       # split dX at reserve 32: 129 tiles of 128 x 128 on 240 ranges
    ("seg-x3-g128", 3, 30, 35, 320, 512, 2, 1, 1, 0),       # split dX at reserve 256: 65 tiles of 256 x 64 on 128 ranges
    ("seg-sk-g480", 2, 33, 33, 384, 1536, 3, 1, 1, 0),      # fp32-MFMA dX at reserve 32: 54 tiles on 480 ranges
    ("seg-sk-g256", 1, 30, 36, 384, 1280, 2, 2, 1, 0),      # ... at reserve 256: 27 tiles on 256 ranges
    ("chunk-t15", 7, 34, 39, 64, 192, 5, 1, 1, 0),          # dW: T = 15 tiles of 64 x 64, K = 256: refused at 0 / 16, nchunk = 32 (Q = 8) / 17 (Q = 4)
    ("chunk-t15-k255", 8, 34, 34, 64, 192, 5, 1, 1, 0),     # ... one K step fewer: refused at 32 as well
    ("chunk-t30", 4, 34, 39, 64, 256, 5, 3, 1, 0),          # dW: T = 30 tiles of 128 x 64, K = 139: nchunk 17 / 16 / 16 / 8, Q = 4 / 4 / 4 / 2
    ("thr-sk", 8, 54, 5, 256, 384, 4, 4, 2, 0),             # fp32-MFMA dX: S in [4 x 480, 4 x 496): refused at 0 and 16, accepted at 32
    ("thr-sk-less", 7, 54, 5, 256, 384, 4, 4, 2, 0),        # ... a clip fewer: refused everywhere but at 256
    ("thr-x3-less", 7, 31, 40, 192, 256, 3, 3, 2, 1),       # k3s2p1 with a clip fewer
]
# bf16 storage
NEW_BF = [
    ("seg-bf2-g240", 5, 31, 35, 384, 640, 3, 1, 1, 0),
    ("seg-bf2-g128", 3, 30, 35, 320, 1024, 2, 1, 1, 0),
    ("seg-bfsk-g480", 3, 31, 35, 320, 1280, 3, 1, 1, 0),
    ("seg-bfsk-g256", 1, 30, 36, 320, 1536, 2, 2, 1, 0),
    ("chunk-t15", 7, 34, 39, 64, 192, 5, 1, 1, 0),          # K = 128 steps of 64 rows
    ("chunk-t15-k127", 8, 12, 127, 64, 192, 5, 1, 1, 0),    # M = 8128: K = 127
    ("chunk-t30", 4, 34, 39, 64, 256, 5, 3, 1, 0),
    ("thr-bfsk", 2, 17, 5, 192, 320, 4, 4, 1, 0),
    ("thr-bfsk-less", 1, 17, 5, 192, 320, 4, 4, 1, 0),
    ("thr-bf2-less", 7, 31, 40, 192, 256, 3, 3, 2, 1),      # k3s2p1 with a clip fewer: stays on convsk_kernel<128, 64> at 32 (the 8-wave kernel takes k3s2p1 there)
]
# (tag, mode, reserve at which the dX plan has the segments, kernel)
SEGMENTS = (("seg-x3-g240", "split", 32, "convbf2_kernel<float"), ("seg-x3-g128", "split", 256, "convbf2_kernel<float"),
            ("seg-sk-g480", "mfma", 32, "convsk_kernel"), ("seg-sk-g256", "mfma", 256, "convsk_kernel"),
            ("seg-bf2-g240", "bf16", 32, "convbf2_kernel"), ("seg-bf2-g128", "bf16", 256, "convbf2_kernel"),
            ("seg-bfsk-g480", "bf16", 32, "convsk_kernel"), ("seg-bfsk-g256", "bf16", 256, "convsk_kernel"))
CHUNKS = ("chunk-t15", "chunk-t30", "k3s2p1")
# (mode, what, case refused at reserve 0 and accepted at `reserve`, its neighbour that stays refused there)
THRESHOLDS = (("split", "dx", "k3s2p1", 32, "thr-x3-less"), ("mfma", "dx", "thr-sk", 32, "thr-sk-less"), ("split", "dx", "thr-sk", 32, "thr-sk-less"),
              ("bf16", "dx", "thr-bfsk", 32, "thr-bfsk-less"), ("bf16", "dx", "k3s2p1", 32, "thr-bf2-less"),
              ("split", "dw", "chunk-t15", 32, "chunk-t15-k255"),
              ("mfma", "dw", "chunk-t15", 32, "chunk-t15-k255"), ("bf16", "dw", "chunk-t15", 32, "chunk-t15-k127"))
# cases re-routed by a reserve, measured on the host planner when this module was written: at least as many now
MIN_MOVED = {(32, "split"): 1, (256, "split"): 17, (256, "mfma"): 11}


def cases_of(mode):
    return (H.CASES + NEW_BF) if mode == "bf16" else (F.CASES + NEW)


def case_of(mode, tag):
    return {c[0]: c for c in cases_of(mode)}[tag]


def hand_made(mode):
    return NEW_BF if mode == "bf16" else NEW


class routing:
    """ops under (mode, reserve), restored on every exit path"""

    def __init__(self, o, mode, reserve, fwd=0):
        self.o, self.mode, self.reserve, self.fwd = o, mode, reserve, fwd

    def __enter__(self):
        o = self.o
        self.prev = (o.SK_RESERVED_SLOTS, o.SK_RESERVED_SLOTS_FWD, o.F32_SPLIT, o.STORAGE)
        o.SK_RESERVED_SLOTS, o.SK_RESERVED_SLOTS_FWD, o.F32_SPLIT = self.reserve, self.fwd, self.mode != "mfma"
        o.clear_plans()
        return o

    def __exit__(self, *exc):
        o = self.o
        o.SK_RESERVED_SLOTS, o.SK_RESERVED_SLOTS_FWD, o.F32_SPLIT = self.prev[:3]
        if o.STORAGE != self.prev[3]:
            o.set_storage(self.prev[3])
        o.clear_plans()


def serve(o, mode, c, dev):
    return H.served(o, c, dev) if mode == "bf16" else served(o, c, dev)


def _dtype(mode):
    from speechdrivestemplates_amd import _lib
    return _lib.BF16 if mode == "bf16" else _lib.F32


def dx_plan(o, mode, c, dev):
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    pack = o.dx_pack(B, Hi, Wi, Cin, Cout, kh, kw, s, p, False)
    return None if pack is None else o._sk_plan(pack[0], pack[1], -1, 1, dev, dtype=_dtype(mode))


def dw_plan(o, mode, c, dev):
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    return o._sk_dw_plan(o.fwd_geom(B, Hi, Wi, Cin, Cout, kh, kw, s, p), dev, _dtype(mode))


def grid_of(plan):
    return plan.host[3] & 0xffff, (plan.host[3] >> 16) & 0xff


def dw_chunks(plan):
    """(G, T, K, nchunk, Q) of a weight-gradient plan: nchunk = G / T and the Q of the ordered reduce as csrc/convsk.hip dw_go picks them"""
    P = plan.host
    G, T, K = P[3] & 0xffff, P[6], P[9]
    nchunk = G // T
    blocks1 = T * (P[1] * P[2] // 4 // 256)
    q = 1 if (blocks1 >= 512 or nchunk < 8) else 2 if (blocks1 >= 256 or nchunk < 16) else 4 if (blocks1 >= 128 or nchunk < 32) else 8
    return G, T, K, nchunk, q


def ranges_per_tile(plan):
    """the largest number of ranges one tile of a forward / dX plan is cut among (the tables segment_lengths reads)"""
    P = plan.host
    G, T, S = P[3] & 0xffff, P[6], P[7]
    cum = P[P[12]:P[12] + T + 1]
    n, tile = collections.Counter(), 0
    for r in range(G):
        a, b = r * S // G, (r + 1) * S // G
        while a < b:
            while cum[tile + 1] <= a:
                tile += 1
            n[tile] += 1
            a = min(b, cum[tile + 1])
    return max(n.values())


def _dx_form(mode, e):
    return None if e.dx is None else F._form(e.dx)


def _dw_form(mode, e):
    return e.dw if e.dw is not None else "fall-back"


def dx_forms(mode):
    """the dX forms an input gradient can reach under the size cap in a mode, each wanted in three cases per reserve"""
    if mode == "split":
        return ("convbf2_kernel<float, 128, 128>", "convbf2_kernel<float, 256, 64>", "convsk_kernel<128, 128>")
    if mode == "mfma":
        return ("convsk_kernel<128, 128>",)
    return ("convbf2_kernel<128, 128>", "convbf2_kernel<256, 64>", "convsk_kernel<128, 128>", "convsk_kernel<128, 64>")


def dw_forms(mode):
    k = {"split": "convx3_dw_kernel", "mfma": "convsk_dw_kernel", "bf16": "convbf_dw_kernel"}[mode]
    return tuple(k + t for t in ("<128, 128>", "<128, 64>", "<64, 128>", "<64, 64>")) + ("sdt_conv_dw_det_f32" if mode != "bf16" else "fall-back",)


def select(mode, base, now):
    """tags of a (reserve, mode) table: every sweep case routed differently from reserve 0, the fewest further ones (greedy, in table order)
    that bring every form to three cases, and the hand-made ones"""
    own = [c[0] for c in hand_made(mode)]
    tags = [t for t in now if t in own or now[t] != base[t]]
    count = collections.Counter()
    for t in tags:
        count[_dx_form(mode, now[t])] += 1
        count[_dw_form(mode, now[t])] += 1
    want = dx_forms(mode) + dw_forms(mode)
    while any(count[f] < 3 for f in want):
        gain = lambda t: sum(count[f] < 3 for f in {_dx_form(mode, now[t]), _dw_form(mode, now[t])} if f in want)  # noqa: E731
        t = max((t for t in now if t not in tags), key=gain)
        assert gain(t) > 0, (mode, {f: count[f] for f in want})
        tags.append(t)
        count[_dx_form(mode, now[t])] += 1
        count[_dw_form(mode, now[t])] += 1
    order = [c[0] for c in cases_of(mode)]
    return sorted(tags, key=order.index)


def plans_now(o, mode, reserve):
    cpu = torch.device("cpu")
    with routing(o, mode, reserve):
        return {c[0]: serve(o, mode, c, cpu) for c in cases_of(mode)}


FSV, HSV = F.Served, H.Served
# ---- BEGIN TABLES (python tests/test_reserved_conv_sweep_gpu.py --plans)
EXPECT_RESERVED = {
    (16, 'split'): {  # 0 of the sweep's 75 cases routed differently from reserve 0
        "k2s2":            FSV('convbf2_kernel<float, 128, 128>', 'convbf2_kernel<float, 128, 128> x4', 'convx3_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),
        "k3s2p1":          FSV('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=5', 'convx3_dw_kernel<128, 64>', 'fwd - | dx -'),
        "k4s2p1-even":     FSV('convbf2_kernel<float, 128, 128>', 'convbf2_kernel<float, 256, 64> x4', 'convx3_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),
        "ho-wo-1-c256":    FSV('convsk_kernel<128, 64>', 'convbf2_kernel<float, 128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd - | dx BN'),
        "pad-k-1":         FSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd - | dx IN BN'),
        "k3x5s2":          FSV('convsk_kernel<128, 128>', 'convbf2_kernel<float, 256, 64> x4', 'convx3_dw_kernel<128, 64>', 'fwd - | dx IN BN'),
        "cap-c320":        FSV('convbf2_kernel<float, 256, 64>', 'sdt_conv_taps_multi_f32 x1 k=5', 'convx3_dw_kernel<64, 64>', 'fwd IN BN | dx -'),
        "cap-cin192":      FSV('convsk_kernel<128, 64>', 'convbf2_kernel<float, 256, 64> x4', 'convx3_dw_kernel<64, 128>', 'fwd - | dx IN BN'),
        "dw-64x64":        FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=11', 'convx3_dw_kernel<64, 64>', 'fwd - | dx -'),
        "dw-64x64-b":      FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=7', 'convx3_dw_kernel<64, 64>', 'fwd IN BN | dx -'),
        "seg-x3-g240":     FSV('convsk_kernel<128, 64>', 'convbf2_kernel<float, 128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd IN BN | dx IN BN'),
        "seg-x3-g128":     FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx IN BN'),
        "seg-sk-g480":     FSV('convbf2_kernel<float, 128, 128>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),
        "seg-sk-g256":     FSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<128, 128>', 'fwd IN | dx IN'),
        "chunk-t15":       FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'),
        "chunk-t15-k255":  FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'),
        "chunk-t30":       FSV('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x1 k=7', 'convx3_dw_kernel<128, 64>', 'fwd IN BN | dx -'),
        "thr-sk":          FSV('sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x4 k=12', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),
        "thr-sk-less":     FSV('sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x4 k=12', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),
        "thr-x3-less":     FSV('sdt_conv_taps_splitk_f32 k=4', 'sdt_conv_taps_multi_f32 x4 k=6', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),
    },
    (32, 'split'): {  # 1 of the sweep's 75 cases routed differently from reserve 0
        "k2s2":            FSV('convbf2_kernel<float, 128, 128>', 'convbf2_kernel<float, 128, 128> x4', 'convx3_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),
        "k3s2p1":          FSV('convsk_kernel<128, 128>', 'convbf2_kernel<float, 256, 64> x4', 'convx3_dw_kernel<128, 64>', 'fwd - | dx IN BN'),  # reserve 0: 'convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=5', 'convx3_dw_kernel<128, 64>', 'fwd - | dx -'
        "k4s2p1-even":     FSV('convbf2_kernel<float, 128, 128>', 'convbf2_kernel<float, 256, 64> x4', 'convx3_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),
        "ho-wo-1-c256":    FSV('convsk_kernel<128, 64>', 'convbf2_kernel<float, 128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd - | dx BN'),
        "cap-c320":        FSV('convbf2_kernel<float, 256, 64>', 'sdt_conv_taps_multi_f32 x1 k=5', 'convx3_dw_kernel<64, 64>', 'fwd IN BN | dx -'),
        "cap-cin192":      FSV('convsk_kernel<128, 64>', 'convbf2_kernel<float, 256, 64> x4', 'convx3_dw_kernel<64, 128>', 'fwd - | dx IN BN'),
        "dw-64x64":        FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=11', 'convx3_dw_kernel<64, 64>', 'fwd - | dx -'),
        "seg-x3-g240":     FSV('convsk_kernel<128, 64>', 'convbf2_kernel<float, 128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd IN BN | dx IN BN'),
        "seg-x3-g128":     FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx IN BN'),
        "seg-sk-g480":     FSV('convbf2_kernel<float, 128, 128>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),
        "seg-sk-g256":     FSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<128, 128>', 'fwd IN | dx IN'),
        "chunk-t15":       FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'convx3_dw_kernel<64, 64>', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'),  # reserve 0: 'sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'
        "chunk-t15-k255":  FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'),
        "chunk-t30":       FSV('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x1 k=7', 'convx3_dw_kernel<128, 64>', 'fwd IN BN | dx -'),
        "thr-sk":          FSV('sdt_conv_taps_splitk_f32 k=16', 'convsk_kernel<128, 128> x4', 'sdt_conv_dw_det_f32', 'fwd - | dx IN BN'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x4 k=12', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "thr-sk-less":     FSV('sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x4 k=12', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),
        "thr-x3-less":     FSV('sdt_conv_taps_splitk_f32 k=4', 'sdt_conv_taps_multi_f32 x4 k=6', 'convx3_dw_kernel<128, 64>', 'fwd - | dx -'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=4', 'sdt_conv_taps_multi_f32 x4 k=6', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
    },
    (256, 'split'): {  # 17 of the sweep's 75 cases routed differently from reserve 0
        "tile-plus-one":   FSV('sdt_conv_taps_splitk_f32 k=16', 'convsk_kernel<128, 128> x1', 'sdt_conv_dw_det_f32', 'fwd - | dx IN BN'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x1 k=15', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "one-256-tile":    FSV('sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x1 k=16', 'convx3_dw_kernel<64, 128>', 'fwd - | dx -'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x1 k=16', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "257-rows":        FSV('sdt_conv_taps_splitk_f32 k=16', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd - | dx IN'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=16', 'convsk_kernel<128, 128> x1', 'sdt_conv_dw_det_f32', 'fwd - | dx IN'
        "clips-per-tile":  FSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd - | dx IN BN'),  # reserve 0: 'convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=11', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "k1s1":            FSV('convbf2_kernel<float, 256, 64>', 'convbf2_kernel<float, 128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd IN BN | dx IN BN'),  # reserve 0: 'convbf2_kernel<float, 256, 64>', 'convbf2_kernel<float, 128, 128> x1', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx IN BN'
        "k1s2":            FSV('convbf2_kernel<float, 256, 64>', 'sdt_conv_taps_splitk_f32 per class (1 of 4) k=1', 'convx3_dw_kernel<64, 128>', 'fwd IN BN | dx -'),  # reserve 0: 'convbf2_kernel<float, 256, 64>', 'sdt_conv_taps_splitk_f32 per class (1 of 4) k=1', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx -'
        "k3s2p1":          FSV('convsk_kernel<128, 128>', 'convbf2_kernel<float, 256, 64> x4', 'convx3_dw_kernel<128, 64>', 'fwd - | dx IN BN'),  # reserve 0: 'convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=5', 'convx3_dw_kernel<128, 64>', 'fwd - | dx -'
        "k4s2p1-odd":      FSV('sdt_conv_taps_splitk_f32 k=11', 'convbf2_kernel<float, 128, 128> x4', 'sdt_conv_dw_det_f32', 'fwd - | dx IN BN'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=11', 'sdt_conv_taps_multi_f32 x4 k=4', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "ho-wo-1-c128":    FSV('convsk_kernel<128, 64>', 'convbf2_kernel<float, 128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd - | dx BN'),  # reserve 0: 'convsk_kernel<128, 64>', 'convbf2_kernel<float, 128, 128> x1', 'sdt_conv_dw_det_f32', 'fwd - | dx BN'
        "two-classes":     FSV('sdt_conv_taps_splitk_f32 k=4', 'convbf2_kernel<float, 128, 128> x2', 'sdt_conv_dw_det_f32', 'fwd - | dx IN BN'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=4', 'sdt_conv_taps_multi_f32 x2 k=3', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "cap-c320":        FSV('convbf2_kernel<float, 256, 64>', 'sdt_conv_taps_multi_f32 x1 k=5', 'convx3_dw_kernel<64, 64>', 'fwd IN BN | dx -'),
        "cap-c384":        FSV('convbf2_kernel<float, 128, 128>', 'convbf2_kernel<float, 256, 64> x4', 'convx3_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),  # reserve 0: 'convbf2_kernel<float, 128, 128>', 'sdt_conv_taps_multi_f32 x4 k=7', 'convx3_dw_kernel<128, 128>', 'fwd IN BN | dx -'
        "cap-cin128":      FSV('convsk_kernel<128, 128>', 'convbf2_kernel<float, 128, 128> x4', 'convx3_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),  # reserve 0: 'convsk_kernel<128, 128>', 'convbf2_kernel<float, 128, 128> x4', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx IN BN'
        "cout64":          FSV('convsk_kernel<128, 64>', 'convbf2_kernel<float, 128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd - | dx IN BN'),  # reserve 0: 'convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd - | dx IN BN'
        "cout192":         FSV('convsk_kernel<128, 64>', 'convbf2_kernel<float, 128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd IN BN | dx IN BN'),  # reserve 0: 'convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd IN BN | dx IN BN'
        "stat-in-31":      FSV('convbf2_kernel<float, 128, 128>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<128, 128>', 'fwd BN | dx BN'),  # reserve 0: 'convbf2_kernel<float, 128, 128>', 'sdt_conv_taps_multi_f32 x1 k=1', 'convx3_dw_kernel<128, 128>', 'fwd BN | dx BN'
        "random-1":        FSV('convsk_kernel<128, 64>', 'convbf2_kernel<float, 256, 64> x4', 'convx3_dw_kernel<64, 128>', 'fwd - | dx IN BN'),  # reserve 0: 'convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x4 k=7', 'convx3_dw_kernel<64, 128>', 'fwd - | dx -'
        "random-5":        FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=4', 'convx3_dw_kernel<64, 128>', 'fwd - | dx -'),  # reserve 0: 'convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "seg-x3-g240":     FSV('convsk_kernel<128, 64>', 'convbf2_kernel<float, 128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd IN BN | dx IN BN'),
        "seg-x3-g128":     FSV('sdt_conv_taps_f32', 'convbf2_kernel<float, 256, 64> x1', 'convx3_dw_kernel<128, 128>', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx IN BN'),  # reserve 0: 'sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx IN BN'
        "seg-sk-g480":     FSV('convbf2_kernel<float, 128, 128>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),
        "seg-sk-g256":     FSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<128, 128>', 'fwd IN | dx IN'),
        "chunk-t15":       FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'convx3_dw_kernel<64, 64>', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'),  # reserve 0: 'sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'
        "chunk-t15-k255":  FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'convx3_dw_kernel<64, 64>', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'),  # reserve 0: 'sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'
        "chunk-t30":       FSV('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x1 k=7', 'convx3_dw_kernel<128, 64>', 'fwd IN BN | dx -'),
        "thr-sk":          FSV('sdt_conv_taps_splitk_f32 k=16', 'convsk_kernel<128, 128> x4', 'sdt_conv_dw_det_f32', 'fwd - | dx IN BN'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x4 k=12', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "thr-sk-less":     FSV('sdt_conv_taps_splitk_f32 k=16', 'convsk_kernel<128, 128> x4', 'sdt_conv_dw_det_f32', 'fwd - | dx IN BN'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x4 k=12', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "thr-x3-less":     FSV('sdt_conv_taps_splitk_f32 k=4', 'convbf2_kernel<float, 256, 64> x4', 'convx3_dw_kernel<128, 64>', 'fwd - | dx IN BN'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=4', 'sdt_conv_taps_multi_f32 x4 k=6', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
    },
    (16, 'mfma'): {  # 0 of the sweep's 75 cases routed differently from reserve 0
        "k2s2":            FSV('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=1', 'convsk_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),
        "k3s2p1":          FSV('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=5', 'convsk_dw_kernel<128, 64>', 'fwd - | dx -'),
        "ho-wo-1-c256":    FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=1', 'convsk_dw_kernel<64, 128>', 'fwd - | dx BN'),
        "pad-k-1":         FSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<64, 128>', 'fwd - | dx IN BN'),
        "k3x5s2":          FSV('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=4', 'convsk_dw_kernel<128, 64>', 'fwd - | dx -'),
        "cap-c320":        FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=5', 'convsk_dw_kernel<64, 64>', 'fwd IN BN | dx -'),
        "dw-64x64":        FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=11', 'convsk_dw_kernel<64, 64>', 'fwd - | dx -'),
        "dw-64x64-b":      FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=7', 'convsk_dw_kernel<64, 64>', 'fwd IN BN | dx -'),
        "seg-x3-g240":     FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=1', 'convsk_dw_kernel<64, 128>', 'fwd IN BN | dx IN BN'),
        "seg-x3-g128":     FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx IN BN'),
        "seg-sk-g480":     FSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),
        "seg-sk-g256":     FSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<128, 128>', 'fwd IN | dx IN'),
        "chunk-t15":       FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'),
        "chunk-t15-k255":  FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'),
        "chunk-t30":       FSV('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x1 k=7', 'convsk_dw_kernel<128, 64>', 'fwd IN BN | dx -'),
        "thr-sk":          FSV('sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x4 k=12', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),
        "thr-sk-less":     FSV('sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x4 k=12', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),
        "thr-x3-less":     FSV('sdt_conv_taps_splitk_f32 k=4', 'sdt_conv_taps_multi_f32 x4 k=6', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),
    },
    (32, 'mfma'): {  # 0 of the sweep's 75 cases routed differently from reserve 0
        "k2s2":            FSV('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=1', 'convsk_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),
        "k3s2p1":          FSV('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=5', 'convsk_dw_kernel<128, 64>', 'fwd - | dx -'),
        "ho-wo-1-c256":    FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=1', 'convsk_dw_kernel<64, 128>', 'fwd - | dx BN'),
        "pad-k-1":         FSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<64, 128>', 'fwd - | dx IN BN'),
        "cap-c320":        FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=5', 'convsk_dw_kernel<64, 64>', 'fwd IN BN | dx -'),
        "dw-64x64":        FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=11', 'convsk_dw_kernel<64, 64>', 'fwd - | dx -'),
        "seg-x3-g240":     FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=1', 'convsk_dw_kernel<64, 128>', 'fwd IN BN | dx IN BN'),
        "seg-x3-g128":     FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx IN BN'),
        "seg-sk-g480":     FSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),
        "seg-sk-g256":     FSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<128, 128>', 'fwd IN | dx IN'),
        "chunk-t15":       FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'convsk_dw_kernel<64, 64>', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'),  # reserve 0: 'sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'
        "chunk-t15-k255":  FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'),
        "chunk-t30":       FSV('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x1 k=7', 'convsk_dw_kernel<128, 64>', 'fwd IN BN | dx -'),
        "thr-sk":          FSV('sdt_conv_taps_splitk_f32 k=16', 'convsk_kernel<128, 128> x4', 'sdt_conv_dw_det_f32', 'fwd - | dx IN BN'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x4 k=12', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "thr-sk-less":     FSV('sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x4 k=12', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),
        "thr-x3-less":     FSV('sdt_conv_taps_splitk_f32 k=4', 'sdt_conv_taps_multi_f32 x4 k=6', 'convsk_dw_kernel<128, 64>', 'fwd - | dx -'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=4', 'sdt_conv_taps_multi_f32 x4 k=6', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
    },
    (256, 'mfma'): {  # 11 of the sweep's 75 cases routed differently from reserve 0
        "tile-plus-one":   FSV('sdt_conv_taps_splitk_f32 k=16', 'convsk_kernel<128, 128> x1', 'sdt_conv_dw_det_f32', 'fwd - | dx IN BN'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x1 k=15', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "one-256-tile":    FSV('sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x1 k=16', 'convsk_dw_kernel<64, 128>', 'fwd - | dx -'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x1 k=16', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "257-rows":        FSV('sdt_conv_taps_splitk_f32 k=16', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<64, 128>', 'fwd - | dx IN'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=16', 'convsk_kernel<128, 128> x1', 'sdt_conv_dw_det_f32', 'fwd - | dx IN'
        "clips-per-tile":  FSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<64, 128>', 'fwd - | dx IN BN'),  # reserve 0: 'convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=11', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "k1s1":            FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=1', 'convsk_dw_kernel<64, 128>', 'fwd IN BN | dx IN BN'),  # reserve 0: 'convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx IN BN'
        "k1s2":            FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_splitk_f32 per class (1 of 4) k=1', 'convsk_dw_kernel<64, 128>', 'fwd IN BN | dx -'),  # reserve 0: 'convsk_kernel<128, 64>', 'sdt_conv_taps_splitk_f32 per class (1 of 4) k=1', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx -'
        "k3s2p1":          FSV('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=5', 'convsk_dw_kernel<128, 64>', 'fwd - | dx -'),
        "ho-wo-1-c128":    FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=1', 'convsk_dw_kernel<64, 128>', 'fwd - | dx BN'),  # reserve 0: 'convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd - | dx BN'
        "cap-c320":        FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=5', 'convsk_dw_kernel<64, 64>', 'fwd IN BN | dx -'),
        "cap-cin128":      FSV('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=1', 'convsk_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),  # reserve 0: 'convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x4 k=1', 'sdt_conv_dw_det_f32', 'fwd IN BN | dx IN BN'
        "cout64":          FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=1', 'convsk_dw_kernel<64, 128>', 'fwd - | dx IN BN'),  # reserve 0: 'convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd - | dx IN BN'
        "stat-in-31":      FSV('sdt_conv_taps_f32', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<128, 128>', 'fwd BN:sdt_conv_taps_stats_f32 | dx BN'),  # reserve 0: 'sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=1', 'convsk_dw_kernel<128, 128>', 'fwd BN:sdt_conv_taps_stats_f32 | dx BN'
        "random-5":        FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=4', 'convsk_dw_kernel<64, 128>', 'fwd - | dx -'),  # reserve 0: 'convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "seg-x3-g240":     FSV('convsk_kernel<128, 64>', 'sdt_conv_taps_multi_f32 x1 k=1', 'convsk_dw_kernel<64, 128>', 'fwd IN BN | dx IN BN'),
        "seg-x3-g128":     FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=1', 'convsk_dw_kernel<128, 128>', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx IN BN'),  # reserve 0: 'sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=1', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx IN BN'
        "seg-sk-g480":     FSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<128, 128>', 'fwd IN BN | dx IN BN'),
        "seg-sk-g256":     FSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<128, 128>', 'fwd IN | dx IN'),
        "chunk-t15":       FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'convsk_dw_kernel<64, 64>', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'),  # reserve 0: 'sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'
        "chunk-t15-k255":  FSV('sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'convsk_dw_kernel<64, 64>', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'),  # reserve 0: 'sdt_conv_taps_f32', 'sdt_conv_taps_multi_f32 x1 k=4', 'sdt_conv_dw_det_f32', 'fwd IN:sdt_conv_taps_stats_f32 BN:sdt_conv_taps_stats_f32 | dx -'
        "chunk-t30":       FSV('convsk_kernel<128, 128>', 'sdt_conv_taps_multi_f32 x1 k=7', 'convsk_dw_kernel<128, 64>', 'fwd IN BN | dx -'),
        "thr-sk":          FSV('sdt_conv_taps_splitk_f32 k=16', 'convsk_kernel<128, 128> x4', 'sdt_conv_dw_det_f32', 'fwd - | dx IN BN'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x4 k=12', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "thr-sk-less":     FSV('sdt_conv_taps_splitk_f32 k=16', 'convsk_kernel<128, 128> x4', 'sdt_conv_dw_det_f32', 'fwd - | dx IN BN'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=16', 'sdt_conv_taps_multi_f32 x4 k=12', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
        "thr-x3-less":     FSV('sdt_conv_taps_splitk_f32 k=4', 'sdt_conv_taps_multi_f32 x4 k=6', 'convsk_dw_kernel<128, 64>', 'fwd - | dx -'),  # reserve 0: 'sdt_conv_taps_splitk_f32 k=4', 'sdt_conv_taps_multi_f32 x4 k=6', 'sdt_conv_dw_det_f32', 'fwd - | dx -'
    },
    (16, 'bf16'): {  # 0 of the sweep's 39 cases routed differently from reserve 0
        "tile-plus-one":   HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', None),
        "k2s2":            HSV('convbf2_kernel<128, 128>', 'convbf2_kernel<128, 128> x4', 'convbf_dw_kernel<128, 128>'),
        "k4s2p1-even":     HSV('convbf2_kernel<128, 128>', 'convbf2_kernel<256, 64> x4', 'convbf_dw_kernel<128, 128>'),
        "pad-k-1":         HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convbf_dw_kernel<64, 128>'),
        "k3x5s2":          HSV('convsk_kernel<128, 128>', 'convbf2_kernel<256, 64> x4', 'convbf_dw_kernel<128, 64>'),
        "cap-c320":        HSV('convbf2_kernel<256, 64>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<64, 64>'),
        "cap-cin192":      HSV('convsk_kernel<128, 64>', 'convbf2_kernel<256, 64> x4', 'convbf_dw_kernel<64, 128>'),
        "cap-cin128":      HSV('convsk_kernel<128, 128>', 'convbf2_kernel<128, 128> x4', None),
        "dw-64x64":        HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<64, 64>'),
        "dw-64x128":       HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convbf_dw_kernel<64, 128>'),
        "random-7":        HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x4', 'convbf_dw_kernel<64, 64>'),
        "seg-bf2-g240":    HSV('convbf2_kernel<128, 128>', 'convbf2_kernel<128, 128> x1', 'convbf_dw_kernel<128, 128>'),
        "seg-bf2-g128":    HSV('convbf2_kernel<128, 128>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<128, 128>'),
        "seg-bfsk-g480":   HSV('convbf2_kernel<128, 128>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<128, 64>'),
        "seg-bfsk-g256":   HSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<128, 128>'),
        "chunk-t15":       HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x1', None),
        "chunk-t15-k127":  HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x1', None),
        "chunk-t30":       HSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<128, 64>'),
        "thr-bfsk":        HSV(None, None, None),
        "thr-bfsk-less":   HSV(None, None, None),
        "thr-bf2-less":    HSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x4', None),
    },
    (32, 'bf16'): {  # 2 of the sweep's 39 cases routed differently from reserve 0
        "one-256-tile":    HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', None),  # reserve 0: 'convsk_kernel<128, 64>', None, None
        "k2s2":            HSV('convbf2_kernel<128, 128>', 'convbf2_kernel<128, 128> x4', 'convbf_dw_kernel<128, 128>'),
        "k3s2p1":          HSV('convsk_kernel<128, 128>', 'convbf2_kernel<256, 64> x4', 'convbf_dw_kernel<128, 64>'),  # reserve 0: 'convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x4', 'convbf_dw_kernel<128, 64>'
        "k4s2p1-even":     HSV('convbf2_kernel<128, 128>', 'convbf2_kernel<256, 64> x4', 'convbf_dw_kernel<128, 128>'),
        "pad-k-1":         HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convbf_dw_kernel<64, 128>'),
        "cap-c320":        HSV('convbf2_kernel<256, 64>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<64, 64>'),
        "cap-cin192":      HSV('convsk_kernel<128, 64>', 'convbf2_kernel<256, 64> x4', 'convbf_dw_kernel<64, 128>'),
        "cap-cin128":      HSV('convsk_kernel<128, 128>', 'convbf2_kernel<128, 128> x4', None),
        "dw-64x64":        HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<64, 64>'),
        "dw-64x128":       HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convbf_dw_kernel<64, 128>'),
        "seg-bf2-g240":    HSV('convbf2_kernel<128, 128>', 'convbf2_kernel<128, 128> x1', 'convbf_dw_kernel<128, 128>'),
        "seg-bf2-g128":    HSV('convbf2_kernel<128, 128>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<128, 128>'),
        "seg-bfsk-g480":   HSV('convbf2_kernel<128, 128>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<128, 64>'),
        "seg-bfsk-g256":   HSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<128, 128>'),
        "chunk-t15":       HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<64, 64>'),  # reserve 0: 'convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x1', None
        "chunk-t15-k127":  HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x1', None),
        "chunk-t30":       HSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<128, 64>'),
        "thr-bfsk":        HSV(None, 'convsk_kernel<128, 64> x1', None),  # reserve 0: None, None, None
        "thr-bfsk-less":   HSV(None, None, None),
        "thr-bf2-less":    HSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x4', 'convbf_dw_kernel<128, 64>'),  # reserve 0: 'convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x4', None
    },
    (256, 'bf16'): {  # 14 of the sweep's 39 cases routed differently from reserve 0
        "one-128-tile":    HSV(None, 'convsk_kernel<128, 128> x1', None),  # reserve 0: None, None, None
        "one-256-tile":    HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convbf_dw_kernel<64, 128>'),  # reserve 0: 'convsk_kernel<128, 64>', None, None
        "257-rows":        HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convbf_dw_kernel<64, 128>'),  # reserve 0: 'convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', None
        "clips-per-tile":  HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convbf_dw_kernel<64, 128>'),  # reserve 0: 'convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', None
        "k1s1":            HSV('convsk_kernel<128, 64>', 'convbf2_kernel<128, 128> x1', 'convbf_dw_kernel<64, 128>'),  # reserve 0: 'convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', None
        "k1s2":            HSV('convsk_kernel<128, 64>', None, 'convbf_dw_kernel<64, 128>'),  # reserve 0: 'convsk_kernel<128, 64>', None, None
        "k3s2p1":          HSV('convsk_kernel<128, 128>', 'convbf2_kernel<256, 64> x4', 'convbf_dw_kernel<128, 64>'),  # reserve 0: 'convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x4', 'convbf_dw_kernel<128, 64>'
        "k4s2p1-odd":      HSV('convsk_kernel<128, 128>', 'convbf2_kernel<128, 128> x4', None),  # reserve 0: 'convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x4', None
        "ho-wo-1-c128":    HSV('convsk_kernel<128, 64>', 'convbf2_kernel<256, 128> x1', 'convbf_dw_kernel<64, 128>'),  # reserve 0: 'convsk_kernel<128, 64>', 'convbf2_kernel<256, 128> x1', None
        "two-classes":     HSV('convsk_kernel<128, 128>', 'convbf2_kernel<128, 128> x2', None),  # reserve 0: 'convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x2', None
        "cap-c384":        HSV('convbf2_kernel<128, 128>', 'convbf2_kernel<256, 64> x4', 'convbf_dw_kernel<128, 128>'),  # reserve 0: 'convbf2_kernel<128, 128>', 'convsk_kernel<128, 64> x4', 'convbf_dw_kernel<128, 128>'
        "cap-cin128":      HSV('convsk_kernel<128, 128>', 'convbf2_kernel<128, 128> x4', 'convbf_dw_kernel<128, 128>'),  # reserve 0: 'convsk_kernel<128, 128>', 'convbf2_kernel<128, 128> x4', None
        "random-2":        HSV('convsk_kernel<128, 64>', 'convbf2_kernel<256, 64> x4', 'convbf_dw_kernel<64, 128>'),  # reserve 0: 'convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x4', 'convbf_dw_kernel<64, 128>'
        "random-7":        HSV('convsk_kernel<128, 64>', 'convbf2_kernel<256, 64> x4', 'convbf_dw_kernel<64, 64>'),  # reserve 0: 'convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x4', 'convbf_dw_kernel<64, 64>'
        "seg-bf2-g240":    HSV('convbf2_kernel<128, 128>', 'convbf2_kernel<128, 128> x1', 'convbf_dw_kernel<128, 128>'),
        "seg-bf2-g128":    HSV('convbf2_kernel<128, 128>', 'convbf2_kernel<256, 64> x1', 'convbf_dw_kernel<128, 128>'),  # reserve 0: 'convbf2_kernel<128, 128>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<128, 128>'
        "seg-bfsk-g480":   HSV('convbf2_kernel<128, 128>', 'convbf2_kernel<256, 64> x1', 'convbf_dw_kernel<128, 64>'),  # reserve 0: 'convbf2_kernel<128, 128>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<128, 64>'
        "seg-bfsk-g256":   HSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<128, 128>'),
        "chunk-t15":       HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<64, 64>'),  # reserve 0: 'convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x1', None
        "chunk-t15-k127":  HSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<64, 64>'),  # reserve 0: 'convsk_kernel<128, 64>', 'convsk_kernel<128, 64> x1', None
        "chunk-t30":       HSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x1', 'convbf_dw_kernel<128, 64>'),
        "thr-bfsk":        HSV(None, 'convsk_kernel<128, 64> x1', None),  # reserve 0: None, None, None
        "thr-bfsk-less":   HSV(None, None, None),
        "thr-bf2-less":    HSV('convsk_kernel<128, 128>', 'convbf2_kernel<256, 64> x4', 'convbf_dw_kernel<128, 64>'),  # reserve 0: 'convsk_kernel<128, 128>', 'convsk_kernel<128, 64> x4', None
    },
}
# ---- END TABLES

# Measured on the CPU (`python tests/test_reserved_conv_sweep_gpu.py`): fp32 torch (one thread) against float64 on the inputs of the named check of
# a hand-made case, listed where 4x the error exceeds 0.8 of the stated bar, as in test_f32_conv_sweep_gpu.py (the sweeps' cases keep their tables)
FP32_REF_ERR = {
    "seg-x3-g240 dx": 1.35e-06, "seg-x3-g128 dx": 1.44e-06, "seg-sk-g480 dx": 2.39e-06, "seg-sk-g480 IN bwd sum g": 9.03e-07,
    "seg-sk-g480 BN bwd sum g": 1.06e-06, "seg-sk-g256 dx": 1.42e-06, "seg-sk-g256 IN bwd sum g": 9.11e-07, "chunk-t15 dx": 1.48e-06,
    "chunk-t15-k255 dx": 1.20e-06, "thr-sk dx": 8.87e-07, "thr-sk-less dx": 1.18e-06, "thr-x3-less dx": 8.49e-07, "thr-x3-less dW": 2.21e-06,
    "bf16 seg-bfsk-g480 dx": 2.13e-06,  # (bf16 storage: keys carry the mode; long plain fp32 sums on the CPU, 3840 terms per output)
}


def tol_for(key, stated):
    e32 = FP32_REF_ERR.get(key)
    return F.tol_for(key, stated) if e32 is None else max(stated, 4.0 * e32)


def tol_for_bf16(key, stated):
    e32 = FP32_REF_ERR.get("bf16 " + key)
    return H.tol_for(key, stated) if e32 is None else max(stated, 4.0 * e32)


@pytest.fixture()
def reserved(ops):  # noqa: F811
    """restores SK_RESERVED_SLOTS, SK_RESERVED_SLOTS_FWD, F32_SPLIT and the storage mode and drops the plans, on every exit path; the library's
    process-wide knob must be back at 0 after every test"""
    from speechdrivestemplates_amd import _lib
    prev = (ops.SK_RESERVED_SLOTS, ops.SK_RESERVED_SLOTS_FWD, ops.F32_SPLIT, ops.BF16_SHAPED, ops.STORAGE)
    try:
        yield ops
        assert not ops.streamk_error_codes()
        assert _lib.load().sdt_convsk_grid() == 512, "a plan builder left the process-wide reserve set"
    finally:
        ops.SK_RESERVED_SLOTS, ops.SK_RESERVED_SLOTS_FWD, ops.F32_SPLIT, ops.BF16_SHAPED = prev[:4]
        if ops.STORAGE != prev[4]:
            ops.set_storage(prev[4])
        ops.clear_plans()


_REF = collections.OrderedDict()  # (mode is bf16, tag) -> (Data, belows): the float64 reference of a case, shared by its reserves


def ref_of(mode, c):
    key = (mode == "bf16", c[0])
    if key not in _REF:
        mod = H if mode == "bf16" else F
        _REF[key] = (mod.reference(c), {m: mod.below(c, m, g) for m, g in holder_modes(c)})
        while len(_REF) > 2:  # (tag-major parametrization: a case's reserves follow one another; each mode's test computes its references anew)
            _REF.popitem(last=False)
    return _REF[key]


def _params(mode):
    return [(t, r) for t in [c[0] for c in cases_of(mode)] for r in RESERVES if t in EXPECT_RESERVED.get((r, mode), {})]


def accumulates(mode, reserve, tag):
    """the first case of each dW form in the table: a second call adds on top, and a call onto a pre-filled .grad"""
    first = {}
    for t, e in EXPECT_RESERVED[(reserve, mode)].items():
        first.setdefault(_dw_form(mode, e), t)
    first.pop("fall-back", None)  # (bf16 tensors the planner refuses go to sdt_conv_dw_det_f32, which the fp32 modes accumulate into)
    return tag in first.values()


def _line(mode, reserve, c, expect, errs, o, dev, t0):
    dxp, dwp = dx_plan(o, mode, c, dev), dw_plan(o, mode, c, dev)
    seg = "-" if dxp is None else "G %d segs %s" % (grid_of(dxp)[0], ",".join(map(str, sorted(segment_lengths(dxp)))))
    chk = "-" if dwp is None else "G %d nchunk %d Q %d" % (dw_chunks(dwp)[0], dw_chunks(dwp)[3], dw_chunks(dwp)[4])
    print("  case %-16s %-5s r=%-3d dX %-40s [%s] dW %-28s [%s] %s | %s | %.2f s" % (
        c[0], mode, reserve, expect.dx, seg, expect.dw, chk, getattr(expect, "stats", "").split("| ")[-1],
        "  ".join("%s %.2e" % kv for kv in errs.items()), time.time() - t0))


def _run_fp32(ops, mode, tag, reserve):
    t0 = time.time()
    c = case_of(mode, tag)
    d, belows = ref_of(mode, c)
    expect = EXPECT_RESERVED[(reserve, mode)][tag]
    dev = torch.device(DEV, torch.cuda.current_device())
    ops.F32_SPLIT, ops.SK_RESERVED_SLOTS = mode == "split", reserve
    ops.clear_plans()
    got = served(ops, c, dev)
    assert got == expect, "%s [%s, reserve %d]: served by %r, the table says %r" % (tag, mode, reserve, got, expect)
    errs = {}
    F.run_backward(ops, c, d, belows, expect, "%s [%s r%d]" % (tag, mode, reserve), errs, accumulates(mode, reserve, tag), tol=tol_for)
    assert not ops.streamk_error_codes(), tag
    _line(mode, reserve, c, expect, errs, ops, dev, t0)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,reserve", _params("split"))
def test_reserved_sweep_split(reserved, tag, reserve):
    """ops.conv_input_grad (no holder, IN, BN; twice each from NaN-poisoned allocations, bit-identical; unreachable pixels +0; fused statistics
    exactly where the table says) and ops.conv_weight_grad (twice; for one case per form a second call and a pre-filled .grad) against float64
    with ops.SK_RESERVED_SLOTS = reserve, production arithmetic; the serving kernels are the table's."""
    _run_fp32(reserved, "split", tag, reserve)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,reserve", _params("mfma"))
def test_reserved_sweep_mfma(reserved, tag, reserve):
    """... with ops.F32_SPLIT = False: the fp32-MFMA kernels"""
    _run_fp32(reserved, "mfma", tag, reserve)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,reserve", _params("bf16"))
def test_reserved_sweep_bf16(reserved, tag, reserve):
    """... on bf16 tensors, the bf16 sweep's bars; the whole backward half twice, every tensor bit-identical"""
    ops, mode, t0 = reserved, "bf16", time.time()
    c = case_of(mode, tag)
    d, belows = ref_of(mode, c)
    expect = EXPECT_RESERVED[(reserve, mode)][tag]
    dev = torch.device(DEV, torch.cuda.current_device())
    ops.SK_RESERVED_SLOTS = reserve
    ops.clear_plans()
    got = H.served(ops, c, dev)
    assert got == expect, "%s [bf16, reserve %d]: served by %r, the table says %r" % (tag, reserve, got, expect)
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    errs, name, runs = {}, "%s [bf16 r%d]" % (tag, reserve), []
    for rep in range(2):
        _poison((Cin, kh * kw, Cout), (B, Hi, Wi, Cin))
        runs.append(H.run_backward(ops, c, d, belows, expect, name, errs, rep == 0 and accumulates(mode, reserve, tag), tol_for=tol_for_bf16))
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs)), "%s: the second run differs from the first" % name
    assert not ops.streamk_error_codes(), tag
    _line(mode, reserve, c, expect, errs, ops, dev, t0)


# one case per forward kernel form: (tag, mode)
FORWARD = (("k2s2", "split"), ("k1s1", "split"), ("k3s2p1", "split"), ("dw-64x64", "split"), ("cout96", "split"), ("k2s2", "mfma"), ("k2s2", "bf16"),
           ("cap-c320", "bf16"), ("k3s2p1", "bf16"), ("dw-64x64", "bf16"))


@pytest.mark.gpu
@pytest.mark.parametrize("tag,mode", FORWARD, ids=["%s-%s" % f for f in FORWARD])
def test_forward_under_a_reserve(reserved, tag, mode):
    """ops.SK_RESERVED_SLOTS_FWD = 256, the shared-GPU setting: conv_forward without and with a bias and ConvStatsFn under IN / BN, the checks of
    the sweeps' forward halves; the plan runs on the reserved grid."""
    ops = reserved
    c = case_of(mode, tag)
    d, _belows = ref_of(mode, c)
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    dev = torch.device(DEV, torch.cuda.current_device())
    ops.F32_SPLIT, ops.SK_RESERVED_SLOTS_FWD, ops.SK_RESERVED_SLOTS = mode != "mfma", 256, 0
    ops.clear_plans()
    plan = ops._sk_plan(ops.fwd_geom(B, Hi, Wi, Cin, Cout, kh, kw, s, p), 1, B * Ho * Wo, 1, dev, forward=True, dtype=_dtype(mode))
    if plan is not None:
        G, wpc = grid_of(plan)
        assert G == (256 if wpc == 2 else 128), (tag, G, wpc)
    errs = {}
    if mode == "bf16":
        H.run_forward(ops, c, d, H.served(ops, c, dev), "%s [bf16 fwd r256]" % tag, errs)
    else:
        F.run_forward(ops, c, d, "%s [%s fwd r256]" % (tag, mode), errs, tol=tol_for)
    print("  fwd  %-16s %-5s %s | %s" % (tag, mode, None if plan is None else ops._sk_name(plan), "  ".join("%s %.2e" % kv for kv in errs.items())))


# power-of-two scaling at reserve 32: one case per backward kernel family, (tag, mode)
SCALED = (("k3s2p1", "split"), ("cout192", "split"), ("dw-128x128", "mfma"), ("cout96", "split"))
# what serves them at reserve 32 (asserted against the planner on the host, against `served` on the device)
SCALED_SERVED = {
    ('k3s2p1', 'split'): FSV('convsk_kernel<128, 128>', 'convbf2_kernel<float, 256, 64> x4', 'convx3_dw_kernel<128, 64>', 'fwd - | dx IN BN'),
    ('cout192', 'split'): FSV('convsk_kernel<128, 64>', 'convsk_kernel<128, 128> x1', 'convx3_dw_kernel<64, 128>', 'fwd IN BN | dx IN BN'),
    ('dw-128x128', 'mfma'): FSV('convsk_kernel<128, 128>', 'convsk_kernel<128, 128> x1', 'convsk_dw_kernel<128, 128>', 'fwd - | dx IN BN'),
    ('cout96', 'split'): FSV('sdt_conv_taps_splitk_f32 k=5', 'sdt_conv_taps_multi_f32 x1 k=5', 'sdt_conv_dw_det_f32', 'fwd - | dx -'),
}
SCALED_FAMILIES = {"dx convbf2_kernel", "dx convsk_kernel", "dx sdt_conv_taps_multi_f32", "dW convx3_dw_kernel", "dW convsk_dw_kernel", "dW sdt_conv_dw_det_f32"}


@pytest.mark.gpu
@pytest.mark.parametrize("tag,mode", SCALED, ids=["%s-%s" % f for f in SCALED])
def test_power_of_two_scaling_at_reserve_32(reserved, tag, mode):
    """x 2^a, w 2^b, gy 2^c: dx and dW are bit-identical to the unscaled run times 2^(b+c), 2^(a+c) (derived, as in the fp32 sweep: splits,
    products, fp32 accumulation and the flush are exact under a power-of-two scale; operands have |value| in [2^-10, 2^4])."""
    import zlib
    ops, c = reserved, case_of(mode, tag)
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    ops.F32_SPLIT, ops.SK_RESERVED_SLOTS = mode == "split", 32
    ops.clear_plans()
    assert served(ops, c, torch.device(DEV, torch.cuda.current_device())) == SCALED_SERVED[(tag, mode)]
    g = torch.Generator().manual_seed(zlib.crc32((tag + " scaled").encode()))
    x = F._clamped(torch.randn(B, Hi, Wi, Cin, generator=g, dtype=torch.float64))
    w = F._clamped(torch.randn(Cout, Cin, kh, kw, generator=g, dtype=torch.float64) * (2.0 / (Cin * kh * kw)) ** 0.5)
    gy = F._clamped(torch.randn(B, Ho, Wo, Cout, generator=g, dtype=torch.float64))

    def run(a, b, cc):
        xd, gyd = (x * 2.0 ** a).float().to(DEV), (gy * 2.0 ** cc).float().to(DEV)
        wd = F._param(ops, w * 2.0 ** b)
        assert torch.equal(xd.double().cpu(), x * 2.0 ** a) and torch.equal(wd.detach().double().cpu(), w * 2.0 ** b)  # the scaled operands are exact
        assert torch.equal(gyd.double().cpu(), gy * 2.0 ** cc)
        dx = ops.conv_input_grad(gyd, wd, (B, Hi, Wi, Cin), s, p)
        ops.conv_weight_grad(xd, gyd, wd, s, p)
        torch.cuda.synchronize()
        return dx, wd.grad

    dx0, dw0 = run(0, 0, 0)
    for a, b, cc in F.SCALES:
        dx1, dw1 = run(a, b, cc)
        for q, t0, t1, e in (("dx", dx0, dx1, b + cc), ("dW", dw0, dw1, a + cc)):
            assert torch.equal(t1, t0 * 2.0 ** e), "%s %s under (a, b, c) = %r: %d of %d elements are not the unscaled ones times 2^%d" % (
                tag, q, (a, b, cc), int((t1 != t0 * 2.0 ** e).sum()), t0.numel(), e)


# =============================================================================================================================
# host only
# =============================================================================================================================
def test_reserved_tables_cover_the_planner():
    """The pinned tables are what the planner says now; SK_RESERVED_SLOTS does not touch forward plans; every plan header carries the reserved
    grid; every reachable dX form and every dW form (fall-back included) serves three cases per (reserve, mode); at least as many cases are
    re-routed as when the tables were written (an ops that ignores the reserve fails here); the hand-made cases have the segments, chunks and
    thresholds they were made for, read off the plans' own tables."""
    from speechdrivestemplates_amd import ops as o
    cpu = torch.device("cpu")
    qs = {m: set() for m in MODES}
    for mode in MODES:
        base = plans_now(o, mode, 0)
        if mode == "split":
            assert {t: base[t] for t in F.EXPECT} == F.EXPECT
        for c in hand_made(mode):
            B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
            assert B * Ho * Wo <= MAX_PIXELS and B * Ho * Wo * Cout * kh * kw * Cin <= MAX_MACS and kh * kw <= 20, c
        for reserve in RESERVES:
            now, table = plans_now(o, mode, reserve), EXPECT_RESERVED[(reserve, mode)]
            assert list(table) == select(mode, base, now), (mode, reserve, set(table) ^ set(select(mode, base, now)))
            assert table == {t: now[t] for t in table}, {t: (now[t], table[t]) for t in table if now[t] != table[t]}
            assert all(now[t].fwd == base[t].fwd for t in now), (mode, reserve)
            if mode != "bf16":  # (the forward part of the statistics field as well)
                assert all(now[t].stats.split(" | ")[0] == base[t].stats.split(" | ")[0] for t in now)
            moved = sum(now[c[0]] != base[c[0]] for c in (H.CASES if mode == "bf16" else F.CASES))
            assert moved >= MIN_MOVED.get((reserve, mode), 0), (mode, reserve, moved)
            count = collections.Counter()
            for e in table.values():
                count[_dx_form(mode, e)] += 1
                count[_dw_form(mode, e)] += 1
            for form in dx_forms(mode) + dw_forms(mode):
                assert count[form] >= 3, (mode, reserve, form, count)
            if mode == "mfma":
                assert not any("convbf2" in (e.dx or "") or "convx3" in (e.dw or "") for e in now.values())
            with routing(o, mode, reserve):
                for t in table:
                    for plan in (dx_plan(o, mode, case_of(mode, t), cpu), dw_plan(o, mode, case_of(mode, t), cpu)):
                        if plan is not None:
                            G, wpc = grid_of(plan)
                            assert G == (512 - reserve if wpc == 2 else (256 - reserve // 2) & ~7), (mode, reserve, t, G, wpc)
    # ---- segments: 1, CADENCE - 1, CADENCE, CADENCE + 1, 2 CADENCE + 1 steps and a tile cut among three ranges or more
    for tag, mode, reserve, kernel in SEGMENTS:
        with routing(o, mode, reserve):
            plan = dx_plan(o, mode, case_of(mode, tag), cpu)
            name = o._sk_name(plan)
            assert name.startswith(kernel) and ("float" in name) == ("float" in kernel), (tag, name)
            assert grid_of(plan)[0] == {("convbf2_kernel", 32): 240, ("convbf2_kernel", 256): 128, ("convsk_kernel", 32): 480,
                                        ("convsk_kernel", 256): 256}[(kernel.split("<")[0], reserve)]
            assert SEG_NEED <= set(segment_lengths(plan)) and ranges_per_tile(plan) >= 3, (tag, sorted(segment_lengths(plan)), ranges_per_tile(plan))
    # ---- chunks, per dW kernel family
    for mode in MODES:
        seen = {}
        for tag in CHUNKS:
            for reserve in (0,) + RESERVES:
                with routing(o, mode, reserve):
                    plan = dw_plan(o, mode, case_of(mode, tag), cpu)
                    if plan is not None:
                        seen[(tag, reserve)] = dw_chunks(plan)
        rows = list(seen.values())
        assert {q for _G, _T, _K, _n, q in rows} == {1, 2, 4, 8}, (mode, seen)
        assert any(n % q for _G, _T, _K, n, q in rows) and any(T * n < G for G, T, _K, n, _q in rows) and any(K % n for _G, _T, K, n, _q in rows)
        assert all(any(n % q and T * n < G and K % n for G, T, K, n, q in (v for (t, _r), v in seen.items() if t == tag)) for tag in CHUNKS), (mode, seen)
        for edge in (8, 16, 32):  # the same layer on both sides of the edge, hence reduced with different Q
            assert any({seen[k][3] >= edge for k in seen if k[0] == tag} == {True, False} for tag in CHUNKS), (mode, edge, seen)
        assert any(len({seen[k][4] for k in seen if k[0] == tag}) > 1 for tag in CHUNKS)
    # ---- thresholds: refused at reserve 0, accepted under the reserve; the neighbour stays refused
    for mode, what, tag, reserve, less in THRESHOLDS:
        get = dx_plan if what == "dx" else dw_plan
        kern = lambda plan: None if plan is None else (o._sk_name(plan).split(",")[0] if what == "dx" else "dw")  # noqa: E731
        with routing(o, mode, reserve):
            on = kern(get(o, mode, case_of(mode, tag), cpu))
            off = kern(get(o, mode, case_of(mode, less), cpu))
        with routing(o, mode, 0):
            on0 = kern(get(o, mode, case_of(mode, tag), cpu))
            off0 = kern(get(o, mode, case_of(mode, less), cpu))
        assert on is not None and on != on0 and off != on, (mode, what, tag, on0, on, off)
        # "stays refused": the neighbour is served under the reserve by what serves it at reserve 0 (no plan at all for a weight gradient)
        assert off == off0 and (what == "dx" or off is None), (mode, what, less, off0, off)
    # ---- one case per backward kernel family under power-of-two scaling; one per forward form under the forward reserve
    fam = set()
    for t, mode in SCALED:
        e = plans_now(o, mode, 32)[t]
        assert e == SCALED_SERVED[(t, mode)], (t, mode, e)
        fam |= {"dx " + F._form(e.dx).split("<")[0], "dW " + e.dw.split("<")[0]}
    assert fam >= SCALED_FAMILIES, fam
    fwd = set()
    for t, mode in FORWARD:
        with routing(o, mode, 0, fwd=256):
            fwd.add((mode == "bf16", serve(o, mode, case_of(mode, t), cpu).fwd.split(" k=")[0]))
    assert fwd >= {(False, "convbf2_kernel<float, 128, 128>"), (False, "convbf2_kernel<float, 256, 64>"), (False, "convsk_kernel<128, 128>"),
                   (False, "convsk_kernel<128, 64>"), (True, "convbf2_kernel<128, 128>"), (True, "convbf2_kernel<256, 64>"),
                   (True, "convsk_kernel<128, 128>"), (True, "convsk_kernel<128, 64>")}, fwd
    assert any(not f.startswith("conv") for _b, f in fwd)  # ... and the 64 x 64 fall-back, which no reserve touches


def _cpu_rows(mode, c):
    """(key, fp32-torch-vs-float64 error, stated bar) of every backward check of a hand-made case"""
    if mode != "bf16":
        return [r for r in F.cpu_fp32_rows(c) if " y" not in r[0] and " sum" not in r[0].replace("bwd sum", "")]
    d64 = H.reference(c)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        d32 = H.reference(c, torch.float32, d64)
        rows = [("bf16 %s dx" % c[0], rel_err(d32.dx, d64.dx), H.TOL_BF16), ("bf16 %s dW" % c[0], rel_err(d32.dw, d64.dw), H.TOL_DW)]
        for m, g in holder_modes(c):
            bl = H.below(c, m, g)
            for q, a, b in zip(("sum g", "sum g yhat"), H.bwd_sums(bl, d32.dx, torch.float32), H.bwd_sums(bl, d64.dx)):
                rows.append(("bf16 %s %s bwd %s" % (c[0], m, q), rel_err(a, b), H.TOL_BSUMS))
        return rows
    finally:
        torch.set_num_threads(threads)


def test_cpu_fp32_stays_below_a_quarter_of_the_bars():
    """fp32 torch on the CPU against float64 on the inputs of every backward check of the hand-made cases: below a quarter of the stated bar, or
    listed in FP32_REF_ERR with the figure measured here (the sweeps' own cases are held to this by the sweeps)."""
    seen = set()
    for mode in ("split", "bf16"):
        for c in hand_made(mode):
            for key, e, stated in _cpu_rows(mode, c):
                seen.add(key)
                if key in FP32_REF_ERR:
                    assert FP32_REF_ERR[key] / 1.5 <= e <= 1.5 * FP32_REF_ERR[key] and 4.0 * FP32_REF_ERR[key] > 0.8 * stated, (key, e, FP32_REF_ERR[key])
                else:
                    assert 4.0 * e <= stated, "%s: fp32 torch on the CPU errs by %.2e, more than a quarter of %.1e: list it in FP32_REF_ERR" % (key, e, stated)
    assert set(FP32_REF_ERR) <= seen, set(FP32_REF_ERR) - seen


def test_reserved_bars_discriminate():
    """On the float64 reference of every hand-made case, with one thing removed, each removal a STAND-IN of the same size for what a plan could
    lose, not read off every plan: (dW) the contribution of one K step of 32 rows (64 for bf16) to a 64 x 64 block of dW, the last step of chunk
    0 of the reserve-256 plan; (dW reduce) chunk nchunk / Q - 1 of that plan, the last one of part 0 of the reduce (whether or not that part is an
    uneven one: the chunks are of equal size up to a step); (dX) one K step -- tap (0, 0) on 32 (64) channels of dY -- for the first 128 input
    pixels on 64 channels, no larger than a one-step segment of any tile form.  Each removal exceeds the bar of its check, by orders of magnitude."""
    from speechdrivestemplates_amd import ops as o
    cpu = torch.device("cpu")
    for mode in ("split", "bf16"):
        step, chan = (64, 64) if mode == "bf16" else (32, 32)
        tol_dw = H.TOL_DW if mode == "bf16" else TOL_DW
        for c in hand_made(mode):
            B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
            d = (H if mode == "bf16" else F).reference(c)
            M = B * Ho * Wo
            x2, gy2 = d.x, d.gy.reshape(M, Cout)
            # dW: rows [m0, m0 + step) of dY contribute gy^T x-window to every tile; remove them from the first 64 x 64 block of dW
            with routing(o, mode, 256):
                plan = dw_plan(o, mode, c, cpu)
            cuts = [(0, step, "the first K step")]  # (no stream-K dW plan at any reserve: the dX threshold cases; the fall-back has no chunks)
            if plan is not None:
                G, T, K, nchunk, q = dw_chunks(plan)
                last = K // nchunk - 1  # the last step of chunk 0
                c1 = max(nchunk // q, 1)  # part 0 of the reduce sums the chunks [0, c1)
                cuts = [(last * step, (last + 1) * step, "the last K step of chunk 0"),
                        ((c1 - 1) * K // nchunk * step, c1 * K // nchunk * step, "the last chunk of part 0 of the reduce")]
            for lo, hi, what in cuts:
                gy_cut = gy2.clone()
                gy_cut[lo:min(hi, M), :64] = 0
                part = F._dw_of(c, x2, gy_cut.reshape(d.gy.shape))
                e = rel_err(part, d.dw)
                assert e > (tol_for_bf16 if mode == "bf16" else tol_for)("%s dW" % c[0], tol_dw), (mode, c[0], what, e)
            # dX: one K step of the first tile: 32 (64) channels of dY for the rows of one 128-row tile of dx
            # (a step is one tap on 32 (64) channels of dY; the tile: the first 128 input pixels on the first 64 channels -- no larger than any form's)
            w_cut = d.w.clone()
            w_cut[:chan, :, 0, 0] = 0
            dx_cut = d.dx.clone()
            dx_cut.view(-1, Cin)[:128, :64] = F._dx_of(c, d.gy, w_cut).reshape(-1, Cin)[:128, :64]
            e = rel_err(dx_cut, d.dx)
            bar = tol_for("%s dx" % c[0], TOL_DX) if mode != "bf16" else 2.0 ** -8 + tol_for_bf16("%s dx" % c[0], H.TOL_BF16)  # (bf16: the most check_bf16 allows anywhere)
            assert e > bar, (mode, c[0], "one K step of one dX tile", e)


# =============================================================================================================================
# `python tests/test_reserved_conv_sweep_gpu.py --plans` prints the tables, `--info` the hand-made cases' plans, no argument FP32_REF_ERR
# =============================================================================================================================
def _print_plans():
    from speechdrivestemplates_amd import ops as o
    print("EXPECT_RESERVED = {")
    for mode in MODES:
        base = plans_now(o, mode, 0)
        for reserve in RESERVES:
            now = plans_now(o, mode, reserve)
            moved = sum(now[c[0]] != base[c[0]] for c in (H.CASES if mode == "bf16" else F.CASES))
            print("    (%d, %r): {  # %d of the sweep's %d cases routed differently from reserve 0" % (reserve, mode, moved, len(base) - len(hand_made(mode))))
            for t in select(mode, base, now):
                e = now[t]
                print("        %-18s %s(%s),%s" % ('"%s":' % t, "HSV" if mode == "bf16" else "FSV", ", ".join(repr(v) for v in e),
                                                   "  # reserve 0: %s" % ", ".join(repr(v) for v in base[t]) if e != base[t] else ""))
            print("    },")
    print("}")


def _print_info():
    from speechdrivestemplates_amd import ops as o
    cpu = torch.device("cpu")
    for mode in MODES:
        for c in hand_made(mode) + [case_of(mode, "k3s2p1")]:
            for reserve in (0,) + RESERVES:
                with routing(o, mode, reserve):
                    dxp, dwp = dx_plan(o, mode, c, cpu), dw_plan(o, mode, c, cpu)
                    dxs = "-" if dxp is None else "%s G %d T %d S %d cut<=%d segs %s" % (o._sk_name(dxp), grid_of(dxp)[0], dxp.host[6], dxp.host[7],
                                                                                         ranges_per_tile(dxp), sorted(segment_lengths(dxp)))
                    dws = "-" if dwp is None else "%dx%d G %d T %d K %d nchunk %d Q %d" % ((dwp.host[1], dwp.host[2]) + dw_chunks(dwp))
                    print("%-5s %-16s r=%-3d dX %s | dW %s" % (mode, c[0], reserve, dxs, dws))


def _measure():
    for mode in ("split", "bf16"):
        for c in hand_made(mode):
            rows = _cpu_rows(mode, c)
            print("# %-5s %-16s worst fp32-vs-float64 / stated bar: %.2f" % (mode, c[0], max(e / t for _k, e, t in rows)), flush=True)
            for key, e, t in rows:
                if 4.0 * e > 0.8 * t:
                    print('    "%s": %.2e,' % (key, e), flush=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _print_plans() if "--plans" in sys.argv else _print_info() if "--info" in sys.argv else _measure()
