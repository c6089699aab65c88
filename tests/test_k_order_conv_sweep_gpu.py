"""The chunk-major K order of the 8-wave Conv2d kernels (csrc/convbf.hip convbf2_kernel, bf16 storage and split-fp32; ops.SK_K_ORDER = 1,
sdt_convsk_set_k_order(1)) swept against float64 and against the default tap-major order.

Under order 1 a tile walks all live taps of one 128-byte channel chunk before the next chunk, where the default walks all chunks of one tap.
Two places of the loader change with it: commit() derives (chunk, remaining-tap mask) of a range's first step inside a tile from the segment start
f.a as (f.a / nlive, f.a % nlive), and load_advance() strips one live-tap bit per step and moves to the next chunk when the mask runs out.
nlive = popcount(ti_mask) is the tile's live-tap count, nkc = tile steps / nlive its 128-byte chunks (bf16: Cin / 64, fp32: Cin / 32; for an
input gradient "Cin" is the layer's Cout).

The helpers, tables, operands and bars are the two sweeps' own (test_bf16_conv_sweep_gpu.py, test_f32_conv_sweep_gpu.py); a new node id has no
recorded margin, so the stated tolerances and FP32_REF_ERR entries of those files apply as they are.  The order of summation does not enter them.

LIST is the case list: (dtype, tag, reserve).  reserve 32 sets ops.SK_RESERVED_SLOTS (what input-gradient plans read) and
ops.SK_RESERVED_SLOTS_FWD (what forward plans read): G = 240 ranges instead of 256, every range boundary moves.
test_cases_reach_the_chunk_major_cursor_edges (host only) decides that the list reaches the cursor edges (a) to (i) named there;
`python tests/test_k_order_conv_sweep_gpu.py` prints which launch of which case reaches which (`--all`: of every candidate of both sweeps)."""
import collections
import contextlib
import os
import sys
import zlib

import pytest
import torch

import test_bf16_conv_sweep_gpu as H
import test_f32_conv_sweep_gpu as F
from test_bf16_conv_sweep_gpu import MAX_MACS, MAX_PIXELS, dims
from test_edge_shapes_bf16_gpu import BF, bf16r
from test_edge_shapes_gpu import DEV, ops  # noqa: F401  (ops: the fixture)
from test_geometry import _read_plan
from test_ops_gpu import _presplit_case
from test_ops_gpu import test_presplit_weights_are_bit_identical_to_the_in_kernel_split as _presplit_test

RESERVE = 32
# (tag, B, Hi, Wi, Cin, Cout, kh, kw, s, p): geometries for the conditions the sweeps' own cases leave unreached (see the coverage test)
NEW = [
    # 3 x 3 pad 1 on 8-row images: image-row-major tiles, the top / bottom kernel row culled in the first / last image row's tiles (6 of 9 taps
    # live) with rot = 6 at the bottom; M = 8192 rows = 64 x 2 tiles of 128 x 128 (T = 128 = G / 2, the fewest the planner takes), S = 4.1 G
    ("short-rows", 16, 8, 64, 128, 256, 3, 3, 1, 1),
    # a (6, 3) kernel as large as the input (Ho = Wo = 1), 456 clips: the input gradient is ONE class of 8208 rows = 65 row tiles of 128 (the last
    # of 16 rows) x 3 column tiles over 2.6 MB (bf16) / 5.3 MB of weights: the n-tile-major tile order (>= 64 row tiles, > 2 MB, several n-tiles)
    ("nt-major", 456, 6, 3, 384, 192, 6, 3, 1, 0),
]
NEW_F32 = [
    ("short-rows", 16, 8, 64, 64, 256, 3, 3, 1, 1),         # (Cin = 64: two 32-channel chunks per tap, S = 4.1 G as above)
    ("nt-major", 456, 6, 3, 384, 192, 6, 3, 1, 0),
]


def case_of(dtype, tag):
    own = {c[0]: c for c in (NEW if dtype == "bf16" else NEW_F32)}
    return own[tag] if tag in own else (H if dtype == "bf16" else F).CASE[tag]


LIST = [
    ("bf16", "k2s2", 0), ("bf16", "k4s2p1-even", 0), ("bf16", "k3x5s2", 0), ("bf16", "cap-c320", 0), ("bf16", "ho-wo-1-c256", 0),
    ("bf16", "ho-wo-1-c128", 0), ("bf16", "short-rows", 0), ("bf16", "nt-major", 0), ("bf16", "k3s2p1", RESERVE),
    ("f32", "k2s2", 0), ("f32", "k4s2p1-even", 0), ("f32", "k3x5s2", 0), ("f32", "cap-c320", 0), ("f32", "cin32-k3", 0),
    ("f32", "cout384", 0), ("f32", "short-rows", 0), ("f32", "nt-major", 0), ("f32", "k3s2p1", RESERVE),
]
IDS = ["%s-%s%s" % (d, t, "-reserve%d" % r if r else "") for d, t, r in LIST]


@contextlib.contextmanager
def k_order(o, order, reserve=0):
    """ops under (SK_K_ORDER, reserve) with fresh plans; everything restored on every exit path, and the LIBRARY left tap-major: the setting is
    process-wide and is only pushed by the next launch that finds ops._K_ORDER_SET stale"""
    from speechdrivestemplates_amd import _lib
    prev = (o.SK_K_ORDER, o.SK_RESERVED_SLOTS, o.SK_RESERVED_SLOTS_FWD)
    o.SK_K_ORDER, o.SK_RESERVED_SLOTS, o.SK_RESERVED_SLOTS_FWD = order, reserve, reserve
    o.clear_plans()
    try:
        yield o
    finally:
        o.SK_K_ORDER, o.SK_RESERVED_SLOTS, o.SK_RESERVED_SLOTS_FWD = prev
        o.clear_plans()
        _lib.check(_lib.load().sdt_convsk_set_k_order(0))
        o._K_ORDER_SET[0] = 0


# =============================================================================================================================
# host: the plans of a case's launches and where their (range, tile) segments put the chunk-major cursor
# =============================================================================================================================
def _lib_dtype(dtype):
    from speechdrivestemplates_amd import _lib
    return _lib.BF16 if dtype == "bf16" else _lib.F32


def launches(o, dtype, c, dev):
    """[(role, kernel name, plan)] of the forward and the input-gradient launch of a case, as ops routes them now (plans kept on the host as
    plan.host; the statistics grouping changes a plan's group column only, never its tiles or ranges)"""
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    dt, out = _lib_dtype(dtype), []
    plan = o._sk_plan(o.fwd_geom(B, Hi, Wi, Cin, Cout, kh, kw, s, p), 1, 0 if dtype == "f32" else Ho * Wo, 1, dev, forward=True, dtype=dt)
    if plan is not None:
        out.append(("fwd", o._sk_name(plan), plan))
    pack = o.dx_pack(B, Hi, Wi, Cin, Cout, kh, kw, s, p, False)
    plan = None if pack is None else o._sk_plan(pack[0], pack[1], -1, 1, dev, dtype=dt)
    if plan is not None:
        out.append(("dx", "%s x%d" % (o._sk_name(plan), pack[1]), plan))
    return out


Seg = collections.namedtuple("Seg", "r tile cls a b n nlive nkc ntaps rot")


def segments(plan):
    """Every (range, tile) segment [a, b) of a plan, in steps of the tile, with the tile's facts -- recomputed from the plan's own tables as the
    kernel does: range r runs the steps [r S / G, (r + 1) S / G), a tile's steps are tilecum[t] .. tilecum[t + 1], its live-tap mask and rotation
    are tileinfo[class.mt_begin + mt]"""
    hdr, _rowinfo, tileinfo, tilecum, range_tile, classes = _read_plan(plan.host)
    G, S, T, nnb = hdr["G"], hdr["S"], hdr["T"], hdr["nnb"]
    assert tilecum[0] == 0 and tilecum[T] == S
    out = []
    for r in range(G):
        pos, end = r * S // G, (r + 1) * S // G
        tile = int(range_tile[r])
        assert tilecum[tile] <= pos < tilecum[tile + 1]
        while pos < end:
            if hdr["ntmajor"]:
                cls, mt = 0, tile % int(classes[0][7])
            else:
                cls = max(k for k in range(hdr["ncls"]) if int(classes[k][6]) <= tile)
                mt = (tile - int(classes[cls][6])) // nnb
            ntaps, nkc, mt_begin = int(classes[cls][4]), int(classes[cls][5]), int(classes[cls][9])
            mask, rot = int(tileinfo[mt_begin + mt][0]) & 0xffffffff, int(tileinfo[mt_begin + mt][1])
            nlive, n = bin(mask).count("1"), int(tilecum[tile + 1] - tilecum[tile])
            assert nlive >= 1 and n == nlive * nkc, (tile, nlive, nkc, n)
            a, b = pos - int(tilecum[tile]), min(end, int(tilecum[tile + 1])) - int(tilecum[tile])
            out.append(Seg(r, tile, cls, a, b, n, nlive, nkc, ntaps, rot))
            pos, tile = int(tilecum[tile]) + b, tile + 1
    return hdr, out


CONDITIONS = collections.OrderedDict([
    ("a", "a range starts inside a tile at a step that is no multiple of the live-tap count"),
    ("b", "... where the two orders begin at a different (tap, chunk)"),
    ("c", "a range ends before the tile's end at a step that is no multiple of the live-tap count"),
    ("d", "such a start in a tile with culled taps and a non-zero rotation"),
    ("e", "a tile with one live tap"),
    ("f", "a launch with one chunk per tap (nkc == 1)"),
    ("g", "an input-gradient range that crosses into a parity class with another tap count"),
    ("h", "an n-tile-major plan"),
    ("i256", "256-row tiles"),
    ("i128", "the 128 x 128 tile"),
    ("mix", "a launch where nlive > 1 and nkc > 1: the two orders sum in a different order"),
])


def reached(role, hdr, segs):
    """the conditions of CONDITIONS a launch reaches"""
    got = set()
    for i, s in enumerate(segs):
        if s.a > 0 and s.a % s.nlive:
            got.add("a")
        if s.a > 0 and (s.a // s.nlive != s.a % s.nkc or s.a % s.nlive != s.a // s.nkc):
            got.add("b")
            if s.nlive < s.ntaps and s.rot:
                got.add("d")
        if s.b < s.n and s.b % s.nlive:
            got.add("c")
        if s.nlive == 1:
            got.add("e")
        if s.nkc == 1:
            got.add("f")
        if s.nlive > 1 and s.nkc > 1:
            got.add("mix")
        if role == "dx" and i and segs[i - 1].r == s.r and segs[i - 1].cls != s.cls and segs[i - 1].ntaps != s.ntaps:
            got.add("g")
    if hdr["ntmajor"]:
        got.add("h")
    got.add("i256" if hdr["bm"] == 256 else "i128")
    if hdr["bm"] == 128:
        assert hdr["bn"] == 128
    return got


def coverage(o, entries):
    """{(dtype, tag, reserve, role): (kernel name, conditions)} of the convbf2_kernel launches of ``entries``, planned on the host"""
    cpu, out = torch.device("cpu"), collections.OrderedDict()
    for dtype, tag, reserve in entries:
        with k_order(o, 0, reserve):
            for role, name, plan in launches(o, dtype, case_of(dtype, tag), cpu):
                if name.startswith("convbf2_kernel"):
                    out[(dtype, tag, reserve, role)] = (name, reached(role, *segments(plan)))
    return out


def test_cases_reach_the_chunk_major_cursor_edges():
    """Plans of every (dtype, case, reserve) of LIST built on the host (as test_table_covers_the_planner does): each case has a launch on
    convbf2_kernel, in the form the sweeps' tables pin at reserve 0, and over the list -- for bf16 and for fp32 each -- the (range, tile) segments
    reach (a) to (i) of CONDITIONS.

    What no accepted plan reaches, and the planner rule that excludes it, asserted here: (i) on fp32 tensors the only 256-row form is 256 x 64
    (csrc/convsk.hip plan_shape: the split form takes 128 x 128, or 256 x 64 where Cout is no multiple of 128) -- no split-fp32 launch of any
    case of test_f32_conv_sweep_gpu.py has another form; 256 x 256 and 256 x 128 are bf16 forms, and the bf16 list holds all three.
    (h) needs a geometry of its own for either dtype: n-tile-major wants more than 2 MB of weights, several n-tiles AND 64 row tiles of a
    one-class launch (plan_build), which no case of the two sweeps has on convbf2_kernel (asserted)."""
    from speechdrivestemplates_amd import ops as o
    assert o.SK_K_ORDER == 0 and o.F32_SPLIT and o.BF16_SHAPED
    cov = coverage(o, LIST)
    assert o.SK_K_ORDER == 0 and o._K_ORDER_SET[0] == 0
    for dtype, tag, reserve in LIST:
        mine = {k[3]: v for k, v in cov.items() if k[:3] == (dtype, tag, reserve)}
        assert mine, "%s %s reserve %d: no launch on convbf2_kernel" % (dtype, tag, reserve)
        c = case_of(dtype, tag)
        B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
        assert B * Ho * Wo <= MAX_PIXELS and B * Ho * Wo * Cout * kh * kw * Cin <= MAX_MACS and kh * kw * max(Cin, Cout) * 8 < 2 ** 24, c
        table = (H if dtype == "bf16" else F).EXPECT
        if reserve == 0 and tag in table:  # the sweeps' tables pin the same kernel and tile form
            for role, (name, _got) in mine.items():
                assert name == getattr(table[tag], role), (dtype, tag, role, name)
    for dtype in ("bf16", "f32"):
        assert sum(1 for d, _t, r in LIST if d == dtype and r == 0) <= 8 and sum(1 for d, _t, r in LIST if d == dtype and r) == 1
        union = set().union(*[got for k, (_n, got) in cov.items() if k[0] == dtype])
        assert union >= set(CONDITIONS), "%s: the list does not reach %s" % (dtype, sorted(set(CONDITIONS) - union))
        # (a) - (d) together with a launch whose orders differ: the edge is met where the order matters
        assert any({"a", "b", "c", "mix"} <= got for k, (_n, got) in cov.items() if k[0] == dtype), dtype
        assert any({"d", "mix"} <= got for k, (_n, got) in cov.items() if k[0] == dtype), dtype
    forms = {name.split(" x")[0] for name, _got in cov.values()}
    assert forms == {"convbf2_kernel<256, 256>", "convbf2_kernel<256, 128>", "convbf2_kernel<256, 64>", "convbf2_kernel<128, 128>",
                     "convbf2_kernel<float, 256, 64>", "convbf2_kernel<float, 128, 128>"}, forms
    # launches that must not move: each dtype has a case whose dx stays on the 4-wave kernel
    for dtype in ("bf16", "f32"):
        assert any(_convsk_dx(o, d, t, r) for d, t, r in LIST if d == dtype), dtype
    # (h): no convbf2 launch of the two sweeps' own cases is n-tile-major;  (i): the split form's tiles are these two
    every = coverage(o, [("f32", c[0], 0) for c in F.CASES])
    assert every and {n.split(" x")[0] for n, _g in every.values()} == {"convbf2_kernel<float, 256, 64>", "convbf2_kernel<float, 128, 128>"}
    every.update(coverage(o, [("bf16", c[0], 0) for c in H.CASES]))
    assert not any("h" in got for _n, got in every.values())


def _convsk_dx(o, dtype, tag, reserve):
    with k_order(o, 0, reserve):
        return any(role == "dx" and name.startswith("convsk_kernel<128") for role, name, _p in launches(o, dtype, case_of(dtype, tag), torch.device("cpu")))


def test_the_setter_checks_its_argument():
    """sdt_convsk_set_k_order takes 0 and 1; anything else is an argument error that names the setter and the two values, and leaves it usable"""
    from speechdrivestemplates_amd import _lib
    lib = _lib.load()
    try:
        for bad in (2, -1):
            assert lib.sdt_convsk_set_k_order(bad) != 0
            msg = lib.sdt_last_error()
            msg = msg.decode() if isinstance(msg, bytes) else msg
            assert "sdt_convsk_set_k_order" in msg and "tap-major" in msg and "chunk-major" in msg, msg
        assert lib.sdt_convsk_set_k_order(1) == 0
    finally:
        assert lib.sdt_convsk_set_k_order(0) == 0


# =============================================================================================================================
# GPU
# =============================================================================================================================
def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _launch(o, dtype, c, d, fwd, dx=True):
    """(y or None, dx) of a case through the public entry points: ops.conv_forward (fp32) / ConvStatsFn, y only (bf16); ops.conv_input_grad
    without a holder"""
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    el = BF if dtype == "bf16" else torch.float32
    xd, gyd = d.x.to(el).to(DEV), d.gy.to(el).to(DEV)
    wd = torch.nn.Parameter(o.to_weight_layout(d.w.float()).to(DEV))
    y = None
    if fwd and dtype == "f32":
        y = o.conv_forward(xd, wd, None, s, p)
    elif fwd:
        groups = H.fwd_modes(c)[0][1]
        assert o.conv_stats_fusable(xd, wd, s, p, groups)
        with torch.no_grad():
            y = o.ConvStatsFn.apply(xd, wd, s, p, groups, None)[0]
    dxd = o.conv_input_grad(gyd, wd, (B, Hi, Wi, Cin), s, p) if dx else None
    torch.cuda.synchronize()
    return y, dxd


def _routes(o, dtype, c):
    dev = torch.device(DEV, torch.cuda.current_device())
    return {role: name for role, name, _plan in launches(o, dtype, c, dev)}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tag,reserve", LIST, ids=IDS)
def test_integer_operands_are_exact_under_both_k_orders(ops, dtype, tag, reserve):  # noqa: F811
    """x, gy uniform in -4 .. 4, w in -2 .. 2: every product and partial sum is an integer below taps x channels x 8 < 2^24, so fp32 accumulation
    is exact in ANY order, the stream-K fix-up of partial tiles included, and float64 conv2d / autograd is exact too.  y and dx under both K
    orders equal the reference bit for bit (bf16: its one rounding to nearest even), hence each other; unreachable input pixels are exactly +0;
    the error word stays clear.  A dropped, repeated or mismatched (tap, chunk) step is an integer error: no tolerance to hide behind."""
    c = case_of(dtype, tag)
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    assert kh * kw * max(Cin, Cout) * 8 < 2 ** 24
    g = torch.Generator().manual_seed(zlib.crc32((tag + " integers").encode()))
    data = H.Data(_ints((B, Hi, Wi, Cin), -4, 4, g), _ints((Cout, Cin, kh, kw), -2, 2, g), _ints((B, Ho, Wo, Cout), -4, 4, g), None, None, None)
    d = H.reference(c, data=data)
    assert float(d.y.abs().max()) < 2 ** 24 and float(d.dx.abs().max()) < 2 ** 24 and torch.equal(d.y, d.y.round()) and torch.equal(d.dx, d.dx.round())
    want_y, want_dx = (bf16r(d.y), bf16r(d.dx)) if dtype == "bf16" else (d.y, d.dx)
    dead = H.unreachable(c)
    got = {}
    for order in (0, 1):
        with k_order(ops, order, reserve):
            routes = _routes(ops, dtype, c)
            assert any(n.startswith("convbf2_kernel") for n in routes.values()), routes
            y, dx = _launch(ops, dtype, c, d, dtype == "f32" or ("fwd" in routes and bool(H.fwd_modes(c))))
            assert not ops.streamk_error_codes(), (tag, order)
        got[order] = (y, dx)
        for q, t, want in (("y", y, want_y), ("dx", dx, want_dx)):
            if t is None:
                continue
            assert t.dtype == (BF if dtype == "bf16" else torch.float32), (q, t.dtype)
            t64 = t.double().cpu()
            bad = t64 != want
            print("  %s %s reserve %d order %d %-2s (%s): %d of %d elements differ from the exact result" % (
                dtype, tag, reserve, order, q, routes.get("fwd" if q == "y" else "dx"), int(bad.sum()), bad.numel()))
            assert torch.equal(t64, want), "%s %s order %d: %s differs from the exact result in %d of %d elements, the first at %r: %r for %r" % (
                dtype, tag, order, q, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()), float(t64[bad][0]), float(want[bad][0]))
        if bool(dead.any()):
            z = dx[:, dead.to(DEV)].float()
            assert bool((z == 0).all()) and not bool(torch.signbit(z).any()), "%s order %d: unreachable input pixels are not exactly +0" % (tag, order)
    for a, b in zip(got[0], got[1]):
        assert (a is None and b is None) or torch.equal(a, b), "%s %s: the two K orders differ" % (dtype, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tag,reserve", LIST, ids=IDS)
def test_chunk_major_conv_sweep(ops, dtype, tag, reserve):  # noqa: F811
    """Under ops.SK_K_ORDER = 1, on the sweep's own random operands and at its own bars: y, forward sums under IN and BN, dx under no holder, an IN
    and a BN holder, the backward sums, dW (run_forward / run_backward of the dtype's sweep file).  Two guards against a vacuous pass:
    the switch reached the kernel -- where a convbf2 launch has nlive > 1 and nkc > 1 the summation order changed, so y or dx differs from order 0
    in at least one element; and what must not move did not -- dW (convbf_dw_kernel / convx3_dw_kernel are launched with korder = 0) and every y / dx
    the 4-wave convsk_kernel or a fall-back serves are bit-identical between the orders."""
    M = H if dtype == "bf16" else F
    c = case_of(dtype, tag)
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    d = M.reference(c)
    belows = {mode: M.below(c, mode, groups) for mode, groups in H.holder_modes(c)}
    dev = torch.device(DEV, torch.cuda.current_device())
    el = BF if dtype == "bf16" else torch.float32
    both = {}
    for order in (0, 1):
        with k_order(ops, order, reserve):
            launched = launches(ops, dtype, c, dev)
            routes = {role: name for role, name, _plan in launched}
            y, dx = _launch(ops, dtype, c, d, dtype == "f32" or ("fwd" in routes and bool(H.fwd_modes(c))))
            wd = torch.nn.Parameter(ops.to_weight_layout(d.w.float()).to(DEV))
            ops.conv_weight_grad(d.x.to(el).to(DEV), d.gy.to(el).to(DEV), wd, s, p)
            torch.cuda.synchronize()
            both[order] = (y, dx, wd.grad.clone())
            if order == 1:
                mixes = any(name.startswith("convbf2_kernel") and "mix" in reached(role, *segments(plan)) for role, name, plan in launched)
                expect = M.served(ops, c, dev)
                if reserve == 0 and tag in M.EXPECT:
                    assert expect == M.EXPECT[tag], (expect, M.EXPECT[tag])
                errs, name = {}, "%s %s [chunk-major%s]" % (dtype, tag, ", reserve %d" % reserve if reserve else "")
                if dtype == "bf16":
                    H.run_forward(ops, c, d, expect, name, errs)
                    H.run_backward(ops, c, d, belows, expect, name, errs, False)
                else:
                    F.run_forward(ops, c, d, name, errs)
                    F.run_backward(ops, c, d, belows, expect, name, errs, False)
                assert not ops.streamk_error_codes(), name
                print("  case %-44s fwd %-34s dX %-38s | %s" % (name, expect.fwd, expect.dx, "  ".join("%s %.2e" % kv for kv in errs.items())))
    (y0, dx0, dw0), (y1, dx1, dw1) = both[0], both[1]
    assert torch.equal(dw0, dw1), "%s: dW moved with the K order of the forward / dx kernels" % tag
    moved = []
    for role, a, b in (("fwd", y0, y1), ("dx", dx0, dx1)):
        if a is None:
            continue
        n = int((a != b).sum())
        print("  %s %s %s (%s): %d of %d elements differ between the K orders" % (dtype, tag, role, routes.get(role, "fall-back"), n, a.numel()))
        if routes.get(role, "").startswith("convbf2_kernel"):
            moved.append(n)
        else:
            assert n == 0, "%s %s: %s is served by %s, which has one K order, and moved with the switch" % (dtype, tag, role, routes.get(role, "a fall-back"))
    if mixes:
        assert any(moved), "%s %s: nothing differs between the K orders although a tile sums in another order: the switch did not reach the kernel" % (dtype, tag)


_PRESPLIT = [m for m in _presplit_test.pytestmark if m.name == "parametrize"][0].args[1]


@pytest.mark.gpu
@pytest.mark.parametrize("case", _PRESPLIT, ids=lambda c: c[0])
def test_presplit_weights_are_bit_identical_under_chunk_major(ops, case):  # noqa: F811
    """the three cases of test_ops_gpu.py::test_presplit_weights_are_bit_identical_to_the_in_kernel_split under ops.SK_K_ORDER = 1: the planes
    path (W3: byte shifts halved in load_prep, 64 bytes per plane and chunk) is bit-identical to the in-kernel split under the same order"""
    assert ops.F32_SPLIT
    prev_w3 = ops.W3_PRESPLIT
    try:
        with k_order(ops, 1):
            ops.W3_PRESPLIT = True
            _presplit_case(ops, case)
            assert not ops.streamk_error_codes()
    finally:
        ops.W3_PRESPLIT = prev_w3


@pytest.mark.gpu
def test_the_default_order_is_back_after_the_switch(ops):  # noqa: F811
    """a launch after k_order(1) has exited is tap-major again: bit-identical to the one before it, and not to the one inside (cout384: 9 live
    taps x 4 chunks on the 8-wave kernel, the orders sum differently); the same after an exception inside the block"""
    c = case_of("f32", "cout384")
    d = F.reference(c)
    assert ops.SK_K_ORDER == 0
    before = _launch(ops, "f32", c, d, True, dx=False)[0]
    with k_order(ops, 1):
        inside = _launch(ops, "f32", c, d, True, dx=False)[0]
    assert ops.SK_K_ORDER == 0 and ops._K_ORDER_SET[0] == 0
    after = _launch(ops, "f32", c, d, True, dx=False)[0]
    assert torch.equal(before, after) and not torch.equal(before, inside)
    with pytest.raises(ZeroDivisionError):
        with k_order(ops, 1):
            1 / 0
    assert ops.SK_K_ORDER == 0 and ops._K_ORDER_SET[0] == 0
    assert torch.equal(before, _launch(ops, "f32", c, d, True, dx=False)[0])


# =============================================================================================================================
# `python tests/test_k_order_conv_sweep_gpu.py` prints which launch of LIST reaches which condition; `--all`: of every candidate of both sweeps
# =============================================================================================================================
def _print_coverage(entries):
    from speechdrivestemplates_amd import ops as o
    cov = coverage(o, entries)
    keys = list(CONDITIONS)
    print("%-5s %-14s %-3s %-4s %-38s %s" % ("dtype", "case", "rsv", "role", "kernel", " ".join("%-4s" % k for k in keys)))
    for (dtype, tag, reserve, role), (name, got) in cov.items():
        print("%-5s %-14s %-3d %-4s %-38s %s" % (dtype, tag, reserve, role, name, " ".join("%-4s" % ("x" if k in got else ".") for k in keys)))
    for k, text in CONDITIONS.items():
        who = ["%s %s%s %s" % (d, t, "+r%d" % r if r else "", role) for (d, t, r, role), (_n, got) in cov.items() if k in got]
        print("(%s) %s:\n      %s" % (k, text, ", ".join(who) or "-- nobody"))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if "--all" in sys.argv:
        _print_coverage([("bf16", c[0], r) for r in (0, RESERVE) for c in H.CASES + NEW] + [("f32", c[0], r) for r in (0, RESERVE) for c in F.CASES + NEW_F32])
    else:
        _print_coverage(LIST)
