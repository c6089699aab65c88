"""Float64 emulation of the opt-in product arithmetic of the fp32-tensor conv kernels (csrc/conv.hip: conv_taps_bf_kernel<NS>,
conv_dw_kernel<.., true, NS>; ops.set_conv_math('bf16' | 'bf16x3' | 'bf16x6')), its host-side proofs, and the case table of the GPU sweep
(tests/test_conv_math_modes_sweep_gpu.py imports all three).  Nothing here needs a GPU.

The kernels round or split each fp32 OPERAND into bf16 pieces and multiply piece by piece on the bf16 MFMA with fp32 accumulation:
  bf16    x1 = rne_bf16(x)                                                   products a1 b1
  bf16x3  x1 = trunc_bf16(x), x2 = trunc_bf16(x - x1), the rest dropped      a1 b1 + a1 b2 + a2 b1
  bf16x6  x1, x2 as above, x3 = (x - x1) - x2 (exact: 8 + 8 + 8 bits)        the three above + a2 b2 + a1 b3 + a3 b1
The convolution is bilinear, so the value a mode defines -- before any accumulation error -- is a fixed SUM OF FLOAT64 CONVOLUTIONS over those
operand pieces: emulated().  Only the fp32 accumulation order separates a correct kernel from it, which is why every mode can be held to the
exact-fp32 sweep's bars (4e-6 / 4e-6 / 8e-6) instead of the modes' own rounding (3e-6 / 1e-4 / 1.5e-2 against plain float64).

emulated() evaluates the pair sum grouped by the a piece -- sum_i op(a_i, sum_{j: (i, j) in pairs} b_j) -- one convolution per a piece instead
of one per pair.  The inner sums are exact in float64 (the pieces of one value are disjoint bit ranges of a 24-bit significand), so this is the
same sum of products up to float64 rounding (1e-16)."""
import functools
import zlib

import torch
import torch.nn.functional as F

MODES = ("bf16", "bf16x3", "bf16x6")
PAIRS = {
    "bf16": ((0, 0),),
    "bf16x3": ((0, 0), (0, 1), (1, 0)),
    "bf16x6": ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)),
}
BARS_VS_FLOAT64 = {"bf16x6": 3e-6, "bf16x3": 1e-4, "bf16": 1.5e-2}  # the bars of tests/test_ops_gpu.py::test_conv_math_modes
TOL_Y, TOL_DX, TOL_DW = 4e-6, 4e-6, 8e-6                            # the bars of tests/test_f32_conv_sweep_gpu.py, quantity by quantity
# Below 2^-100 the low pieces of a split go subnormal and a truncation to bf16 keeps fewer than 8 bits of them (the kernel's own third piece
# would drop bits there too); the identities that speak of bf16-representable pieces are stated, and the sweep's operands asserted, above it.
SPLIT_FLOOR = 2.0 ** -100


def trunc_bf16(x):
    """fp32 -> fp32 with the low 16 bits of the word cleared (csrc/conv.hip: trunc_bf16 / pack_hi16)"""
    assert x.dtype == torch.float32
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def rne_bf16(x):
    assert x.dtype == torch.float32
    return x.to(torch.bfloat16).float()


def pieces(t, mode, first=None, rest=None):
    """The float64 pieces of an fp32 tensor as ``mode`` multiplies them.  ``first`` / ``rest``: the fp32 -> bf16 maps of the first piece and of
    the later ones -- the kernels' by default (rounding for 'bf16', truncation in the splits); the sensitivity study passes others."""
    assert t.dtype == torch.float32, "the kernels split fp32 values: hand over the fp32 tensor itself"
    first = first or (rne_bf16 if mode == "bf16" else trunc_bf16)
    rest = rest or trunc_bf16
    x1 = first(t)
    if mode == "bf16":
        return [x1.double()]
    r1 = t - x1       # exact in fp32 (Sterbenz-like: x1 holds the leading bits of t)
    x2 = rest(r1)
    if mode == "bf16x3":
        return [x1.double(), x2.double()]
    assert mode == "bf16x6", mode
    return [x1.double(), x2.double(), r1.double() - x2.double()]


def emulated(op, a, b, mode, pairs=None, pieces_a=None, pieces_b=None):
    """float64 value of the bilinear ``op(a, b)`` under ``mode``: the sum of op over the piece pairs the kernel multiplies (see the module
    docstring for the grouping).  ``op`` takes and returns float64 tensors; ``a`` and ``b`` are fp32."""
    pa = pieces_a if pieces_a is not None else pieces(a, mode)
    pb = pieces_b if pieces_b is not None else pieces(b, mode)
    out = None
    for i in range(len(pa)):
        js = [j for (ii, j) in (pairs if pairs is not None else PAIRS[mode]) if ii == i]
        if not js:
            continue
        term = op(pa[i], sum(pb[j] for j in js))
        out = term if out is None else out + term
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the three bilinear operations of a layer, on channels-first float64 tensors; nd = 2 (Conv2d) or 1 (Conv1d)
# ---------------------------------------------------------------------------------------------------------------------------------
def _conv(nd):
    return F.conv2d if nd == 2 else F.conv1d


def op_forward(nd, s, p):
    return lambda x, w: _conv(nd)(x, w, None, s, p)


def op_input_grad(nd, s, p, x_shape):
    """(gy, w) -> dL/dx by autograd on float64"""
    def op(gy, w):
        x0 = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(_conv(nd)(x0, w, None, s, p), x0, gy)[0]
    return op


def op_weight_grad(nd, s, p, w_shape):
    """(x, gy) -> dL/dw by autograd on float64"""
    def op(x, gy):
        w0 = torch.zeros(w_shape, dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(_conv(nd)(x, w0, None, s, p), w0, gy)[0]
    return op


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------------------------------------------
# The sweep's cases: (tag, nd, B, Hi, Wi, Cin, Cout, kh, kw, s, p); a 1-D case has Hi = kh = 1 and neither stride nor padding on that axis.
# The tile is 64 rows (M = B Ho Wo) x 64 columns (Cout), a K step 32 channels of one tap; the host asks for a K split of k =
# min(ceil(512 / tiles), steps / 4, 16) slices while a launch has fewer than 192 tiles (768 in 1-D), so most small cases run split-K + reduce;
# the cases marked "unsplit" store from the kernel's own epilogue.  dX swaps the roles: its rows are the input pixels of a stride class, its
# columns Cin, its K the Cout channels; it stays on the bf16 MFMA only while Cout % 32 == 0 (forward: Cin % 32 == 0; dW: Cin % 4 == Cout % 4 == 0).
# ---------------------------------------------------------------------------------------------------------------------------------
CASES = [
    # ---- 3x3 p1 s1: row-tile edges M = 15, 64, 65, 129 and column-tile edges Cout = 4, 60, 64, 68, 132; Cin = 32, 64, 96
    ("3x3-m15", 2, 1, 3, 5, 32, 64, 3, 3, 1, 1),        # M = 15 < one tile, B = 1; dX: 32 of 64 columns, K = 2 chunks x 9 taps
    ("3x3-m64", 2, 1, 8, 8, 64, 64, 3, 3, 1, 1),        # M = 64: exactly one tile, B = 1
    ("3x3-m65-c4", 2, 5, 1, 13, 32, 4, 3, 3, 1, 1),     # M = 65: a tile and one row; Cout = 4; Hi = 1: six of nine taps dead everywhere; dX falls back
    ("3x3-m129-c60", 2, 1, 3, 43, 96, 60, 3, 3, 1, 1),  # M = 129: two tiles and one row, B = 1; Cin = 96: three chunks; Cout = 60; dX falls back
    ("3x3-c68", 2, 2, 5, 7, 64, 68, 3, 3, 1, 1),        # Cout = 68: a column tile of 4; M = 70; dX falls back
    ("3x3-c132", 2, 2, 6, 6, 32, 132, 3, 3, 1, 1),      # Cout = 132: three column tiles, the last of 4; dX falls back
    ("3x3-cin96-c96", 2, 2, 7, 9, 96, 96, 3, 3, 1, 1),  # forward and dX alike: three chunks, a column tile of 32; M = 126
    ("3x3-unsplit", 2, 4, 32, 32, 32, 192, 3, 3, 1, 1),  # 192 tiles: the forward launch is UNSPLIT with nine taps; dX: 64 tiles, k = 8; dW: M = 4096
    # ---- 4x4 s2 p1: the input gradient has four stride classes of four taps, one launch each under a math mode
    ("k4s2", 2, 2, 10, 14, 64, 64, 4, 4, 2, 1),         # M = 70; classes of 35 rows
    ("k4s2-odd", 2, 1, 9, 11, 32, 96, 4, 4, 2, 1),      # odd Hi, Wi: classes of 30, 25, 24, 20 rows; B = 1; dX: three chunks, 32 columns
    ("k4s2-c32", 2, 2, 18, 18, 64, 32, 4, 4, 2, 1),     # classes of 162 rows and four K steps: UNSPLIT class launches ('f32' mode: one fused launch)
    # ---- (6,3) p0 on a 6-row image: Ho = 1, 18 taps (launch_taps computes its tile rotation for the dX launch; conv_taps_bf_kernel takes the plain geometry)
    ("k6x3", 2, 2, 6, 40, 64, 128, 6, 3, 1, 0),         # M = 76
    # ---- 1x1: unsplit (three / five K steps)
    ("k1", 2, 3, 5, 9, 96, 160, 1, 1, 1, 0),            # M = 135; Cout = 160: a column tile of 32; dX: five chunks, 96 columns
    # ---- 1-D
    ("1d-k3", 1, 3, 1, 21, 64, 64, 1, 3, 1, 1),         # M = 63, unsplit (six steps)
    ("1d-k4s2-t64", 1, 2, 1, 64, 64, 128, 1, 4, 2, 1),  # T = 64 -> 32: M = 64
    ("1d-k4s2-t37", 1, 3, 1, 37, 32, 64, 1, 4, 2, 1),   # T = 37 (odd) -> 18: classes of 19 and 18 positions; unsplit (four steps)
    # ---- split-K on the short 1-D layers that conv1d_small_kernel takes in fp32 mode (Cin = Cout = 256, T <= 8)
    ("1d-k4s2-t4", 1, 4, 1, 4, 256, 256, 1, 4, 2, 1),   # T = 4 -> 2: M = 8
    ("1d-k3-t8", 1, 4, 1, 8, 256, 256, 1, 3, 1, 1),     # M = 32
    ("1d-k3-t4", 1, 4, 1, 4, 256, 256, 1, 3, 1, 1),     # M = 16
    # ---- tap culling: an image smaller than its kernel
    ("cull-2x2", 2, 3, 2, 2, 32, 64, 3, 3, 1, 1),       # every row has four live taps of nine, the tile all nine; M = 12
    ("cull-1x3", 2, 2, 1, 3, 64, 32, 3, 3, 1, 1),       # three live taps of nine: the kernel splits 6 live steps where the host counted 18
    ("cull-1x1", 2, 5, 1, 1, 64, 64, 3, 3, 1, 1),       # ONE live tap: 2 live steps in k = 4 slices -- two slices run no step and store zeros
    # ---- input rows no output reads (stride 2 without padding over 10 rows: the last row, a whole row of the odd stride class without a live
    # tap -- the geometry of tests/test_ops_gpu.py::test_input_gradient_with_unreachable_rows with a kernel whose forward launch fits the tap table)
    ("unreach-k3s2", 2, 2, 10, 13, 32, 64, 3, 3, 2, 0),
    # ---- weight gradient: (Cin, Cout) = (36, 68) is on its vector path (% 4) with partial tiles both ways, M = 1000: seven row ranges;
    # forward (Cin = 36) and dX (Cout = 68) fall back to exact fp32
    ("dw-m1000", 2, 2, 20, 25, 36, 68, 3, 3, 1, 1),
    # ---- documented fall-backs on the 242-channel pose layers: forward and dW with Cin = 242, dX and dW with Cout = 242
    ("1d-cin242", 1, 3, 1, 21, 242, 64, 1, 3, 1, 1),
    ("1d-cout242", 1, 3, 1, 21, 64, 242, 1, 1, 1, 0),   # the forward launch stays on the bf16 MFMA: four column tiles, the last of 50
]
CASE = {c[0]: c for c in CASES}
SPLITK_1D = ("1d-k4s2-t4", "1d-k3-t8", "1d-k3-t4")   # must launch with splitk > 1 and off conv1d_small_kernel
ACCUMULATE = ("3x3-m15", "k4s2", "1d-k3", "dw-m1000", "1d-cin242")  # dW twice onto one .grad, then onto a pre-filled one


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def dims(c):
    tag, nd, B, Hi, Wi, Cin, Cout, kh, kw, s, p = c
    Ho = out_size(Hi, kh, s, p) if nd == 2 else 1
    return nd, B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, out_size(Wi, kw, s, p)


def on_mode(c):
    """(forward, dX, dW): does the launch stay on the bf16 MFMA under a math mode (else: the exact-fp32 kernel, silently)"""
    Cin, Cout = c[5], c[6]
    return Cin % 32 == 0, Cout % 32 == 0, Cin % 4 == 0 and Cout % 4 == 0


def _randn32(shape, g, scale=1.0):
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float()


@functools.lru_cache(maxsize=None)
def operands(tag):
    """(x, w, gy, bias) fp32, channels-first, seeded by the tag: randn ROUNDED TO fp32 -- the full 24-bit significand, so that the second and
    third pieces carry data -- and clear of the subnormal range of the splits (asserted)"""
    c = CASE[tag]
    nd, B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    g = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
    sp, ks, osp = ((Hi, Wi), (kh, kw), (Ho, Wo)) if nd == 2 else ((Wi,), (kw,), (Wo,))
    x = _randn32((B, Cin) + sp, g)
    w = _randn32((Cout, Cin) + ks, g, (2.0 / (Cin * kh * kw)) ** 0.5)
    gy = _randn32((B, Cout) + osp, g)
    bias = _randn32((Cout,), g)
    for t in (x, w, gy):
        assert float(t.abs().min()) > SPLIT_FLOOR
        assert not torch.equal(trunc_bf16(t - trunc_bf16(t)), t - trunc_bf16(t)), "the low pieces carry no data"
    return x, w, gy, bias


def ops_of(c):
    """{quantity: (op, a, b)} -- a and b in the order the kernels take them (the pair sets are symmetric, so the order does not matter)"""
    nd, B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    x, w, gy, _bias = operands(c[0])
    return {"y": (op_forward(nd, s, p), x, w), "dx": (op_input_grad(nd, s, p, tuple(x.shape)), gy, w),
            "dw": (op_weight_grad(nd, s, p, tuple(w.shape)), x, gy)}


@functools.lru_cache(maxsize=None)
def reference(tag, mode):
    """{'y', 'dx', 'dw'} channels-first float64: plain float64 for mode 'f64', else the mode's emulation.  Shared, never written to."""
    out = {}
    for q, (op, a, b) in ops_of(CASE[tag]).items():
        out[q] = op(a.double(), b.double()) if mode == "f64" else emulated(op, a, b, mode)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# host proofs
# ---------------------------------------------------------------------------------------------------------------------------------
def _bits(v):
    return torch.tensor(v, dtype=torch.int32).view(torch.float32)


def _probe_values():
    g = torch.Generator().manual_seed(20261021)
    r = torch.randn(200000, generator=g)                                        # both signs
    wide = r * torch.exp2(torch.randint(-60, 60, r.shape, generator=g).float())  # across the exponent range
    pow2 = torch.exp2(torch.arange(-100, 101).float())
    normal = torch.cat([r, wide, pow2, -pow2, torch.tensor([0.0, -0.0, 1.0, -1.0, 3.0, 1.0 + 2.0 ** -23, 2.0 - 2.0 ** -23, 2.0 ** 127])])
    # a few subnormals (and the smallest normals, whose low pieces are subnormal): only the sum identity is claimed for these
    tiny = torch.cat([_bits([1, 2, 0x7fff, 0x8000, 0x12345, 0x7fffff, 0x800000, 0x812345]), -_bits([1, 0x12345, 0x7fffff, 0x812345])])
    return normal, tiny


def _bf16_representable(p):
    p32 = p.float()
    return torch.equal(p32.double(), p) and torch.equal(trunc_bf16(p32), p32)


def test_bf16x6_pieces_sum_to_the_input_exactly():
    normal, tiny = _probe_values()
    for v in (normal, tiny):
        ps = pieces(v, "bf16x6")
        assert len(ps) == 3 and torch.equal(ps[0] + ps[1] + ps[2], v.double())
        assert torch.equal(ps[0] + (ps[1] + ps[2]), v.double())  # (any association: the pieces are disjoint bit ranges)
    z = pieces(torch.tensor([0.0, -0.0]), "bf16x6")
    assert all(bool((p == 0).all()) for p in z) and bool(torch.signbit(z[0][1])) and not bool(torch.signbit(z[0][0]))


def test_every_piece_is_bf16_representable():
    normal, _tiny = _probe_values()
    v = normal[(normal.abs() > SPLIT_FLOOR) | (normal == 0)]
    assert v.numel() > 400000
    for mode in MODES:
        for k, p in enumerate(pieces(v, mode)):
            assert _bf16_representable(p), "%s piece %d" % (mode, k + 1)
    # the kernel's own third piece is trunc_bf16((x - x1) - x2): the same value, since that remainder has at most 8 significant bits
    x1 = trunc_bf16(v)
    r2 = (v - x1) - trunc_bf16(v - x1)
    assert torch.equal(trunc_bf16(r2), r2) and torch.equal(r2.double(), pieces(v, "bf16x6")[2])


def test_bf16x3_remainder_is_below_2_to_minus_15():
    normal, _tiny = _probe_values()
    v = normal[normal.abs() > SPLIT_FLOOR]
    x1, x2 = pieces(v, "bf16x3")
    rem = (v.double() - x1 - x2).abs()
    assert bool((rem <= 2.0 ** -15 * v.double().abs()).all())
    assert float((rem / v.double().abs()).max()) > 2.0 ** -16  # (and the bound is not slack by more than a bit)
    # truncation: every piece has the sign of x (or is zero) -- the dropped remainder is a BIAS towards zero, not noise
    assert bool(((x1 * v.double()) >= 0).all()) and bool(((x2 * v.double()) >= 0).all())


def test_bf16_piece_is_the_rounded_value():
    normal, tiny = _probe_values()
    for v in (normal, tiny):
        (p,) = pieces(v, "bf16")
        assert torch.equal(p, v.to(torch.bfloat16).double())
    assert not torch.equal(pieces(normal, "bf16")[0], pieces(normal, "bf16x3")[0])  # (rounding is not truncation)


def test_emulation_orders_the_modes_within_their_stated_bars():
    """One small conv: the emulated y, dx, dW lie within the bars test_conv_math_modes states for the modes (3e-6, 1e-4, 1.5e-2 of max|ref|) and
    the distances are ordered bf16x6 < bf16x3 < bf16 -- the emulation models what the modes claim; bf16x6 is exact to 2^-23 per product."""
    tag = "3x3-cin96-c96"
    ref = reference(tag, "f64")
    for q in ("y", "dx", "dw"):
        d = {mode: rel(reference(tag, mode)[q], ref[q]) for mode in MODES}
        print("  %s %-2s" % (tag, q), "  ".join("%s %.2e" % kv for kv in d.items()))
        assert d["bf16x6"] < d["bf16x3"] < d["bf16"], (q, d)
        for mode in MODES:
            assert d[mode] < BARS_VS_FLOAT64[mode], (q, mode, d[mode])
        assert d["bf16x6"] < 3 * 2.0 ** -23 and d["bf16x3"] > 10 * d["bf16x6"] and d["bf16"] > 10 * d["bf16x3"]


def test_grouped_pair_sum_is_the_pair_sum():
    """emulated() groups the pairs by the a piece; pair by pair gives the same value to float64 rounding"""
    tag = "cull-2x2"
    for q, (op, a, b) in ops_of(CASE[tag]).items():
        for mode in MODES:
            pa, pb = pieces(a, mode), pieces(b, mode)
            flat = sum(op(pa[i], pb[j]) for i, j in PAIRS[mode])
            assert rel(emulated(op, a, b, mode), flat) < 1e-14


# ---- sensitivity: what the sweep's bars can see, shown on the reference instead of on a deliberately broken kernel
SENSITIVITY_CASES = ("3x3-m15", "cull-2x2", "k4s2-odd", "1d-k3", "k1")
_TOL = {"y": TOL_Y, "dx": TOL_DX, "dw": TOL_DW}


def _zero_border_tap(c, x, w):
    """the forward value with ONE tap skipped at ONE border of the image: the centre-row, right-hand tap (kw - 1) on the output's first column"""
    nd, B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    w1 = torch.zeros_like(w)
    tap = (kh // 2, kw - 1) if nd == 2 else (kw - 1,)
    w1[(slice(None), slice(None)) + tap] = w[(slice(None), slice(None)) + tap]
    only = op_forward(nd, s, p)(x, w1)
    out = torch.zeros_like(only)
    out[..., 0] = only[..., 0]
    return out


def sensitivity_rows():
    """(perturbation, case, mode, quantity, shift of the emulated reference / max|reference|, bar)"""
    rows = []
    for tag in SENSITIVITY_CASES:
        c = CASE[tag]
        for q, (op, a, b) in ops_of(c).items():
            for mode in MODES:
                ref = reference(tag, mode)[q]
                if mode != "bf16":  # a correction term dropped
                    got = emulated(op, a, b, mode, pairs=[pr for pr in PAIRS[mode] if pr != (1, 0)])
                    rows.append(("drop a2 b1", tag, mode, q, rel(got, ref), _TOL[q]))
                # the other rounding in the split: truncation <-> rounding to nearest even, in every piece
                other = trunc_bf16 if mode == "bf16" else rne_bf16
                got = emulated(op, a, b, mode, pieces_a=pieces(a, mode, other, other), pieces_b=pieces(b, mode, other, other))
                rows.append(("rounding swapped", tag, mode, q, rel(got, ref), _TOL[q]))
                if q == "y" and c[8] > 1:  # one border tap zeroed (the cases with a kernel wider than one tap)
                    pa, pb = pieces(a, mode), pieces(b, mode)
                    miss = sum(_zero_border_tap(c, pa[i], pb[j]) for i, j in PAIRS[mode])
                    rows.append(("one border tap zeroed", tag, mode, q, rel(ref - miss, ref), _TOL[q]))
    return rows


def test_bars_see_the_three_error_classes():
    """Each perturbation of the REFERENCE moves it by more than 10x the bar at some swept case: a kernel that made that error would fail there.
    Where a perturbation is invisible that is stated too: bf16x6 with a rounding split is another exact split (its six products differ from the
    kernel's by less than the dropped terms), and bf16x3 with a rounding split moves by the size of the bias it removes, a few bars."""
    rows = sensitivity_rows()
    worst = {}
    for what, tag, mode, q, shift, bar in rows:
        key = (what, mode)
        if shift / bar > worst.get(key, (0.0,))[0]:
            worst[key] = (shift / bar, tag, q, shift)
    for (what, mode), (ratio, tag, q, shift) in sorted(worst.items()):
        print("  %-22s %-7s largest shift %.2e = %6.1f bars (%s %s)" % (what, mode, shift, ratio, tag, q))
    for mode in ("bf16x3", "bf16x6"):
        assert worst[("drop a2 b1", mode)][0] > 10
    for mode in MODES:
        assert worst[("one border tap zeroed", mode)][0] > 10
    assert worst[("rounding swapped", "bf16")][0] > 10
    assert worst[("rounding swapped", "bf16x3")][0] > 5      # < 2^-15 = 7.6 bars of dW by construction: the bias of a truncated two-piece split
                                                             # (3.8e-5 on '3x3-m15' y: 9.6 stated bars, 37x the 1.0e-6 its recorded margin holds it to)
    assert worst[("rounding swapped", "bf16x6")][0] < 1      # an exact split either way


def test_case_table():
    """the table holds what its comments promise: the row, column and K edges, one case per fall-back, bounded size"""
    ms, couts, cins = set(), set(), set()
    for c in CASES:
        nd, B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
        assert Ho >= 1 and Wo >= 1 and (nd == 2 or (Hi == 1 and kh == 1))
        assert B * Ho * Wo * Cout <= 2 ** 21 and B * Hi * Wi * Cin <= 2 ** 21 and B * Ho * Wo * Cout * kh * kw * Cin <= 3e8
        if (kh, kw, s, p) == (3, 3, 1, 1):
            ms.add(B * Ho * Wo), couts.add(Cout), cins.add(Cin)
    assert {15, 64, 65, 129, 1000} <= ms and {4, 60, 64, 68, 132} <= couts and {32, 64, 96} <= cins
    assert any(c[2] == 1 for c in CASES)
    assert [on_mode(CASE[t]) for t in ("dw-m1000", "1d-cin242", "1d-cout242")] == [(False, False, True), (False, True, False), (True, False, False)]
    assert all(CASE[t][5] == CASE[t][6] == 256 and CASE[t][4] <= 8 for t in SPLITK_1D) and len(SPLITK_1D) >= 3


if __name__ == "__main__":
    for row in sensitivity_rows():
        print("%-22s %-14s %-7s %-2s shift %.3e  bar %.0e  x%.1f" % (row + (row[4] / row[5],)))
