"""The persistent Conv1d chain (csrc/chain1d.hip, ops.Chain1dFn) swept over the wirings chain_check() admits, against a plain float64 statement
of a generic chain.  tests/test_chain1d_gpu.py runs the generator's own sixteen-block wiring at T = 64 / 32 only: frame counts 64 .. 1 by halving,
upsampling ratio exactly 2, geometries (3, 1, 1) and (4, 2, 1).  ops.chain1d_usable hands the kernel anything chain_check() passes; this file runs it.

Families (CASES; every admitted row asserts ops.chain1d_usable, every refused row asserts refusal by chain1d_usable AND by the C ABI forward
entry, with nothing launched and the counters untouched):
  len-*    ONE plain block, (3, 1, 1) at 256 and 288 input channels and (4, 2, 1) at 256, T = 1 .. 64, B = 2: the row clamp (m >= M), the 2-wave /
           4-wave split at M = 32 | 33, the staging tails, the one-block chain (n = 1: the external gradient lands on block 0) and the 288-channel
           extra columns of the input gradient at ragged Ti
  geom-*   every (k, stride, pad) in {3, 4} x {1, 2} x {0 .. k-1} at Ti in {5, 33, 62, 63, 64}, B = 1: as the MIDDLE block of three (its input
           gradient is consumed) and as BLOCK 0 (256 channels: k 3 and 4; 288: k 3; k 4 at 288 is refused): both halos (the "after" rows exist only
           with pad = k - 1 or stride 2 on an odd Ti), the backward row function (num / stride, the off-grid test, to < To) at odd lengths and
           pad != 1, the LDS limit of 68 rows from both sides ((4, 2, 3): 63 and 62 fit exactly, 64 does not)
  up-*     U shapes as the generator's (two plain-stride blocks, the down blocks, one UPADD per level, one block after), B = 2: ratios 2 at ragged
           lengths, 1.5 .. 1.94 (T = 33), exactly 1, 64 / 63, 5 / 3 and 9 / 5 (the source index is an integer in real arithmetic), 7 / 5; the
           six-candidate window of the backward gather; a block that is ONLY an upsampling source; 2 -> 5 is refused
  fan-*    consumer tables: two direct consumers and no upsampling one; g_id0, g_id1 and g_up all set; 20 blocks; 21 are refused
  batch-*  the generator's wiring at T = 32 with 288 channels, B in {1, 7, 9, 33, 65}: windows of 8 clusters, launches of 32 clips, a last launch
           that owns ONE clip, counter slots reused by consecutive launches -- forward against float64 and z[i], dh[i] BIT-IDENTICAL to the B = 1
           run of clip i (a cluster's arithmetic does not depend on its slot or launch; no tolerance)
  bf16-*   ops.CHAIN_MATH = 'bf16' on one-block chains with bf16-representable operands (exact products: the forward keeps the fp32 bar; the
           input gradient against a float64 emulation that rounds dy to bf16, on seeds whose dy is clear of rounding ties: bf16_tie_margin), B = 1

Per value case: z, dh and EVERY weight gradient against float64 (the weight gradients come from the x / dy tensors the two launches leave in HBM,
consecutive slices of one allocation per kind: a lost, duplicated or overrun frame of any block shows in a dW or in a neighbour's), on memory
that was NaN-filled just before, a second run bit-identical, the cluster counters back at zero and no error word.  Bars are the project's:
forward 1e-5 of the tensor's maximum, input gradient and weight gradients 3e-5 (test_chain1d_gpu.py, test_conv1d_stage_lengths_gpu.py), bf16 input
gradient 1e-4.  FP32_REF_ERR would widen a bar to 4 x what fp32 torch on the CPU errs against float64; it is empty.

The kink: the network is piecewise linear, so every case has a SEED (SEEDS; default 0) whose float64 pre-activations all keep |u| >= KINK = 4e-6
from zero (twice the DELTA of test_chain1d_gpu.py; asserted, no element excluded, no flip accounting) for the real slope 0.2, and runs once more
with slope 1.0 under another seed.  `python tests/test_chain1d_sweep_gpu.py --seeds` prints the first passing seed per case (CPU only)."""
import collections
import functools
import os
import sys
import zlib

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda"
SLOPE, EPS = 0.2, 1e-5  # EPS == ops.BN_EPS (asserted by the oracle tie)
TOL_FWD, TOL_GRAD, TOL_BF16_DX = 1e-5, 3e-5, 1e-4
KINK = 4e-6
OTHER_SEED = 1000  # the slope-1.0 run of every case
P, N, U = 0, 1, 2  # _lib.CHAIN_PLAIN, CHAIN_NORM, CHAIN_UPADD
B3 = (3, 1, 1)

Case = collections.namedtuple("Case", "tag T cin0 B spec admitted defer")
Data = collections.namedtuple("Data", "h gz ws")
Ref = collections.namedtuple("Ref", "z dh dws dys umin")


def _out(Ti, k, s, p):
    return (Ti + 2 * p - k) // s + 1 if Ti + 2 * p >= k else 0


def _fits(Ti, k, s, p):
    """chain_check(): 1 <= To <= 64 and the padded tile within the 68 LDS rows"""
    To = _out(Ti, k, s, p)
    after = max(0, (To - 1) * s + k - 1 - p - (Ti - 1))
    return 1 <= To <= 64 and p + Ti + after <= 68


def _ushape(downs):
    """generator.py:53-85 in small: e0, e1 at full length, the down blocks, one UPADD per level (skips deepest-but-one .. e1), one block after"""
    spec = [B3 + (P, -1, -1), B3 + (N, 0, -1)]
    for g in downs:
        spec.append(tuple(g) + (N, len(spec) - 1, -1))
    deepest = len(spec) - 1
    for j in range(len(downs)):
        spec.append(B3 + (U, len(spec) - 1, deepest - 1 - j))
    spec.append(B3 + (N, len(spec) - 1, -1))
    return tuple(spec)


def generator_wiring():
    w = [(P, -1, -1)] + [(N, i - 1, -1) for i in range(1, 7)] + [(U, 6 + j, 5 - j) for j in range(5)] + [(N, 11 + j, -1) for j in range(4)]
    down = [False, False, True, True, True, True, True] + [False] * 9
    return tuple(((4, 2, 1) if d else B3) + x for d, x in zip(down, w))


LEN_T = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 63, 64)
GEOMS = [(k, s, p) for k in (3, 4) for s in (1, 2) for p in range(k)]
GEOM_T = (5, 33, 62, 63, 64)


def _cases():
    out = []

    def add(tag, T, cin0, B, spec, admitted=True, defer=False):
        out.append(Case(tag, T, cin0, B, tuple(spec), admitted, defer))

    for name, g, cin0 in (("k3", B3, 256), ("k3c288", B3, 288), ("k4s2", (4, 2, 1), 256)):
        for T in LEN_T:
            if _out(T, *g) >= 1:
                add("len-%s-T%d" % (name, T), T, cin0, 2, [g + (P, -1, -1)])
    for (k, s, p) in GEOMS:
        for T in GEOM_T:
            g, ok = "k%ds%dp%d-T%d" % (k, s, p, T), _fits(T, k, s, p)
            add("geom-mid-" + g, T, 256, 1, [B3 + (P, -1, -1), (k, s, p, N, 0, -1), B3 + (N, 1, -1)], ok)
            add("geom-b0-" + g, T, 256, 1, [(k, s, p, P, -1, -1), B3 + (N, 0, -1)], ok)
            add("geom-b0c288-" + g, T, 288, 1, [(k, s, p, P, -1, -1), B3 + (N, 0, -1)], ok and k == 3)
    d321 = (3, 2, 1)
    add("up-T33", 33, 256, 2, _ushape([d321] * 6), defer=True)         # 33 17 9 5 3 2 1: ratios 2, 1.5, 1.67, 1.8, 1.89, 1.94
    add("up-T47", 47, 256, 2, _ushape([d321] * 6))                     # 47 24 12 6 3 2 1
    add("up-T64", 64, 256, 2, _ushape([d321] * 6))                     # 64 32 16 8 4 2 1
    add("up-T40k4", 40, 256, 2, _ushape([(4, 2, 1)] * 3), defer=True)  # 40 20 10 5: ratio 2 at ragged lengths
    add("up-ratio1-T19", 19, 256, 2, _ushape([B3]))
    add("up-64of63", 64, 256, 2, _ushape([(4, 1, 1)]))
    add("up-5of3", 5, 256, 2, _ushape([d321]))
    add("up-9of5", 9, 256, 2, _ushape([d321]))
    add("up-7of5", 7, 256, 2, _ushape([(3, 1, 0)]))
    add("up-5of2-refused", 5, 256, 2, [B3 + (P, -1, -1), B3 + (N, 0, -1), d321 + (N, 1, -1), d321 + (N, 2, -1), B3 + (U, 3, 1)], admitted=False)
    # block 0 feeds two NORM blocks that an UPADD of ratio 1 merges: two direct consumers, no upsampling one; block 1 is only an upsampling source
    add("fan-two-direct-T21", 21, 256, 2, [B3 + (P, -1, -1), B3 + (N, 0, -1), B3 + (N, 0, -1), B3 + (U, 1, 2)])
    # block 1 [11] is a NORM source (2), an upsampling source (3: 11 -> 12) and a skip source (4: 10 -> 11); block 3 is only an upsampling source
    add("fan-all-three-T11", 11, 256, 2, [B3 + (P, -1, -1), B3 + (N, 0, -1), (4, 1, 2, N, 1, -1), (3, 1, 0, U, 1, 2), B3 + (U, 3, 1)])
    add("fan-20-blocks-T5", 5, 256, 2, [B3 + (P, -1, -1)] + [B3 + (N, i, -1) for i in range(19)])
    add("fan-21-blocks-refused", 5, 256, 2, [B3 + (P, -1, -1)] + [B3 + (N, i, -1) for i in range(20)], admitted=False)
    return out


CASES = _cases()
CASE = {c.tag: c for c in CASES}
VALUE_TAGS = [c.tag for c in CASES if c.admitted]
REFUSED_TAGS = [c.tag for c in CASES if not c.admitted]
BATCHES = (1, 7, 9, 33, 65)
BF16 = [("bf16-c%d-T%d" % (cin0, T), T, cin0) for cin0 in (256, 288) for T in (1, 17, 33, 64)]
for _tag, _T, _cin0 in BF16:
    CASE[_tag] = Case(_tag, _T, _cin0, 1, (B3 + (P, -1, -1),), True, False)  # (B = 1: see bf16_tie_margin)
SEEDED_TAGS = VALUE_TAGS + [t for t, _T, _c in BF16]

# wirings that only the consumer tables of the backward launch object to (chain_check() refuses them for every entry point)
CONSUMER_RULES = {
    "three direct consumers": (8, [B3 + (P, -1, -1), B3 + (N, 0, -1), B3 + (N, 0, -1), B3 + (N, 0, -1), B3 + (U, 1, 2), B3 + (U, 4, 3)]),
    "two upsampling consumers": (8, [B3 + (P, -1, -1), B3 + (N, 0, -1), B3 + (N, 0, -1), B3 + (U, 1, 2), B3 + (U, 1, 3)]),
    "a dead-end block": (8, [B3 + (P, -1, -1), B3 + (N, 0, -1), B3 + (N, 0, -1)]),
}

# tag -> the first seed whose float64 pre-activations all keep KINK from zero at slope 0.2 (0 where not listed); `--seeds` prints this table
SEEDS = {
    "len-k3c288-T33": 1, "len-k4s2-T63": 1, "geom-b0-k3s1p1-T64": 1, "geom-mid-k3s1p2-T62": 2, "geom-mid-k3s2p2-T63": 1, "geom-mid-k4s1p0-T63": 1,
    "geom-b0-k4s1p0-T64": 1, "geom-b0-k4s2p2-T33": 1, "up-T33": 1, "up-64of63": 1,
    # bf16: the kink and the bf16 rounding ties of dy (bf16_tie_margin)
    "bf16-c256-T33": 9, "bf16-c256-T64": 60, "bf16-c288-T17": 1, "bf16-c288-T33": 19, "bf16-c288-T64": 46,
}

# "tag name" -> fp32-torch-on-the-CPU error against float64 where 4 x that exceeds a bar (the bar is then 4 x this figure): empty
FP32_REF_ERR = {
}


def _threads():
    torch.set_num_threads(max(1, min(16, (os.cpu_count() or 2) // 2)))


def blocks_of(spec, T0, cin0):
    """[(Ti, To, Cin, k, stride, pad, mode, src_a, src_b)]: ops.chain_blocks without its refusal (a refused row still needs a table for the C ABI)"""
    out = []
    for (k, s, p, mode, sa, sb) in spec:
        Ti, Cin = (T0, cin0) if mode == P else (out[sa if mode == N else sb][1], 256)
        out.append((Ti, _out(Ti, k, s, p), Cin, k, s, p, mode, sa, sb))
    return out


def make_data(c, seed, bf16=False):
    """seeded on the CPU: h (B, T, cin0), gz (B, To of the last block, 256), logical weights (256, Cin, k)"""
    g = torch.Generator().manual_seed(zlib.crc32(c.tag.encode()) + seed)
    bl = blocks_of(c.spec, c.T, c.cin0)
    ws = [torch.randn((256, b[2], b[3]), generator=g) * (2.0 / (b[2] * b[3])) ** 0.5 for b in bl]
    h, gz = torch.randn((c.B, c.T, c.cin0), generator=g), torch.randn((c.B, bl[-1][1], 256), generator=g)
    if bf16:
        h, ws = h.bfloat16().float(), [w.bfloat16().float() for w in ws]
    return Data(h, gz, ws)


def chain_ref(spec, d, slope, dtype=torch.float64, grads=True, mut=None):
    """The chain, plainly: per block F.conv1d without bias, normalisation of every frame over its 256 channels (biased variance, EPS;
    oracle/sdt_oracle.py::_norm, the 1-D IN branch), LeakyReLU; an UPADD block reads F.interpolate(a[src_a], Ti, 'linear') + a[src_b].
    Gradients by autograd on (z * gz).sum(); every pre-activation u is recorded (umin = min |u|).  `mut`: the mutations of test_bars_discriminate."""
    mut = mut or {}
    x0 = d.h.to(dtype).permute(0, 2, 1).contiguous().requires_grad_(grads)
    W = [w.to(dtype).clone().requires_grad_(grads) for w in d.ws]
    ys, a, umin = [], [], float("inf")
    for l, (k, s, p, mode, sa, sb) in enumerate(spec):
        if mode == P:
            x = x0
        elif mode == N:
            x = a[sa]
        else:
            skip = a[mut["skip"][1]] if mut.get("skip", (None,))[0] == l else a[sb]
            x = F.interpolate(a[sa], a[sb].shape[-1], mode="linear", align_corners=True if mut.get("align_corners") else None) + skip
        if mut.get("after_row") == l:  # the first halo row behind the last frame holds that frame instead of zeros
            y = F.conv1d(torch.cat([x.new_zeros(x.shape[:2] + (p,)), x, x[..., -1:], x.new_zeros(x.shape[:2] + (p - 1,))], -1), W[l], None, s, 0)
        elif mut.get("drop_x") == l:  # the x tensor left for the weight gradient lacks its last frame (values and dx unchanged)
            xw = x.detach().clone()
            xw[..., -1] = 0
            y = F.conv1d(x, W[l].detach(), None, s, p) + F.conv1d(xw, W[l], None, s, p) - F.conv1d(xw, W[l].detach(), None, s, p)
        else:
            y = F.conv1d(x, W[l], None, s, p)
        if grads:
            y.retain_grad()
        u = (y - y.mean(1, keepdim=True)) / torch.sqrt(y.var(1, unbiased=bool(mut.get("unbiased")), keepdim=True) + EPS)
        umin = min(umin, float(u.detach().abs().min()))
        ys.append(y)
        a.append(F.leaky_relu(u, slope))
    z = a[-1].permute(0, 2, 1)
    if not grads:
        return Ref(z.detach().contiguous(), None, None, None, umin)
    (z * d.gz.to(dtype)).sum().backward()
    return Ref(z.detach().contiguous(), x0.grad.permute(0, 2, 1).contiguous(), [w.grad for w in W], [y.grad for y in ys], umin)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def tol_for(key, stated):
    e32 = FP32_REF_ERR.get(key)
    return stated if e32 is None else max(stated, 4.0 * e32)


def errors(tag, got, ref, dx_bar=TOL_GRAD):
    """[(name, rel-max error, bar)] of z, dh and every dW; got = (z, dh or None, dws or None) in the device's layout (B, T, C) / (256, Cin, k)"""
    z, dh, dws = got
    rows = [("z", rel(z, ref.z), tol_for(tag + " z", TOL_FWD))]
    if dh is not None:
        rows.append(("dh", rel(dh, ref.dh), tol_for(tag + " dh", dx_bar)))
    for l, w in enumerate(dws or ()):
        rows.append(("dW[%d]" % l, rel(w, ref.dws[l]), tol_for(tag + " dW[%d]" % l, TOL_GRAD)))
    return rows


def failed(rows):
    return [(n, e, b) for n, e, b in rows if not e <= b]  # (a NaN fails)


def bf16_tie_margin(c, d, ref):
    """The bf16 kernel rounds dy (the normalisation backward of gz, its fp32 value) to bf16 in front of the input-gradient GEMM.  Where the float64
    dy lies within fp32 rounding of a TIE between two bf16 neighbours, the kernel's fp32 value may round the other way, and ONE such element of
    typical size moves three frames of dh by ulp_bf16(dy) * |w|: up to 5e-4 of max |dh| for a 2.5-sigma element, five times the bar (measured:
    bf16-c288-T33 under its kink-free seed 0, one element, clip 0 frames 2..4, every other element at 2e-7).  Like the kink this is a property of
    the DATA, so the seed of a bf16 case is also chosen, from the float64 run alone, such that no element whose flip could move dh by a quarter
    of the bar is closer to a tie than TIE (|dy| + rms dy) with TIE = 4 x 2^-24: four fp32 epsilons of the element itself, plus as much of the
    tensor's rms for the two frame means the normalisation backward subtracts.  Returns the smallest distance in those units.  B = 1 keeps the
    expected number of such elements per seed near two at T = 64, so that a seed exists within a few dozen."""
    dy = ref.dys[0]  # (B, 256, To) float64
    bits = dy.float().view(torch.int32)
    lo = (bits & -65536).view(torch.float32).double()          # towards zero on the bf16 grid
    hi = ((bits & -65536) + 65536).view(torch.float32).double()  # the next bf16 value away from zero
    wmax = d.ws[0].double().abs().amax((1, 2))  # per output channel
    k, s, p = c.spec[0][:3]
    dh_max = torch.nn.grad.conv1d_input((c.B, c.cin0, c.T), d.ws[0].double(), dy.float().bfloat16().double(), s, p).abs().max()
    matters = (hi - lo).abs() * wmax[None, :, None] / dh_max >= TOL_BF16_DX / 4
    dist = (dy - (lo + hi) / 2).abs() / (dy.abs() + dy.pow(2).mean().sqrt())
    return float(dist[matters].min()) if bool(matters.any()) else float("inf")


TIE = 4 * 2.0 ** -24


def first_seed(c, bf16=False, limit=1024):
    for seed in range(limit):
        d = make_data(c, seed, bf16)
        ref = chain_ref(c.spec, d, SLOPE, grads=bf16)
        if ref.umin >= KINK and (not bf16 or bf16_tie_margin(c, d, ref) >= TIE):
            return seed
    raise AssertionError("%s: no seed below %d keeps every pre-activation %g from zero" % (c.tag, limit, KINK))


# =============================================================================================================================
# host only
# =============================================================================================================================
def test_reference_equals_the_pinned_oracle_on_the_generators_wiring():
    """chain_ref on the generator's wiring (T = 32, B = 2, 288 channels) == oracle.unet_1d + the four decoder blocks, to 1e-12"""
    from speechdrivestemplates_amd import _lib, ops
    from test_chain1d_gpu import _oracle_chain, _wiring
    _threads()
    assert (P, N, U) == (_lib.CHAIN_PLAIN, _lib.CHAIN_NORM, _lib.CHAIN_UPADD) and EPS == ops.BN_EPS
    assert generator_wiring() == _wiring()
    c = Case("oracle-tie", 32, 288, 2, generator_wiring(), True, False)
    d = make_data(c, 0)
    ref = chain_ref(c.spec, d, SLOPE)
    hh = d.h.double().permute(0, 2, 1).contiguous().requires_grad_(True)
    ww = [w.double().clone().requires_grad_(True) for w in d.ws]
    out = _oracle_chain(hh, ww, (), None)
    (out * d.gz.double().permute(0, 2, 1)).sum().backward()
    assert rel(ref.z, out.detach().permute(0, 2, 1)) <= 1e-12 and rel(ref.dh, hh.grad.permute(0, 2, 1)) <= 1e-12
    assert max(rel(a, b.grad) for a, b in zip(ref.dws, ww)) <= 1e-12
    assert [b[:2] for b in blocks_of(c.spec, 32, 288)] == [b[:2] for b in ops.chain_blocks(c.spec, 32, 288)]


def test_table_reaches_what_it_claims():
    """the shapes behind the family descriptions, from the table alone"""
    tags = set(CASE)
    assert len(tags) == len(CASES) + len(BF16)
    b = {t: blocks_of(CASE[t].spec, CASE[t].T, CASE[t].cin0) for t in tags}
    assert [x[0] for x in b["up-T33"]][:8] == [33, 33, 33, 17, 9, 5, 3, 2] and b["up-T33"][7][1] == 1 and len(b["up-T33"]) == 15
    assert [x[1] for x in b["up-T40k4"]][1:5] == [40, 20, 10, 5]
    assert b["up-64of63"][2][1] == 63 and b["up-7of5"][2][1] == 5 and b["up-5of3"][2][1] == 3 and b["up-9of5"][2][1] == 5
    assert b["fan-all-three-T11"][3][:2] == (12, 10) and b["fan-all-three-T11"][4][:2] == (11, 11)
    # the LDS limit from both sides, To > 64, To < 1 and the 288-channel k 4 refusal are all in the table
    assert CASE["geom-mid-k4s2p3-T63"].admitted and CASE["geom-mid-k4s2p3-T62"].admitted and not CASE["geom-mid-k4s2p3-T64"].admitted
    assert not CASE["geom-mid-k3s1p2-T63"].admitted and CASE["geom-mid-k3s1p2-T62"].admitted and not CASE["geom-b0-k4s1p3-T62"].admitted
    assert CASE["geom-b0c288-k3s2p0-T5"].admitted and not any(CASE[t].admitted for t in tags if t.startswith("geom-b0c288-k4"))
    assert all(c.admitted for c in CASES if c.T == 5 and c.tag.startswith("geom-mid"))
    assert sum(c.defer for c in CASES) == 2 and all(len(c.spec) <= 20 for c in CASES if c.admitted)


def test_committed_seeds_are_the_first_passing_ones():
    """what `--seeds` prints == SEEDS: every seed before a case's committed one has a pre-activation within KINK of zero, the committed one none"""
    _threads()
    for tag in SEEDED_TAGS:
        assert first_seed(CASE[tag], tag.startswith("bf16-")) == SEEDS.get(tag, 0), tag
    assert set(SEEDS) <= set(SEEDED_TAGS) and all(SEEDS.values())


@functools.lru_cache(maxsize=None)
def cpu_fp32_rows(tag):
    """(key, fp32-torch-vs-float64 error, stated bar) of every check of a case, both slopes: measured against float64, never against the kernel"""
    c, rows = CASE[tag], []
    for slope, seed in ((SLOPE, SEEDS.get(tag, 0)), (1.0, OTHER_SEED)):
        d = make_data(c, seed)
        r64, r32 = chain_ref(c.spec, d, slope), chain_ref(c.spec, d, slope, torch.float32)
        rows += [("%s %s" % (tag, n), e, b) for n, e, b in errors("", (r32.z, r32.dh, r32.dws), r64)]
    return tuple(rows)


def test_cpu_fp32_stays_below_a_quarter_of_the_bars():
    _threads()
    seen = set()
    for tag in VALUE_TAGS:
        for key, e, stated in cpu_fp32_rows(tag):
            seen.add(key)
            if key in FP32_REF_ERR:
                assert FP32_REF_ERR[key] / 1.5 <= e <= 1.5 * FP32_REF_ERR[key] and 4.0 * FP32_REF_ERR[key] > 0.8 * stated, (key, e)
            else:
                assert 4.0 * e <= stated, "%s: fp32 torch on the CPU errs by %.2e, more than a quarter of %.1e: list it in FP32_REF_ERR" % (key, e, stated)
    assert set(FP32_REF_ERR) <= seen


def _batch_case(B):
    return Case("batch-%d" % B, 32, 288, B, generator_wiring(), True, False)


def test_bars_discriminate():
    """A mutated float64 reference in the device result's place fails a bar on the named case; the unmutated fp32 CPU run passes all of them."""
    _threads()

    def refs(tag, **mut):
        c = CASE[tag]
        d = make_data(c, SEEDS.get(tag, 0))
        return c, d, chain_ref(c.spec, d, SLOPE), (chain_ref(c.spec, d, SLOPE, mut=mut) if mut else None)

    def names(tag, ref, got):
        return [n for n, _e, _b in failed(errors(tag, got, ref))]

    # the last frame of a ragged block dropped from x: that block's weight gradient, and nothing else
    c, d, ref, m = refs("geom-mid-k3s1p1-T33", drop_x=2)
    assert names(c.tag, ref, (m.z, m.dh, m.dws)) == ["dW[2]"]
    r32 = chain_ref(c.spec, d, SLOPE, torch.float32)
    assert not failed(errors(c.tag, (r32.z, r32.dh, r32.dws), ref))
    # align_corners=True; the skip taken from the neighbouring block of the same length (e0 instead of e1)
    c, d, ref, m = refs("up-T33", align_corners=True)
    assert "z" in names(c.tag, ref, (m.z, m.dh, m.dws)) and "dh" in names(c.tag, ref, (m.z, m.dh, m.dws))
    last_up = max(l for l, b in enumerate(c.spec) if b[3] == U)
    assert c.spec[last_up][5] == 1
    c, d, ref, m = refs("up-T33", skip=(last_up, 0))
    assert "z" in names(c.tag, ref, (m.z, m.dh, m.dws))
    # pad off by one on the `after` side: the first halo row behind the data holds the last frame
    c, d, ref, m = refs("geom-mid-k3s1p2-T33", after_row=1)
    assert "z" in names(c.tag, ref, (m.z, m.dh, m.dws))
    # an odd-length stride-2 backward credits the off-grid tap: dx[ti] += dy[(ti + pad - tap) // 2] w[tap] for odd ti + pad - tap as well
    c, d, ref, _m = refs("len-k4s2-T33")
    (k, s, p, _mode, _sa, _sb), dy, w = c.spec[0], ref.dys[0], d.ws[0].double()
    dx = torch.zeros_like(ref.dh)
    for ti in range(c.T):
        for tap in range(k):
            num = ti + p - tap
            if num >= 0 and num // s < dy.shape[-1]:
                dx[:, ti] += dy[:, :, num // s] @ w[:, :, tap]
    on_grid = torch.nn.grad.conv1d_input((c.B, c.cin0, c.T), w, dy, s, p).permute(0, 2, 1)
    assert rel(on_grid, ref.dh) <= 1e-12 and names(c.tag, ref, (ref.z, dx, ref.dws)) == ["dh"]
    # unbiased variance
    c, d, ref, m = refs("len-k3-T17", unbiased=True)
    assert "z" in names(c.tag, ref, (m.z, m.dh, m.dws))
    # the 288-channel extra input-gradient columns left at zero
    c, d, ref, _m = refs("len-k3c288-T17")
    dh0 = ref.dh.clone()
    dh0[..., 256:] = 0
    assert names(c.tag, ref, (ref.z, dh0, ref.dws)) == ["dh"]
    # clip B - 1 of a 33-clip batch replaced by clip 0
    c = _batch_case(33)
    z = chain_ref(c.spec, make_data(c, 0), SLOPE, grads=False).z
    zm = z.clone()
    zm[32] = z[0]
    assert rel(zm, z) > TOL_FWD and not torch.equal(zm[32], z[32])


# =============================================================================================================================
# device
# =============================================================================================================================
def _poison(c):
    """NaN-filled tensors of the sizes Chain1dFn.forward allocates with torch.empty (y, x, zout, dy, dx: one allocation per kind), allocated
    together and freed right before the forward: a frame nobody writes reads as NaN"""
    bl = blocks_of(c.spec, c.T, c.cin0)
    ysz, xsz, dsz = sum(c.B * b[1] * 256 for b in bl), sum(c.B * b[0] * 256 for b in bl[1:]), sum(c.B * b[0] * b[2] for b in bl)
    ts = [torch.full((n,), float("nan"), device=DEV) for n in (ysz, xsz, c.B * bl[-1][1] * 256, ysz, dsz) if n]
    del ts


def device_run(ops, c, d, slope, backward=True):
    """ops.Chain1dFn forward (+ backward, the weight gradients deferred into the grouped launch where the case says so) -> z, dh, [dW] on the device"""
    dev = torch.device(DEV, 0)
    wd = [torch.nn.Parameter(ops.to_weight_layout(w.to(DEV))) for w in d.ws]
    hd, gz = d.h.to(DEV).requires_grad_(backward), d.gz.to(DEV)
    assert ops.chain1d_usable(hd, c.spec, wd), "%s: chain_check() admits this wiring by its rules, chain1d_usable says no" % c.tag
    _poison(c)
    ops.begin_step(dev)
    if not backward:
        with torch.no_grad():
            z = ops.Chain1dFn.apply(hd, c.spec, slope, *wd)
    else:
        z = ops.Chain1dFn.apply(hd, c.spec, slope, *wd)
        if c.defer:
            ops.defer_small_dw(True)
        try:
            z.backward(gz)
        finally:
            if c.defer:
                ops.defer_small_dw(False)
                ops.flush_deferred_dw()
    ops.join_side_stream()
    torch.cuda.synchronize()
    assert ops.streamk_error_codes() == {}, c.tag
    assert int(ops._chain_ws(dev).abs().sum().item()) == 0, "%s: the cluster counters are not back at zero" % c.tag
    return z.detach(), (hd.grad if backward else None), ([w.grad.detach() for w in wd] if backward else None)


def _to_cpu(got):
    z, dh, dws = got
    return z.double().cpu(), None if dh is None else dh.double().cpu(), None if dws is None else [w.double().cpu() for w in dws]


def _report(tag, label, rows):
    dw = [(e, n) for n, e, _b in rows if n.startswith("dW")]
    print("  %-28s %-9s %s%s" % (tag, label, "  ".join("%s %.2e" % (n, e) for n, e, _b in rows if not n.startswith("dW")),
                                "  dW worst %.2e (%s)" % max(dw) if dw else ""), flush=True)


@pytest.fixture()
def ops():
    from speechdrivestemplates_amd import ops as o
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("tag", VALUE_TAGS)
def test_chain_sweep(ops, tag):
    c = CASE[tag]
    _threads()
    for slope, seed in ((SLOPE, SEEDS.get(tag, 0)), (1.0, OTHER_SEED)):
        d = make_data(c, seed)
        ref = chain_ref(c.spec, d, slope)
        if slope != 1.0:
            assert ref.umin >= KINK, "%s: a float64 pre-activation within %g of the kink (%.2e): take the next seed" % (tag, KINK, ref.umin)
        got = device_run(ops, c, d, slope)
        rows = errors(tag, _to_cpu(got), ref)
        _report(tag, "slope %.1f" % slope, rows)
        assert not failed(rows), (tag, slope, failed(rows))
        if slope != 1.0:
            again = device_run(ops, c, d, slope)
            assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]), "%s: a second run differs" % tag
            assert all(torch.equal(a, b) for a, b in zip(got[2], again[2])), "%s: a weight gradient differs in a second run" % tag


def _abi_forward_is_refused(ops, bl, B, T0, cin0):
    """sdt_chain1d_fwd_f32 on real buffers: SDT_ERR_ARG, no store into y / zout, counters and error word untouched"""
    from speechdrivestemplates_amd import _lib
    lib, dev = _lib.load(), torch.device(DEV, 0)
    mark = 7.0
    w = [torch.zeros(256 * b[2] * b[3], device=DEV) for b in bl]
    y = [torch.full((B * max(b[1], 1) * 256,), mark, device=DEV) for b in bl]
    x0, zout = torch.zeros(B * T0 * cin0, device=DEV), torch.full((B * max(bl[-1][1], 1) * 256,), mark, device=DEV)
    tab = (_lib.ChainLayer * len(bl))(*[_lib.ChainLayer(Ti, To, Cin, k, s, p, mode, sa, sb, 0, w[l].data_ptr(), None, y[l].data_ptr(), None, None, None)
                                       for l, (Ti, To, Cin, k, s, p, mode, sa, sb) in enumerate(bl)])
    ws = ops._chain_ws(dev)
    torch.cuda.synchronize()
    before = ws.clone()
    rc = lib.sdt_chain1d_fwd_f32(tab, len(bl), x0.data_ptr(), zout.data_ptr(), B, SLOPE, EPS, 0, ws.data_ptr(), ws.data_ptr() + 4 * ops._CHAIN_ERR,
                                 ops._stream())
    torch.cuda.synchronize()
    assert rc == -1, "SDT_ERR_ARG expected, got %d" % rc
    assert torch.equal(ws, before) and int(ws.abs().sum().item()) == 0
    assert all(bool((t == mark).all()) for t in y + [zout]), "a refused chain was launched"
    assert not lib.sdt_chain1d_supported(tab, len(bl), B)


def _is_refused(ops, T, cin0, B, spec):
    bl = blocks_of(spec, T, cin0)
    wd = [torch.nn.Parameter(ops.to_weight_layout(torch.zeros((256, b[2], b[3]), device=DEV))) for b in bl]
    assert not ops.chain1d_usable(torch.zeros((B, T, cin0), device=DEV), tuple(spec), wd)
    _abi_forward_is_refused(ops, bl, B, T, cin0)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", REFUSED_TAGS)
def test_refused_rows_are_refused_before_any_launch(ops, tag):
    c = CASE[tag]
    _is_refused(ops, c.T, c.cin0, c.B, c.spec)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", sorted(CONSUMER_RULES))
def test_consumer_rules_are_part_of_supported(ops, rule):
    """what only the backward launch's consumer tables object to is refused by chain1d_usable and by the forward entry as well"""
    T, spec = CONSUMER_RULES[rule]
    _is_refused(ops, T, 256, 2, spec)


@pytest.mark.gpu
def test_a_kernel_longer_than_the_padded_input_is_refused(ops):
    """Ti + 2 pad < k: (Ti + 2 pad - k) / stride + 1 truncates towards zero in C and called Ti = 1, (4, 2, 1) one output frame"""
    _abi_forward_is_refused(ops, [(1, 1, 256, 4, 2, 1, P, -1, -1)], 2, 1, 256)


@pytest.mark.gpu
def test_the_generators_wiring_stays_usable(ops):
    for T, cin0 in ((64, 288), (32, 288), (64, 256)):
        bl = blocks_of(generator_wiring(), T, cin0)
        wd = [torch.nn.Parameter(ops.to_weight_layout(torch.zeros((256, b[2], b[3]), device=DEV))) for b in bl]
        assert ops.chain1d_usable(torch.zeros((4, T, cin0), device=DEV), generator_wiring(), wd)


@functools.lru_cache(maxsize=None)
def _batch_data():
    return make_data(_batch_case(max(BATCHES)), 0)


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
def test_batch_windows_and_launches(ops, B):
    """the first B clips of one seeded 65-clip batch: forward against float64; clips 0, 7, 8, 31, 32, B - 1 bit-identical to their B = 1 runs"""
    _threads()
    c, full = _batch_case(B), _batch_data()
    d = Data(full.h[:B].contiguous(), full.gz[:B].contiguous(), full.ws)
    z, dh, _dws = device_run(ops, c, d, SLOPE)
    e = rel(z.double().cpu(), chain_ref(c.spec, d, SLOPE, grads=False).z)
    print("  batch-%-3d forward %.2e" % (B, e), flush=True)
    assert e <= TOL_FWD, e
    assert bool(torch.isfinite(dh).all())
    one = _batch_case(1)
    for i in sorted({i for i in (0, 7, 8, 31, 32, B - 1) if i < B}):
        zi, dhi, _w = device_run(ops, one, Data(d.h[i:i + 1].contiguous(), d.gz[i:i + 1].contiguous(), d.ws), SLOPE)
        assert torch.equal(z[i], zi[0]), "clip %d of %d: z differs from the clip's own run" % (i, B)
        assert torch.equal(dh[i], dhi[0]), "clip %d of %d: dh differs from the clip's own run" % (i, B)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", [t for t, _T, _c in BF16])
def test_bf16_products_on_one_block(ops, tag):
    """bf16-representable h and w: every product is exact, the forward keeps the fp32 bar; the input gradient's first operand (the normalisation
    backward of gz) is rounded to bf16 by the kernel, so it is held to a float64 emulation that rounds there (RNE) at 1e-4 (test_chain1d_gpu.py)"""
    c = CASE[tag]
    d = make_data(c, SEEDS.get(tag, 0), bf16=True)
    ref = chain_ref(c.spec, d, SLOPE)
    assert ref.umin >= KINK and bf16_tie_margin(c, d, ref) >= TIE, (tag, ref.umin, bf16_tie_margin(c, d, ref))
    k, s, p = c.spec[0][:3]
    dy_r = ref.dys[0].float().bfloat16().double()
    emu = ref._replace(dh=torch.nn.grad.conv1d_input((c.B, c.cin0, c.T), d.ws[0].double(), dy_r, s, p).permute(0, 2, 1).contiguous())
    ops.CHAIN_MATH = "bf16"
    try:
        got = device_run(ops, c, d, SLOPE)
        again = device_run(ops, c, d, SLOPE)
    finally:
        ops.CHAIN_MATH = None
    rows = errors(tag, _to_cpu(got), emu, dx_bar=TOL_BF16_DX)
    _report(tag, "bf16", rows)
    assert not failed(rows), (tag, failed(rows))
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]) and torch.equal(got[2][0], again[2][0])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _threads()
    if "--seeds" in sys.argv:
        print("SEEDS = {")
        for _t in SEEDED_TAGS:
            _s = first_seed(CASE[_t], _t.startswith("bf16-"))
            if _s:
                print('    "%s": %d,' % (_t, _s), flush=True)
        print("}")
    else:  # the FP32_REF_ERR entries: fp32 torch on the CPU against float64
        for _t in VALUE_TAGS:
            _rows = cpu_fp32_rows(_t)
            print("# %-28s worst fp32-vs-float64 / bar: %.3f" % (_t, max(e / b for _k, e, b in _rows)), flush=True)
            for _k, _e, _b in _rows:
                if 4.0 * _e > 0.8 * _b:
                    print('    "%s": %.2e,' % (_k, _e), flush=True)
