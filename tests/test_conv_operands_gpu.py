"""The conv operands a TRAINING step reads, and the bias-gradient sum, against exact host models.

Under optim.FlatAdam every Conv weight is registered with ops.WeightMirrors: the B operand of every input-gradient launch is the (Cin, taps, Cout)
mirror, in bf16 storage both conv operands are bf16 copies, with ops.W3_PRESPLIT they are three bf16 planes -- all written by ONE launch of
weight_transpose_batched_kernel (csrc/conv.hip) and served only while the dirty / _version bookkeeping says they are current.  The edge sweeps
(test_f32_conv_sweep_gpu.py, test_bf16_conv_sweep_gpu.py, test_reserved_conv_sweep_gpu.py) build plain, unregistered weights and never run it.
col_sum_kernel (every bias gradient, the head's 2048 x 274 included) has the same standing.

Both helpers are deterministic and their order of operations is written in their comments, so the references are EXACT -- bit patterns, no
tolerance:
  mirror      storage (Cout, taps, Cin) -> permute(2, 1, 0)
  bf16 copy   round to nearest even (`bf16_rne`: integer arithmetic on the fp32 bits; a host test holds it equal to torch's conversion)
  planes      hi = bf16(v), mid = bf16(v - hi), lo = bf16((v - hi) - mid), the differences in fp32 (`split3`)
  col sum     `col_sum_model`: thread q owns rows q (mod 16); rows r + 16 u go to acc[u] while r + 112 < rows, the tail to acc[0], acc[1], ...;
              ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7)); sixteen partials halved 8 / 4 / 2 / 1; the total is added to `out`
Comparisons are on the bit patterns (so -0 is not +0), which implies torch.equal.  The only two tolerances are stated ones of test_ops_gpu.py
(dbias 2e-5 of max, and 2e-5 forward / dX of the two ConvFn cases), against float64; COL_SUM_REF_ERR would widen the first per shape by the CPU
restatement's own error (it is empty: the restatement stays under a quarter of the bar at every shape -- test_col_sum_model_stays_below_a_quarter_of_the_bar).

`simulate_batched` restates the batched kernel workgroup by workgroup (descriptor search, rem % nci / rem % nco / rem / nco, partly filled
tiles, stores) on numpy arrays; the device results and the simulation go through the SAME assertions (`check_group`, `check_col_sum`), and the
host-only teeth tests substitute mutated simulations for the device result and require an AssertionError.

Weights: 0.1 randn with the full 24-bit mantissa, plus SPECIALS spread over every tensor: RNE ties with even and odd neighbours (and their
nearest non-ties), a tie that carries into the exponent, +-0, subnormals, the smallest normal, the largest finite bf16.  The subnormals are
bf16-representable: (p0 + p1) + p2 == w needs every remainder representable, which 2^-140 under a bf16 subnormal step of 2^-133 is not.

Registered against unregistered operands (part 2) launches the sweeps' own geometries, imported by name; the split-fp32 kernels plan only
from 256 output tiles, so those cases' activations are 8 - 10 MB (everything else in this file is under 4 MB)."""
import collections
import functools
import gc
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_bf16_conv_sweep_gpu as bsweep
import test_f32_conv_sweep_gpu as fsweep

gpu = pytest.mark.gpu
DEV = "cuda"
TOL_DBIAS = 2e-5  # test_ops_gpu.py: "dbias", relative to the largest column sum
TOL_CONV = 2e-5   # test_ops_gpu.py: "fwd" / "dX" of test_conv1d / test_conv2d


@pytest.fixture(scope="module")
def ops():
    from speechdrivestemplates_amd import ops as o
    return o


# ---------------------------------------------------------------------------------------------
# exact models
# ---------------------------------------------------------------------------------------------
def bf16_rne(v):
    """fp32 array -> bf16 bit patterns (uint16), round to nearest even, in integer arithmetic (finite inputs)"""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_trunc(v):
    return (np.ascontiguousarray(v, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_f32(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def split3(v, rnd=bf16_rne, mid_from_v=False):
    """(3, ...) uint16: the exact three-way split of csrc/conv.hip wt_store16 (= convbf.hip x3_stage)"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    hi = rnd(v)
    r = v - bf16_f32(hi)
    mid = rnd(v if mid_from_v else r)
    lo = rnd(r - bf16_f32(mid))
    return np.stack([hi, mid, lo])


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


SPECIALS = np.array([
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # ties: 1 + 2^-8 (even neighbour below: down), 1 + 3 2^-8 (odd below: up), and negative
    0x3F808001, 0x3F817FFF,                          # one ulp above / below a tie
    0x3FFF8000,                                      # tie under 2.0: rounds up into the next exponent
    0x00000000, 0x80000000,                          # +0, -0
    0x00100000, 0x80030000,                          # subnormals 2^-129 and -3 2^-133 (bf16-representable)
    0x00800000,                                      # the smallest normal
    0x7F7F0000, 0xFF7F0000,                          # +- the largest finite bf16
    0x3F800001,                                      # 1 + 2^-23: hi = 1, mid = 2^-23
], dtype=np.uint32)


def taps_of(spec):
    k = spec[2]
    return k if isinstance(k, int) else k[0] * k[1]


def is4d(spec):
    return not isinstance(spec[2], int)


def storage_values(spec, seed):
    """(Cout, taps, Cin) fp32 storage of a layer spec (cout, cin, k | (kh, kw)): full-mantissa values with SPECIALS spread from the first to the
    last element (a small tensor takes as many as it has elements, rotated by the seed)"""
    cout, cin, _k = spec
    n = cout * taps_of(spec) * cin
    v = (np.random.Generator(np.random.PCG64(seed)).standard_normal(n) * 0.1).astype(np.float32)
    pos = np.unique(np.linspace(0, n - 1, num=min(n, len(SPECIALS))).astype(np.int64))
    v[pos] = SPECIALS[(np.arange(len(pos)) + seed) % len(SPECIALS)].view(np.float32)
    return v.reshape(cout, taps_of(spec), cin)


Model = collections.namedtuple("Model", "wt w16 wt16")


def model(storage, planes):
    """what a refresh must leave for one layer: the fp32 mirror and (planes 1: bf16 copies, 3: the planes) of the storage and of the mirror"""
    wt = np.ascontiguousarray(storage.transpose(2, 1, 0))
    if planes == 0:
        return Model(wt, None, None)
    f = bf16_rne if planes == 1 else split3
    return Model(wt, f(storage), f(wt))


# ---------------------------------------------------------------------------------------------
# layer tables
# ---------------------------------------------------------------------------------------------
CH = (1, 31, 32, 33, 64, 65)
KS = ((1, 1), (1, 3), (6, 3))  # taps 1, 3, 18


def _singles():
    """every (cin, cout) pair of CH, the tap count cycling 1 / 3 / 18; all three tap counts on the pairs whose tile counts differ most"""
    out = [(co, ci, KS[(i + j) % 3]) for i, ci in enumerate(CH) for j, co in enumerate(CH)]
    out += [(co, ci, k) for (ci, co) in ((33, 65), (65, 33), (1, 65), (31, 1)) for k in KS]
    return out


SINGLES = _singles()
SINGLES_1D = [(65, 33, 3), (1, 31, 1), (32, 64, 4), (33, 1, 3)]  # Conv1d weights: 3-D tensors, never a bf16 copy
ONE = [(1, 1, (1, 1))]


def _forty():
    """~40 layers, 3-D and 4-D mixed, tile counts from 1 to 162: a one-tile layer between two large ones, one-tile layers back to back (every
    workgroup there is the first AND the last of its layer), the last layer a one-tile layer"""
    rng = np.random.Generator(np.random.PCG64(40))
    out = [(65, 65, (6, 3)), (32, 32, (1, 1)), (64, 65, (6, 3)), (1, 1, 1), (31, 1, (1, 1)), (33, 33, 3)]
    while len(out) < 39:
        co, ci = int(rng.choice(CH + (96, 100))), int(rng.choice(CH + (96, 100)))
        k = [1, 3, 4, (1, 1), (1, 3), (2, 2), (6, 3)][int(rng.integers(7))]
        if co * ci * (k if isinstance(k, int) else k[0] * k[1]) <= 40000:
            out.append((co, ci, k))
    out[20] = (17, 5, (1, 1))  # a one-tile 4-D layer in the middle of the random ones
    return out + [(32, 31, (1, 1))]


FORTY = _forty()


def tiles_of(spec):
    cout, cin, _k = spec
    return ((cin + 31) // 32) * ((cout + 31) // 32) * taps_of(spec)


# ---------------------------------------------------------------------------------------------
# destinations inside guarded buffers (host: numpy bit patterns; device: the same patterns in int tensors)
# ---------------------------------------------------------------------------------------------
GUARD = 64
PAT32, PAT16 = 0x7FC0BEEF, 0x7FC1  # NaN patterns no weight holds: guards, and the fill of every destination before the launch


def _guarded_np(n, wide):
    return np.full(n + 2 * GUARD, PAT32 if wide else PAT16, dtype=np.uint32 if wide else np.uint16)


def _guarded_dev(n, dtype):
    wide = dtype == torch.float32
    buf = torch.full((n + 2 * GUARD,), PAT32 if wide else PAT16, dtype=torch.int32 if wide else torch.int16, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(dtype)


def _to_np(buf):
    a = buf.cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.int32 else np.uint16)


def _payload(name, buf, want_bits, tag):
    """guards intact, payload == want, bit for bit"""
    n = want_bits.size
    assert buf.size == n + 2 * GUARD, "%s %s: %d elements, the model has %d" % (tag, name, buf.size - 2 * GUARD, n)
    pat = PAT32 if buf.dtype == np.uint32 else PAT16
    assert (buf[:GUARD] == pat).all() and (buf[GUARD + n:] == pat).all(), "%s %s: a guard element was written" % (tag, name)
    got = buf[GUARD:GUARD + n]
    bad = np.flatnonzero(got != want_bits.reshape(-1))
    assert bad.size == 0, "%s %s: %d of %d elements differ, first at %d: got %#x, model %#x" % (
        tag, name, bad.size, n, bad[0], int(got[bad[0]]), int(want_bits.reshape(-1)[bad[0]]))
    return got


def check_group(specs, storages, outs, planes):
    """THE assertions of part 1, for a device result or a simulated one.  outs[l] = {'wt', 'w16', 'wt16'} -> guarded buffer (bit patterns) | None"""
    assert len(outs) == len(specs)
    for l, (spec, st, o) in enumerate(zip(specs, storages, outs)):
        tag = "layer %d %r planes %d" % (l, spec, planes)
        has16 = planes != 0 and is4d(spec)
        m = model(st, planes if has16 else 0)
        _payload("wt", o["wt"], bits32(m.wt), tag)
        if not has16:
            assert o["w16"] is None and o["wt16"] is None, "%s: a 3-D weight (or fp32 mode) got bf16 copies" % tag
            continue
        for name, want, w in (("w16", m.w16, st), ("wt16", m.wt16, m.wt)):
            assert o[name] is not None, "%s: no %s" % (tag, name)
            got = _payload(name, o[name], want, tag)
            if planes == 3:  # the three planes ARE the weight: fp32 sums of bf16 numbers in this order are exact
                p = bf16_f32(got.reshape(3, -1))
                assert np.array_equal((p[0] + p[1]) + p[2], w.reshape(-1)), "%s %s: (p0 + p1) + p2 != w" % (tag, name)


# ---------------------------------------------------------------------------------------------
# the batched kernel restated on the host, one workgroup at a time, with the mutations of the teeth tests
# ---------------------------------------------------------------------------------------------
def simulate_batched(specs, storages, planes, mutation=None):
    descs, outs, tile0 = [], [], 0
    for spec, st in zip(specs, storages):
        cout, cin, _k = spec
        nel = st.size
        has16 = planes != 0 and is4d(spec)
        lead = 3 if planes == 3 else 1
        o = {"wt": _guarded_np(nel, True), "w16": _guarded_np(lead * nel, False) if has16 else None,
             "wt16": _guarded_np(lead * nel, False) if has16 else None}
        outs.append(o)
        descs.append((cout, taps_of(spec), cin, tile0, planes if has16 else 0, st, o))
        tile0 += tiles_of(spec)

    def store16(dst, idx, nel, pl, v):
        if pl == 3:
            s3 = split3(v, mid_from_v=mutation == "mid_from_v")
            for k in range(3):
                dst[GUARD + k * nel + idx] = s3[k]
        else:
            dst[GUARD + idx] = bf16_trunc(v) if mutation == "truncate" else bf16_rne(v)

    n = len(descs)
    for bid in range(tile0):
        l = 0
        while l + 1 < n and (descs[l + 1][3] < bid if mutation == "boundary" else descs[l + 1][3] <= bid):
            l += 1
        cout, taps, cin, begin, pl, st, o = descs[l]
        nci, nco = (cin + 31) >> 5, (cout + 31) >> 5
        if mutation == "swap":
            nci, nco = nco, nci
        rem = bid - begin
        ci0 = (rem % nci) * 32
        rem //= nci
        co0, t = (rem % nco) * 32, rem // nco
        if t >= taps:  # (only a mutated search / decomposition gets here; the device would be out of bounds: the tile stays unwritten)
            continue
        cin_ok = cin - 1 if (mutation == "tail" and cin % 32 == 1) else cin
        co = np.arange(co0, min(co0 + 32, cout))
        ci = np.arange(ci0, min(ci0 + 32, cin_ok))
        if co.size == 0 or ci.size == 0:
            continue
        v = st[co[:, None], t, ci[None, :]]
        if o["w16"] is not None:
            store16(o["w16"], ((co[:, None] * taps + t) * cin + ci[None, :]), st.size, pl, v)
        idx_t = (ci[:, None] * taps + t) * cout + co[None, :]
        o["wt"][GUARD + idx_t] = bits32(v.T)
        if o["wt16"] is not None:
            store16(o["wt16"], idx_t, st.size, pl, np.ascontiguousarray(v.T))
    return outs


@functools.lru_cache(maxsize=None)
def _storages(name):
    specs = {"singles": SINGLES, "singles1d": SINGLES_1D, "one": ONE, "forty": FORTY}[name]
    return specs, [storage_values(s, zlib.crc32(("%s %d" % (name, i)).encode()) & 0xffff) for i, s in enumerate(specs)]


# ---------------------------------------------------------------------------------------------
# host-only tests of the transposition models
# ---------------------------------------------------------------------------------------------
def test_transpose_models_agree():
    """The integer RNE is torch's conversion; the inputs hold what the docstring says; the workgroup-by-workgroup restatement of the kernel, the
    permute model and the issue's torch statement of it (permute / .to(bfloat16) / fp32 differences) give the same bits on every table"""
    v = np.concatenate([SPECIALS.view(np.float32), storage_values((65, 65, (6, 3)), 1).reshape(-1)])
    t = torch.from_numpy(v)
    assert np.array_equal(bf16_rne(v), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    hi = t.to(torch.bfloat16)
    r = t - hi.float()
    mid = r.to(torch.bfloat16)
    lo = (r - mid.float()).to(torch.bfloat16)
    assert np.array_equal(split3(v), torch.stack([hi, mid, lo]).view(torch.int16).numpy().view(np.uint16))
    # ties round to even, in both directions
    assert [int(x) for x in bf16_rne(SPECIALS[:7].view(np.float32))] == [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F81, 0x4000]
    assert bf16_rne(np.array([-0.0], np.float32))[0] == 0x8000 and split3(np.array([-0.0], np.float32))[:, 0].tolist() == [0x8000, 0, 0]
    low = bits32(v[len(SPECIALS):]) & 0xFFFF
    assert (low != 0).mean() > 0.99 and ((low & 0xFF) != 0).mean() > 0.95  # full mantissas: the mid and low planes carry data
    tiles = [tiles_of(s) for s in FORTY]
    assert len(FORTY) == 40 and tiles[1] == 1 and min(tiles[0], tiles[2]) >= 100 and tiles[-1] == 1 and tiles[3] == tiles[4] == 1
    assert any(is4d(s) for s in FORTY) and any(not is4d(s) for s in FORTY) and len(set(tiles)) >= 8
    assert {taps_of(s) for s in SINGLES} == {1, 3, 18} and {(s[1], s[0]) for s in SINGLES} >= {(a, b) for a in CH for b in CH}
    for name in ("one", "singles1d", "forty"):
        specs, sts = _storages(name)
        for planes in (0, 1, 3):
            check_group(specs, sts, simulate_batched(specs, sts, planes), planes)
    specs, sts = _storages("singles")
    for i in range(0, len(specs), 5):
        check_group(specs[i:i + 1], sts[i:i + 1], simulate_batched(specs[i:i + 1], sts[i:i + 1], 3), 3)


@pytest.mark.parametrize("mutation,planes", [("boundary", 0), ("swap", 0), ("tail", 0), ("truncate", 1), ("mid_from_v", 3)])
def test_transpose_teeth(mutation, planes):
    """A layer boundary off by one tile, nci and nco swapped, the tail column dropped when cin % 32 = 1, truncation for RNE, mid taken from v:
    each one, substituted for the device result, fails check_group -- on the 40-layer table, and the last four on a single layer as well"""
    specs, sts = _storages("forty")
    with pytest.raises(AssertionError):
        check_group(specs, sts, simulate_batched(specs, sts, planes, mutation), planes)
    if mutation != "boundary":  # (one layer has no boundary)
        spec = (65, 33, (1, 3))
        st = [storage_values(spec, 5)]
        check_group([spec], st, simulate_batched([spec], st, planes), planes)
        with pytest.raises(AssertionError):
            check_group([spec], st, simulate_batched([spec], st, planes, mutation), planes)


# ---------------------------------------------------------------------------------------------
# part 1 on the device
# ---------------------------------------------------------------------------------------------
def make_param(storage):
    """a Parameter in the kernel layout (logical (Cout, Cin, kh, kw) | (Cout, Cin, k) over (Cout, taps, Cin) memory) from (storage, spec)"""
    st, spec = storage
    cout, cin, k = spec
    s = torch.from_numpy(st).to(DEV)
    w = s.view(cout, k[0], k[1], cin).permute(0, 3, 1, 2) if is4d(spec) else s.view(cout, k, cin).permute(0, 2, 1)
    return torch.nn.Parameter(w)


class modes:
    """ops.STORAGE / F32_SPLIT / W3_PRESPLIT for one block, restored on exit (and the plan caches dropped, as the sweeps' `routed` fixture does)"""

    def __init__(self, ops, storage="f32", split=True, w3=False):
        self.ops, self.want = ops, (storage, split, w3)

    def __enter__(self):
        o = self.ops
        self.prev = (o.STORAGE, o.F32_SPLIT, o.W3_PRESPLIT)
        o.STORAGE, o.F32_SPLIT, o.W3_PRESPLIT = self.want
        return o

    def __exit__(self, *exc):
        o = self.ops
        o.STORAGE, o.F32_SPLIT, o.W3_PRESPLIT = self.prev
        o.clear_plans()


def plane_mode(ops, planes):
    return modes(ops, storage="bf16" if planes == 1 else "f32", split=True, w3=planes == 3)


def _poison(nbytes):
    """a NaN-filled allocation made and freed: what the group allocates next cannot hide an unwritten element behind stale zeros"""
    t = torch.full((max(nbytes // 4, 1),), float("nan"), device=DEV)
    del t


def _reseat(group):
    """moves every destination of a group into a guarded, pattern-filled buffer and rebuilds the descriptor table; -> the buffers per layer"""
    bufs = []
    for e in group.entries:
        row = {}
        for k, name in ((1, "wt"), (3, "w16"), (4, "wt16")):
            row[name] = None
            if e[k] is not None:
                row[name], pay = _guarded_dev(e[k].numel(), e[k].dtype)
                if k == 1:  # (lookup3 finds a mirror's planes by the mirror's address)
                    type(group)._by_mirror[pay.data_ptr()] = type(group)._by_mirror.pop(e[k].data_ptr())
                e[k] = pay.view(e[k].shape)
        bufs.append(row)
    group._build_table()
    group.dirty = True
    return bufs


def run_group(ops, specs, storages, planes):
    """one WeightMirrors group over the layers, one batched launch, -> outs for check_group"""
    _poison(sum(s.size for s in storages) * 4 * 3)
    params = [make_param(x) for x in zip(storages, specs)]
    for p, st in zip(params, storages):
        assert ops.weight_storage(p).data_ptr() == p.data_ptr() and tuple(ops.weight_storage(p).shape) == st.shape
    group = ops.WeightMirrors(params)
    assert len(group.entries) == len(specs) and group.total_tiles == sum(tiles_of(s) for s in specs)
    assert [e[5] for e in group.entries] == [sum(tiles_of(s) for s in specs[:i]) for i in range(len(specs))]
    if planes:
        assert group.planes == planes
    for e, spec in zip(group.entries, specs):
        assert (e[3] is not None) == (e[4] is not None) == (planes != 0 and is4d(spec)), (spec, planes)
    bufs = _reseat(group)
    group.refresh()
    torch.cuda.synchronize()
    assert not group.dirty
    for p, st in zip(params, storages):  # the launch only reads the weights
        assert np.array_equal(bits32(ops.weight_storage(p.detach()).cpu().numpy()), bits32(st))
    return [{k: None if b is None else _to_np(b) for k, b in row.items()} for row in bufs]


@gpu
@pytest.mark.parametrize("planes", [0, 1, 3])
def test_batched_transpose_single_layers(ops, planes):
    """one layer per launch: cin, cout in {1, 31, 32, 33, 64, 65} x taps 1 / 3 / 18, the 1 x 1 x 1 weight, Conv1d weights (no copies in any mode)"""
    with plane_mode(ops, planes):
        for name in ("one", "singles", "singles1d"):
            specs, sts = _storages(name)
            for spec, st in zip(specs, sts):
                check_group([spec], [st], run_group(ops, [spec], [st], planes), planes)


@gpu
@pytest.mark.parametrize("planes", [0, 1, 3])
def test_batched_transpose_forty_layers(ops, planes):
    """the 40-layer table in ONE launch: tile_begin boundaries on the first and the last workgroup of a layer, one-tile layers between large
    ones and at the end, 3-D weights (descriptor planes 0, null w16) among 4-D ones with copies / planes"""
    with plane_mode(ops, planes):
        specs, sts = _storages("forty")
        check_group(specs, sts, run_group(ops, specs, sts, planes), planes)


@gpu
def test_per_call_transpose(ops):
    """sdt_weight_transpose_f32 -- what conv_input_grad launches for a weight no group has registered -- on the same shapes, same model"""
    from speechdrivestemplates_amd import _lib
    lib = _lib.load()
    for name in ("one", "singles", "singles1d"):
        for spec, st in zip(*_storages(name)):
            _poison(st.size * 8)
            w = make_param((st, spec))
            assert ops.WeightMirrors.lookup(w) is None
            ws = ops.weight_storage(w.detach())
            buf, wt = _guarded_dev(st.size, torch.float32)
            _lib.check(lib.sdt_weight_transpose_f32(ws.data_ptr(), wt.data_ptr(), st.shape[0], st.shape[1], st.shape[2], ops._stream()))
            torch.cuda.synchronize()
            _payload("wt", _to_np(buf), bits32(model(st, 0).wt), "per-call %r" % (spec,))


# ---------------------------------------------------------------------------------------------
# part 2: registered and unregistered operands give the same bits
# ---------------------------------------------------------------------------------------------
# Sweep geometries by name (fsweep.CASE / bsweep.CASE); what serves them is in the sweeps' EXPECT tables (`--plans`), asserted below.
#   fp32 split   forward: convbf2<float,128,128> (k4s2p1-even), convbf2<float,256,64> (cap-c320), convsk<128,128> (dw-128x128), convsk<128,64>
#                (dw-64x64), sdt_conv_taps_f32 (cin3, stat-dx-32), split-K (k3s2p1-small, cin48, no-pack-k2s3)
#                dX: convbf2<float,256,64> x4 (k4s2p1-even, stride 2), convbf2<float,128,128> x4 (stat-dx-32, stride 2), convsk<128,128> x1
#                (dw-128x128), sdt_conv_taps_multi_f32 x1 / x4 (cin3: Cin = 3; cin48: Cin = 48, stride 2, four classes), per-class split-K (no-pack-k2s3)
#   fp32 MFMA    the same geometries under F32_SPLIT = False (convsk forward, multi / convsk dX)
#   bf16         forward / dX: convbf2<128,128> / convbf2<256,64> x4 (k4s2p1-even), convsk<128,128> / convsk<128,64> x4 (k3s2p1, stride 2),
#                convsk<128,128> both (dw-128x128), convsk<128,64> both (dw-64x64), a one-row tail (tile-plus-one), and the planner's refusal
#                (k3s2p1-small: no bf16 forward; the dX falls back to the fp32 kernels and reads the fp32 mirror of a group with bf16 copies)
F32_TAGS = ("k4s2p1-even", "cap-c320", "stat-dx-32", "dw-128x128", "dw-64x64", "k3s2p1-small", "cin3", "cin48", "no-pack-k2s3")
BF16_TAGS = ("k4s2p1-even", "k3s2p1", "dw-128x128", "dw-64x64", "tile-plus-one", "k3s2p1-small")
SETTINGS = {"split": dict(storage="f32", split=True, w3=False), "split-w3": dict(storage="f32", split=True, w3=True),
            "mfma": dict(storage="f32", split=False, w3=False), "bf16": dict(storage="bf16", split=True, w3=False)}
PAIRS = [(t, s) for s in ("split", "split-w3", "mfma") for t in F32_TAGS] + [(t, "bf16") for t in BF16_TAGS]


def test_operand_cases_cover_the_kernel_families():
    """read off the sweeps' own tables (no planner, no GPU): one case per forward and per dX family a registered weight can reach"""
    E = [fsweep.EXPECT[t] for t in F32_TAGS]
    assert {e.fwd.split(" k=")[0] for e in E} >= {"convbf2_kernel<float, 128, 128>", "convbf2_kernel<float, 256, 64>", "convsk_kernel<128, 128>",
                                                 "convsk_kernel<128, 64>", "sdt_conv_taps_f32", "sdt_conv_taps_splitk_f32"}
    dx = {e.dx.split(" k=")[0] for e in E}
    assert dx >= {"convbf2_kernel<float, 256, 64> x4", "convbf2_kernel<float, 128, 128> x4", "convsk_kernel<128, 128> x1", "sdt_conv_taps_multi_f32 x1",
                  "sdt_conv_taps_multi_f32 x4", "sdt_conv_taps_splitk_f32 per class (4 of 9)"}
    M = [fsweep.EXPECT_MFMA[t] for t in F32_TAGS if t in fsweep.EXPECT_MFMA]
    assert {e.fwd for e in M} >= {"convsk_kernel<128, 128>", "convsk_kernel<128, 64>"} and any(e.dx.startswith("convsk_kernel") for e in M)
    Bf = [bsweep.EXPECT[t] for t in BF16_TAGS]
    assert {e.fwd for e in Bf} >= {"convbf2_kernel<128, 128>", "convsk_kernel<128, 128>", "convsk_kernel<128, 64>", None}
    assert {e.dx for e in Bf} >= {"convbf2_kernel<256, 64> x4", "convsk_kernel<128, 64> x4", "convsk_kernel<128, 128> x1", "convsk_kernel<128, 64> x1", None}
    cases = [fsweep.CASE[t] for t in F32_TAGS]
    assert any(c[8] == 2 and c[4] % 32 for c in cases) and any(c[8] == 1 and c[4] % 32 for c in cases)  # Cin = 48 under stride 2, Cin = 3
    assert sum(c[8] == 2 for c in cases) >= 3


def _operands(c):
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = bsweep.dims(c)
    g = torch.Generator().manual_seed(zlib.crc32(("operands " + c[0]).encode()))
    x = torch.randn(B, Hi, Wi, Cin, generator=g)
    st = (torch.randn(Cout, kh * kw, Cin, generator=g) * (2.0 / (Cin * kh * kw)) ** 0.5).numpy()
    gy = torch.randn(B, Ho, Wo, Cout, generator=g)
    return x, st, gy


def _launch_pair(ops, c, w, x, gy):
    """(y | None, dx) through the public entry points; bf16 tensors: ConvStatsFn where a bf16 forward launch exists, as the bf16 sweep runs it"""
    B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = bsweep.dims(c)
    if x.dtype == torch.bfloat16:
        y = None
        for _mode, groups in bsweep.fwd_modes(c)[:1]:
            if ops.conv_stats_fusable(x, w, s, p, groups):
                with torch.no_grad():
                    y = ops.ConvStatsFn.apply(x, w, s, p, groups, None)[0]
    else:
        y = ops.conv_forward(x, w, None, s, p)
    dx = ops.conv_input_grad(gy, w, (B, Hi, Wi, Cin), s, p)
    torch.cuda.synchronize()
    return y, dx


@gpu
@pytest.mark.parametrize("tag,setting", PAIRS, ids=["%s %s" % p for p in PAIRS])
def test_registered_operands_give_the_same_bits(ops, tag, setting):
    """conv_forward and conv_input_grad on a weight no group knows (per-call transposition / conversion / in-loader split) and on the same weight
    inside a WeightMirrors group (mirror / bf16 copies / planes from the batched launch): transposition and conversions are exact, so the
    results are BIT-identical -- derived, not measured"""
    bf = setting == "bf16"
    c = (bsweep if bf else fsweep).CASE[tag]
    spec = (c[5], c[4], (c[6], c[7]))
    x, st, gy = _operands(c)
    dev = torch.device(DEV, torch.cuda.current_device())
    with modes(ops, **SETTINGS[setting]):
        if bf:
            got, want = bsweep.served(ops, c, dev), bsweep.EXPECT[tag]
        else:
            got, want = fsweep.served(ops, c, dev), (fsweep.EXPECT_MFMA.get(tag) if setting == "mfma" else fsweep.EXPECT[tag])
        assert want is None or (got.fwd, got.dx) == (want.fwd, want.dx), "%s %s: served by %r, the sweep's table says %r" % (tag, setting, got, want)
        xd, gyd = (t.to(DEV).to(torch.bfloat16) if bf else t.to(DEV) for t in (x, gy))
        w = make_param((st, spec))
        assert ops.WeightMirrors.lookup(w) is None and ops.WeightMirrors.lookup16(w) is None
        y0, dx0 = _launch_pair(ops, c, w, xd, gyd)
        _poison(st.size * 4 * 4)
        group = ops.WeightMirrors([w])
        assert group.dirty
        y1, dx1 = _launch_pair(ops, c, w, xd, gyd)
        assert not group.dirty and ops.WeightMirrors.lookup(w) is group.entries[0][1]
        if setting == "split-w3":
            assert group.planes == 3 and ops.WeightMirrors.lookup3(ops.weight_storage(w)) is group.entries[0][3]
            assert ops.WeightMirrors.lookup3(group.entries[0][1]) is group.entries[0][4]
        if bf:
            assert group.planes == 1 and ops.WeightMirrors.lookup16(w)[1] is group.entries[0][4]
            assert (y0 is None) == (want.fwd is None) and dx0.dtype == (torch.float32 if want.dx is None else torch.bfloat16)
        assert not ops.streamk_error_codes()
        assert dx0.dtype == dx1.dtype and torch.isfinite(dx0.float()).all() and float(dx0.float().abs().max()) > 0
        assert torch.equal(dx1, dx0), "%s %s: dX differs between the registered and the unregistered weight" % (tag, setting)
        if y0 is not None:
            assert torch.isfinite(y0.float()).all() and torch.equal(y1, y0), "%s %s: forward differs" % (tag, setting)
        # and what the group serves is the exact model of part 1
        assert_served_exact(ops, [w], 3 if setting == "split-w3" else 1 if bf else 0)


# ---------------------------------------------------------------------------------------------
# part 3: currency of the mirrors
# ---------------------------------------------------------------------------------------------
def _bits_dev(t):
    a = t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.int32 else np.uint16)


def assert_served_exact(ops, params, planes, served=None):
    """Every conv weight of ``params``: what WeightMirrors serves NOW (lookup / lookup16 / lookup3; or ``served(p)`` -> (wt, w16, wt16) read
    without a lookup) equals the exact model of the weight's CURRENT values, bit for bit"""
    for i, p in enumerate(params):
        if p.dim() not in (3, 4):
            assert ops.WeightMirrors.lookup(p) is None
            continue
        if served is not None:
            wt, w16, wt16 = served(p)
        else:
            wt = ops.WeightMirrors.lookup(p)
            w16 = wt16 = None
            if p.dim() == 4 and planes == 1:
                w16, wt16 = ops.WeightMirrors.lookup16(p)
            elif p.dim() == 4 and planes == 3:
                w16, wt16 = ops.WeightMirrors.lookup3(ops.weight_storage(p)), ops.WeightMirrors.lookup3(wt)
            elif planes == 1:
                assert ops.WeightMirrors.lookup16(p) is None  # Conv1d weights have no bf16 copies
        torch.cuda.synchronize()
        st = ops.weight_storage(p.detach()).cpu().numpy()
        m = model(st, planes if p.dim() == 4 else 0)
        assert wt is not None and np.array_equal(_bits_dev(wt), bits32(m.wt)), "parameter %d: the fp32 mirror is not the current weight" % i
        for name, got, want in (("w16", w16, m.w16), ("wt16", wt16, m.wt16)):
            assert (got is None) == (want is None), (i, name)
            if want is not None:
                assert tuple(got.shape) == want.shape and np.array_equal(_bits_dev(got), want), "parameter %d: %s is not current" % (i, name)


CURRENCY_SHAPES = [(64, 32, (3, 3)), (40, 36, 3), (17, 65, (1, 3)), (33, 31, 4)]


def tame(st):
    """the +-3.4e38 specials replaced by 0.25: for weights that an optimiser scales, or whose products are compared with float64"""
    return np.where(np.abs(st) < 4.0, st, np.float32(0.25)).astype(np.float32)


def _currency_params(seed, with_bias=True):
    ps = [make_param((tame(storage_values(s, seed + i)), s)) for i, s in enumerate(CURRENCY_SHAPES)]
    if with_bias:
        ps.insert(2, torch.nn.Parameter(torch.randn(33, generator=torch.Generator().manual_seed(seed)).to(DEV)))  # a true 1-D tensor: never registered
    return ps


def _fill_grads(params, seed):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad.copy_(torch.randn(p.shape, generator=g).to(DEV))


def _count_refreshes(group):
    n, inner = [0], group.refresh

    def counted():
        n[0] += 1
        inner()
    group.refresh = counted
    return n


@gpu
@pytest.mark.parametrize("planes", [0, 1, 3])
def test_mirrors_are_current_after_every_event(ops, planes):
    """a real FlatAdam over 4-D, 3-D and 1-D tensors: a step, two steps with one lookup, an in-place edit of one member (the whole group
    refreshes), load_state_dict (module and optimiser), a write through .data (the documented exception) followed by mark_dirty"""
    from speechdrivestemplates_amd.optim import FlatAdam
    with plane_mode(ops, planes):
        ps = _currency_params(100)
        opt = FlatAdam(ps, lr=1e-2)  # a stale operand is off by ~lr: far from bit-equal
        group = opt.mirrors
        conv = [p for p in ps if p.dim() in (3, 4)]
        assert len(group.entries) == len(conv) == 4 and (planes == 0 or group.planes == planes)
        n = _count_refreshes(group)
        assert_served_exact(ops, ps, planes)
        assert n[0] == 1 and not group.dirty  # one launch served every lookup
        before = [p.detach().clone() for p in conv]
        _fill_grads(ps, 1)
        opt.step()
        assert group.dirty and all(not torch.equal(a, p.detach()) for a, p in zip(before, conv))
        assert_served_exact(ops, ps, planes)
        assert n[0] == 2
        for seed in (2, 3):  # two steps, a lookup only after the second
            _fill_grads(ps, seed)
            opt.step()
        assert_served_exact(ops, ps, planes)
        assert n[0] == 3
        # .data write to member 0 (not detected, by contract), then a torch-level in-place edit of member 1: the lookup of member 1 refreshes
        # the WHOLE group, so member 0's operands -- read without a lookup -- hold the .data write as well
        conv[0].data.mul_(1.25)
        assert not group.dirty and group.entries[0][2] == conv[0]._version
        with torch.no_grad():
            conv[1].mul_(0.75)
        assert ops.WeightMirrors.lookup(conv[1]) is not None and n[0] == 4
        ent = {e[0].data_ptr(): e for e in group.entries}
        assert_served_exact(ops, conv, planes, served=lambda p: (ent[p.data_ptr()][1], ent[p.data_ptr()][3], ent[p.data_ptr()][4]))
        # the exception itself: a .data write alone leaves the operands as they were; mark_dirty restores exactness
        conv[2].data.add_(0.5)
        assert ops.WeightMirrors.lookup(conv[2]) is not None and n[0] == 4
        group.mark_dirty()
        assert_served_exact(ops, ps, planes)
        assert n[0] == 5
        # load_state_dict of the module: copy_ into every parameter (version counters)
        holder = torch.nn.ParameterList(ps)
        g = torch.Generator().manual_seed(9)
        holder.load_state_dict({k: torch.randn(v.shape, generator=g) * 0.1 for k, v in holder.state_dict().items()})
        assert not group.dirty
        assert_served_exact(ops, ps, planes)
        assert n[0] == 6
        # ... and of the optimiser (moments only: the weights and their operands stand), then a step from the loaded state
        opt.load_state_dict(opt.state_dict())
        assert_served_exact(ops, ps, planes)
        assert n[0] == 6
        _fill_grads(ps, 4)
        opt.step()
        assert_served_exact(ops, ps, planes)
        assert n[0] == 7


@gpu
def test_two_groups_do_not_disturb_each_other(ops):
    """G and D: a step of one neither dirties nor refreshes the other, and both serve current values afterwards"""
    from speechdrivestemplates_amd.optim import FlatAdam
    with plane_mode(ops, 0):
        pg, pd = _currency_params(200), _currency_params(300, with_bias=False)
        og, od = FlatAdam(pg, lr=1e-2), FlatAdam(pd, lr=1e-2)
        ng, nd = _count_refreshes(og.mirrors), _count_refreshes(od.mirrors)
        assert_served_exact(ops, pg, 0)
        assert_served_exact(ops, pd, 0)
        assert (ng[0], nd[0]) == (1, 1)
        _fill_grads(pg, 1)
        og.step()
        assert og.mirrors.dirty and not od.mirrors.dirty
        assert_served_exact(ops, pd, 0)
        assert (ng[0], nd[0]) == (1, 1)  # D's lookups launched nothing, G's mirrors are still stale and nobody asked for them
        assert_served_exact(ops, pg, 0)
        assert (ng[0], nd[0]) == (2, 1)
        _fill_grads(pd, 2)
        od.step()
        assert od.mirrors.dirty and not og.mirrors.dirty
        assert_served_exact(ops, pg, 0)
        assert_served_exact(ops, pd, 0)
        assert (ng[0], nd[0]) == (2, 2)


@gpu
def test_storage_switched_after_the_group_was_built(ops):
    """ops.STORAGE = 'bf16' on a group built in fp32 storage: outside a capture the copies are allocated and exact; inside a capture lookup16
    raises the documented error and lookup3 returns None, BEFORE anything is allocated or launched (asserted on the host: entries, mode and
    refresh count unchanged)"""
    with plane_mode(ops, 0):
        ps = _currency_params(400)
        group = ops.WeightMirrors(ps)
        conv4 = [p for p in ps if p.dim() == 4]
        assert all(e[3] is None and e[4] is None for e in group.entries)
        assert_served_exact(ops, ps, 0)
        n = _count_refreshes(group)
        marker = torch.zeros(4, device=DEV)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):  # a single branch on a stream of the test's own; never replayed
            marker.add_(1.0)
            assert torch.cuda.is_current_stream_capturing()
            ops.STORAGE = "bf16"
            with pytest.raises(RuntimeError, match="bf16 weight copies must exist before a hipGraph capture"):
                ops.WeightMirrors.lookup16(conv4[0])
            ops.STORAGE, ops.W3_PRESPLIT = "f32", True
            assert ops.WeightMirrors.lookup3(ops.weight_storage(conv4[0])) is None
            assert ops.WeightMirrors.lookup3(group.entries[0][1]) is None
            ops.W3_PRESPLIT = False
            assert ops.WeightMirrors.lookup(conv4[0]) is group.entries[0][1]  # the current fp32 mirror is served inside a capture, no launch
        torch.cuda.synchronize()
        assert n[0] == 0 and not group.dirty and group.planes == 1 and all(e[3] is None and e[4] is None for e in group.entries)
        assert float(marker.sum()) == 0.0  # (a capture runs nothing)
        ops.STORAGE = "bf16"
        assert_served_exact(ops, ps, 1)
        assert n[0] == 1 and all((e[3] is not None) == (e[0].dim() == 4) for e in group.entries)
        ops.STORAGE, ops.W3_PRESPLIT = "f32", True  # ... and on to the three planes: the copies are replaced, one more launch
        assert_served_exact(ops, ps, 3)
        assert n[0] == 2 and group.planes == 3 and tuple(group.entries[0][3].shape)[0] == 3


@gpu
def test_a_dropped_optimiser_serves_nothing(ops):
    """the entries of a dead group leave _by_ptr as they are met; a new weight ON THE SAME ADDRESS (a view of the surviving storage, another
    shape and the same shape) is not served the dead group's mirror, and a fresh group on it serves an exact one"""
    from speechdrivestemplates_amd.optim import FlatAdam
    with plane_mode(ops, 0):
        ps = _currency_params(500)
        opt = FlatAdam(ps, lr=1e-2)
        conv = [p for p in ps if p.dim() in (3, 4)]
        assert_served_exact(ops, ps, 0)
        ptrs = [p.data_ptr() for p in conv]
        assert all(q in ops.WeightMirrors._by_ptr for q in ptrs)
        dead_mirror = opt.mirrors.entries[0][1]
        del opt
        gc.collect()
        with torch.no_grad():
            conv[0].mul_(2.0)
        same_shape = torch.nn.Parameter(conv[0].detach())  # same address, same shape, current values 2 x what the dead mirror holds
        other_shape = torch.nn.Parameter(ops.weight_storage(conv[0].detach()).view(-1)[:9 * 8 * 4].view(8, 9, 4).permute(0, 2, 1))
        assert same_shape.data_ptr() == other_shape.data_ptr() == ptrs[0]
        for w in (same_shape, other_shape):
            assert ops.WeightMirrors.lookup(w) is None and ops.WeightMirrors.lookup16(w) is None
        for p in conv:
            assert ops.WeightMirrors.lookup(p) is None
        assert not any(q in ops.WeightMirrors._by_ptr for q in ptrs)
        x = torch.randn(2, 5, 7, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
        gy = torch.randn(2, 5, 7, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
        dx_plain = ops.conv_input_grad(gy, same_shape, x.shape, 1, 1)  # per-call transposition of the CURRENT values
        group = ops.WeightMirrors([same_shape])
        assert ops.WeightMirrors.lookup(same_shape) is group.entries[0][1] and group.entries[0][1] is not dead_mirror
        assert_served_exact(ops, [same_shape], 0)
        assert torch.equal(ops.conv_input_grad(gy, same_shape, x.shape, 1, 1), dx_plain)
        assert ops.WeightMirrors.lookup(other_shape) is None  # a live group, the same address, another shape


@gpu
def test_a_dead_groups_weight_address_does_not_hide_a_live_mirror(ops):
    """Found by this file: a dead group's key in _by_ptr that nobody has looked up since, and a LIVE group's fp32 mirror on that address (what
    the caching allocator does by itself once the dead group's weight is freed; here the mirror is put there): lookup3 of the mirror met the
    stale key first and answered None, so the input gradient silently split in its loader.  It must serve the live group's planes."""
    import weakref
    with plane_mode(ops, 3):
        spec = (64, 32, (3, 3))
        wa = make_param((tame(storage_values(spec, 1)), spec))
        ga = ops.WeightMirrors([wa])
        ptr = wa.data_ptr()
        del ga
        gc.collect()
        assert ptr in ops.WeightMirrors._by_ptr and ops.WeightMirrors._by_ptr[ptr][0]() is None
        wb = make_param((tame(storage_values(spec, 2)), spec))
        gb = ops.WeightMirrors([wb])
        e = gb.entries[0]
        ops.WeightMirrors._by_mirror.pop(e[1].data_ptr())
        e[1] = ops.weight_storage(wa.detach()).view(e[1].shape)  # same size: the mirror of wb now lives where wa does
        ops.WeightMirrors._by_mirror[ptr] = (weakref.ref(gb), 0)
        gb._build_table()
        gb.dirty = True
        assert e[1].data_ptr() == ptr
        assert ops.WeightMirrors.lookup3(e[1]) is e[4] and e[4] is not None
        assert ptr not in ops.WeightMirrors._by_ptr
        assert_served_exact(ops, [wb], 3)


@gpu
def test_cpu_tensors_are_refused_before_any_launch(ops):
    w = make_param((storage_values((32, 32, (3, 3)), 1), (32, 32, (3, 3))))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.conv_forward(torch.zeros(1, 4, 4, 32), w, None, 1, 1)


# ---------------------------------------------------------------------------------------------
# part 4: col_sum_kernel
# ---------------------------------------------------------------------------------------------
ROWS = (1, 15, 16, 17, 112, 113, 127, 128, 129, 240, 256 + 113, 2048)
COLS = (1, 15, 16, 17, 274)
RHO = 64.0


def col_sum_model(x, out0, mutation=None):
    """csrc/conv.hip col_sum_kernel in numpy float32, in the kernel's order; -> (out after one call, out after a second call)"""
    assert x.dtype == np.float32 and out0.dtype == np.float32
    rows, C = x.shape
    part = np.zeros((16, C), np.float32)
    for q in range(16):
        acc = np.zeros((8, C), np.float32)
        r, trips = q, 0
        while r + 112 < rows:
            acc += x[r:r + 128:16]  # rows r + 16 u -> acc[u], u = 0..7
            r += 128
            trips += 1
        if mutation == "double_at_trip" and trips:
            r -= 16  # the tail starts on the last row of the unrolled trip
        tail = list(range(r, rows, 16))
        if mutation == "drop_last_tail":
            tail = tail[:-1]
        for u, rr in enumerate(tail):
            acc[u] += x[rr]
        part[q] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))
    for w in (8, 4, 2, 1):
        part[:w] += part[w:2 * w]
    total = part[0]
    outs, out = [], out0
    for _call in range(2):
        new = total.copy() if mutation == "assign" else out + total
        if mutation == "skip_last_workgroup" and C % 16:
            new[C // 16 * 16:] = out[C // 16 * 16:]
        outs.append(new)
        out = new
    return outs


@functools.lru_cache(maxsize=None)
def col_sum_case(rows, C):
    """x with a per-column mean of +-RHO standard deviations (a dropped or doubled row moves a sum by mean / (rows * mean): far above the bar),
    a random previous content of `out`, the float64 column sums and the model's results -- computed once, shared, never modified"""
    g = np.random.Generator(np.random.PCG64(zlib.crc32(b"col sum %d %d" % (rows, C))))
    sign = np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    x = (sign * RHO + g.standard_normal((rows, C))).astype(np.float32)
    out0 = g.standard_normal(C).astype(np.float32)
    sums = x.astype(np.float64).sum(0)
    zero = np.zeros(C, np.float32)
    case = dict(x=x, out0=out0, sums=sums, filled=col_sum_model(x, out0), zeros=col_sum_model(x, zero))
    for v in case.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    return case


# 4 x (the restatement's error against float64) where that exceeds the bar; measured on the CPU by
# test_col_sum_model_stays_below_a_quarter_of_the_bar.  Empty: the worst shape reaches 2.4e-7, 0.012 of the bar.
COL_SUM_REF_ERR = {}


def _rel(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def check_col_sum(rows, C, got):
    """THE assertions of part 4, for a device result or a mutated model.  got = {'filled': [out after call 1, call 2], 'zeros': [...]}: fp32
    arrays of C + 2 GUARD elements (guards: NaN pattern)"""
    case = col_sum_case(rows, C)
    tol, worst = max(TOL_DBIAS, 4.0 * COL_SUM_REF_ERR.get((rows, C), 0.0)), 0.0
    for mode, prev in (("filled", case["out0"]), ("zeros", np.zeros(C, np.float32))):
        for call in (0, 1):
            tag = "rows %d C %d out %s call %d" % (rows, C, mode, call + 1)
            buf = got[mode][call]
            assert buf.size == C + 2 * GUARD and (bits32(buf[:GUARD]) == PAT32).all() and (bits32(buf[GUARD + C:]) == PAT32).all(), tag + ": guard written"
            out = buf[GUARD:GUARD + C]
            assert np.isfinite(out).all(), tag
            e = _rel(out, prev.astype(np.float64) + (call + 1) * case["sums"])
            assert e < tol, "%s: %.3e of max against float64 (bar %.1e)" % (tag, e, tol)
            worst = max(worst, e)
            bad = np.flatnonzero(bits32(out) != bits32(case[mode][call]))
            assert bad.size == 0, "%s: %d columns differ from the restatement, first %d: %r vs %r" % (tag, bad.size, bad[0], out[bad[0]], case[mode][call][bad[0]])
    return worst


def _guarded_out(values):
    buf = np.full(values.size + 2 * GUARD, PAT32, np.uint32).view(np.float32)
    buf[GUARD:GUARD + values.size] = values
    return buf


def _as_result(rows, C, mutation=None):
    case = col_sum_case(rows, C)
    return {"filled": [_guarded_out(o) for o in col_sum_model(case["x"], case["out0"], mutation)],
            "zeros": [_guarded_out(o) for o in col_sum_model(case["x"], np.zeros(C, np.float32), mutation)]}


def test_col_sum_model_stays_below_a_quarter_of_the_bar():
    """the restatement itself against float64 at every shape (no entry of COL_SUM_REF_ERR is needed), and through check_col_sum"""
    worst = 0.0
    for rows in ROWS:
        for C in COLS:
            case = col_sum_case(rows, C)
            for mode, prev in (("filled", case["out0"]), ("zeros", np.zeros(C, np.float32))):
                for call in (0, 1):
                    e = _rel(case[mode][call], prev.astype(np.float64) + (call + 1) * case["sums"])
                    worst = max(worst, e)
                    assert e <= 0.25 * TOL_DBIAS or e <= COL_SUM_REF_ERR.get((rows, C), 0.0), (rows, C, mode, call, e)
            check_col_sum(rows, C, _as_result(rows, C))
    print("  col_sum restatement against float64: worst %.2e of max (bar %.1e)" % (worst, TOL_DBIAS))
    # the restatement is a sum: against a plain float64 sum of a tiny integer case it is exact
    x = np.arange(1, 1 + 369 * 3, dtype=np.float32).reshape(369, 3)
    assert np.array_equal(col_sum_model(x, np.ones(3, np.float32))[0], 1 + x.astype(np.float64).sum(0))


@pytest.mark.parametrize("mutation,shapes", [
    ("drop_last_tail", [(17, 16), (113, 1), (256 + 113, 274)]), ("double_at_trip", [(129, 17), (256 + 113, 274), (240, 15)]),
    ("assign", [(1, 1), (2048, 274)]), ("skip_last_workgroup", [(16, 1), (128, 17), (2048, 274)])])
def test_col_sum_teeth(mutation, shapes):
    """a dropped last tail row, a row counted twice at the 128-row boundary, `=` for `+=`, the partly filled last workgroup skipped: each fails
    check_col_sum at every listed shape -- the first two the FLOAT64 BAR itself (rho = 64), not only the bit comparison"""
    for rows, C in shapes:
        with pytest.raises(AssertionError) as err:
            check_col_sum(rows, C, _as_result(rows, C, mutation))
        if mutation in ("drop_last_tail", "double_at_trip"):
            assert "against float64" in str(err.value), str(err.value)


def _col_sum_on_device(ops, rows, C):
    from speechdrivestemplates_amd import _lib
    lib = _lib.load()
    case = col_sum_case(rows, C)
    x = torch.tensor(case["x"]).to(DEV)
    got = {}
    for mode, prev in (("filled", case["out0"]), ("zeros", np.zeros(C, np.float32))):
        buf, out = _guarded_dev(C, torch.float32)
        out.copy_(torch.tensor(prev))
        got[mode] = []
        for _call in range(2):
            _lib.check(lib.sdt_col_sum_f32(x.data_ptr(), out.data_ptr(), rows, C, ops._stream()))
            got[mode].append(_to_np(buf).view(np.float32))
    torch.cuda.synchronize()
    return got


@gpu
@pytest.mark.parametrize("C", COLS)
def test_col_sum_kernel_is_the_restatement(ops, C):
    """sdt_col_sum_f32 through the C ABI at every rows x C: onto random and zero `out`, twice in a row, guard columns on both sides"""
    worst = max(check_col_sum(rows, C, _col_sum_on_device(ops, rows, C)) for rows in ROWS)
    print("  col_sum C = %d, %d row counts x 2 fills x 2 calls: equal to the restatement, worst %.2e of max against float64" % (C, len(ROWS), worst))


@gpu
@pytest.mark.parametrize("case", [("Conv1d 129 rows x 17", 3, 1, 43, 36, 17, 1, 3, 1, 1), ("Conv2d 253 rows x 33", 1, 11, 23, 31, 33, 3, 3, 1, 1)],
                         ids=lambda c: c[0])
def test_bias_gradient_with_a_registered_weight(ops, case):
    """ConvFn with a bias, the weight inside a WeightMirrors group: dbias is the restatement of its dY bit for bit and within the dbias bar of
    float64; forward and dX (through the batched mirror) within the bars of test_conv1d / test_conv2d"""
    tag, B, Hi, Wi, Cin, Cout, kh, kw, s, p = case
    one_d = Hi == 1
    g = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
    x = torch.randn(B, Hi, Wi, Cin, generator=g)
    spec = (Cout, Cin, kw if one_d else (kh, kw))
    st = tame(storage_values(spec, 77))  # (the +-3.4e38 specials would drown every other term of y and dX)
    b = torch.randn(Cout, generator=g)
    w_log = torch.from_numpy(st).view(Cout, kh, kw, Cin).permute(0, 3, 1, 2).double()
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    yr = F.conv2d(xr, w_log, b.double(), s, (0, p) if one_d else p)
    gy = (RHO * torch.where(torch.arange(Cout) % 2 == 0, 1.0, -1.0) + torch.randn(yr.permute(0, 2, 3, 1).shape, generator=g)).float()
    yr.backward(gy.double().permute(0, 3, 1, 2))
    wd, bd = make_param((st, spec)), torch.nn.Parameter(b.to(DEV))
    group = ops.WeightMirrors([wd])
    xd = (x[:, 0] if one_d else x).to(DEV).requires_grad_(True)
    yd = ops.ConvFn.apply(xd, wd, bd, s, p)
    yd.backward((gy[:, 0] if one_d else gy).to(DEV))
    ops.join_side_stream()
    torch.cuda.synchronize()
    assert not group.dirty and ops.WeightMirrors.lookup(wd) is group.entries[0][1]
    rows = gy.numel() // Cout
    assert (rows, Cout) == ((129, 17) if one_d else (253, 33))
    gy2 = gy.reshape(rows, Cout).numpy()
    want = col_sum_model(gy2, np.zeros(Cout, np.float32))[0]
    got = bd.grad.cpu().numpy()
    assert np.array_equal(bits32(got), bits32(want)), tag + ": dbias is not the restatement"
    e = _rel(got, gy2.astype(np.float64).sum(0))
    assert e < TOL_DBIAS, "%s dbias %.3e" % (tag, e)
    e_y = _rel(yd.detach().cpu().numpy().reshape(-1), yr.detach().permute(0, 2, 3, 1).reshape(-1).numpy())
    e_dx = _rel(xd.grad.cpu().numpy().reshape(-1), xr.grad.permute(0, 2, 3, 1).reshape(-1).numpy())
    print("  %s: dbias %.2e, fwd %.2e, dX %.2e of max against float64" % (tag, e, e_y, e_dx))
    assert e_y < TOL_CONV and e_dx < TOL_CONV, (tag, e_y, e_dx)
    assert_served_exact(ops, [wd], 0)
