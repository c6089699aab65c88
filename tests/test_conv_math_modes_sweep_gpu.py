"""The opt-in product-arithmetic modes of the fp32-tensor conv kernels (csrc/conv.hip: conv_taps_bf_kernel<NS>, conv_dw_kernel<.., true, NS>;
ops.set_conv_math('bf16' | 'bf16x3' | 'bf16x6')) swept over edge geometries through ops.conv_forward, ops.conv_input_grad and
ops.conv_weight_grad on full-precision fp32 operands, against the float64 EMULATION of each mode's products (tests/test_conv_math_modes_host.py:
the same operand pieces, the same piece pairs, summed in float64 -- only fp32 accumulation separates a correct kernel from it), and bf16x6 against
plain float64 as well.  The case table, the emulation and its host proofs live in that module.

Bars: those of tests/test_f32_conv_sweep_gpu.py for the same quantity (4e-6 forward and dX, 8e-6 dW), through check(): the stated bar and
10x the error recorded in tests/golden/margins.json.  No entry is widened: on its first run every case met them.

What a math mode reroutes (asserted here, listed in DESIGN.md section 4):
  * no stream-K, no fused multi-class dX launch (one launch per stride class), no conv1d_small_kernel (the short 1-D layers run
    conv_taps_bf_kernel with splitk > 1 + sdt_splitk_reduce_f32, which adds the bias), no ordered / grouped dW (fp32 atomics);
  * every launch is on the 64 x 64 tile (sdt_conv_taps_variant / sdt_conv_dw_variant: the larger instantiations exist in the tuning library only);
  * a forward launch with Cin % 32 != 0, an input gradient with Cout % 32 != 0 and a weight gradient off its vector path (Cin % 4 or Cout % 4)
    run the exact-fp32 kernel, silently: forward and dX bit-identical to 'f32' mode, dW (atomics in a mode, ordered in 'f32') within the dW bar;
  * a NormBwdHolder is NOT filled under a math mode: ops.conv_input_grad launches class by class without the statistics epilogue (dX is the
    mode's own, bit-identical to the call without a holder; the normalisation's backward then runs its own statistics pass), and the library
    refuses a fused-statistics or multi-class launch under a mode with SDT_ERR_ARG.  The exact-fp32 fall-back that launch_taps keeps for a
    launch with statistics is therefore not reachable through the public entry points.

SDT_MATH_SWEEP_TABLE=<path>: every test appends its rows (case, mode, quantity, error vs emulation, error vs float64) there
(profiles/r33_conv_math_sweep.txt is one such run)."""
import collections
import functools
import os

import pytest
import torch

from test_conv_math_modes_host import ACCUMULATE, CASE, CASES, MODES, SPLITK_1D, TOL_DW, TOL_DX, TOL_Y, dims, on_mode, operands, reference
from test_edge_shapes_gpu import DEV, check, ops, rel_err  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu

Got = collections.namedtuple("Got", "y yb dx dw dw2 dwfill")
HOLDER_CASES = ("k1", "k4s2-c32")
STATE_CASE = "3x3-cin96-c96"


def _poison(*shapes):
    """NaN blocks of the sizes the op allocates with torch.empty, allocated and freed: an unwritten element cannot hide behind stale zeros"""
    ts = [torch.full(shape, float("nan"), device=DEV) for shape in shapes]
    del ts


def _dev(ops, t):
    return ops.cl(t).to(DEV)


def _shapes(c):
    nd, B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    return ((B, Hi, Wi, Cin), (B, Ho, Wo, Cout)) if nd == 2 else ((B, Wi, Cin), (B, Wo, Cout))


def _fill(dw):
    """a deterministic pre-filled gradient of the size of dW (fp32-representable)"""
    return ((((torch.arange(dw.numel(), dtype=torch.float64) * 7919) % 13 - 6.0) * 0.125 * float(dw.abs().max())).reshape(dw.shape)).float()


def launch(ops, tag, accumulate=False):
    """y, y + bias, dX, dW (into a fresh .grad; ``accumulate``: a second call onto it and a call onto a pre-filled .grad as well) of a case under
    the math mode in force; channels-first on the CPU"""
    c = CASE[tag]
    s, p = c[9], c[10]
    x, w, gy, bias = operands(tag)
    xs, ys = _shapes(c)
    xd, gyd, bd = _dev(ops, x), _dev(ops, gy), bias.to(DEV)
    wd = torch.nn.Parameter(ops.to_weight_layout(w).to(DEV))
    _poison(ys)
    y = ops.conv_forward(xd, wd, None, s, p)
    _poison(ys)
    yb = ops.conv_forward(xd, wd, bd, s, p)
    _poison((c[5], c[7] * c[8], c[6]), xs)
    dx = ops.conv_input_grad(gyd, wd, xs, s, p)
    ops.conv_weight_grad(xd, gyd, wd, s, p)
    torch.cuda.synchronize()
    assert tuple(y.shape) == ys and tuple(dx.shape) == xs and wd.grad.stride() == wd.stride()
    dw, dw2, dwfill = wd.grad.detach().cpu().clone(), None, None
    if accumulate:
        ops.conv_weight_grad(xd, gyd, wd, s, p)
        dw2 = wd.grad.detach().cpu().clone()
        wd.grad = ops.to_weight_layout(_fill(reference(tag, "f64")["dw"])).to(DEV)
        assert wd.grad.stride() == wd.stride()
        ops.conv_weight_grad(xd, gyd, wd, s, p)
        torch.cuda.synchronize()
        dwfill = wd.grad.detach().cpu().clone()
    return Got(ops.cf_view(y).cpu(), ops.cf_view(yb).cpu(), ops.cf_view(dx).cpu(), dw, dw2, dwfill)


@functools.lru_cache(maxsize=None)
def f32_run(tag):
    """the same launches in the default arithmetic: what a fall-back must reproduce"""
    from speechdrivestemplates_amd import ops as o
    assert o.set_conv_math("f32") == "f32"
    return launch(o, tag)


def _geoms(ops, c):
    """(forward geometry, [input-gradient class geometries])"""
    nd, B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    if nd == 2:
        return ops.fwd_geom(B, Hi, Wi, Cin, Cout, kh, kw, s, p), [g for g, _ in ops.dx_geoms(B, Hi, Wi, Cin, Cout, kh, kw, s, p) if g is not None]
    return ops._fwd_geom_1d(B, Wi, Cin, Cout, kw, s, p), [g for g, _ in ops.dx_geoms_1d(B, Wi, Cin, Cout, kw, s, p) if g is not None]


def _unreachable(c):
    """mask over the spatial axes of the input pixels no output pixel reads: their gradient is exactly +0"""
    nd, B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    hit = torch.zeros(Hi + 2 * p + kh, Wi + 2 * p + kw, dtype=torch.bool)
    for i in range(kh):
        for j in range(kw):
            hit[i:i + (Ho - 1) * s + 1:s, j:j + (Wo - 1) * s + 1:s] = True
    pad_h = p if nd == 2 else 0
    dead = ~hit[pad_h:pad_h + Hi, p:p + Wi]
    return dead if nd == 2 else dead[0]


def _row(tag, mode, q, on, e_emu, e_f64):
    line = "%-16s %-7s %-12s %-9s vs emulation %.3e   vs float64 %.3e" % (tag, mode, q, "bf16 MFMA" if on else "fp32", e_emu, e_f64)
    print("  " + line)
    path = os.environ.get("SDT_MATH_SWEEP_TABLE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _compare(tag, mode, q, on, got, base, emu, f64, tol, bits=True):
    """one quantity: on the bf16 MFMA against the emulation (bf16x6: against float64 too); on a fall-back against 'f32' mode and float64"""
    _row(tag, mode, q, on, rel_err(got, emu), rel_err(got, f64))
    name = "%s %s %s" % (tag, mode, q)
    if on:
        check(name + " vs emulation", got, emu, tol)
        if mode == "bf16x6":
            check(name + " vs float64", got, f64, tol)
    else:
        if bits:
            assert torch.equal(got, base), "%s: the fall-back is not bit-identical to 'f32' mode" % name
        else:
            check(name + " fall-back vs 'f32' mode", got, base.double(), tol)
        check(name + " fall-back vs float64", got, f64, tol)


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
@pytest.mark.parametrize("mode", MODES)
def test_conv_math_sweep(ops, mode, tag):  # noqa: F811
    from speechdrivestemplates_amd import _lib
    lib = _lib.load()
    c = CASE[tag]
    fwd_on, dx_on, dw_on = on_mode(c)
    _x, _w, _gy, bias = operands(tag)
    f64, emu, base = reference(tag, "f64"), reference(tag, mode), f32_run(tag)
    gf, gdx = _geoms(ops, c)
    if tag in SPLITK_1D:  # in 'f32' mode these launches are conv1d_small_kernel's
        for g in [gf] + gdx:
            assert lib.sdt_conv1d_small_used(g, 1, ops._splitk_hint(lib, g)) == 1
    prev = ops.set_conv_math(mode)
    try:
        assert prev == "f32"
        for g in [gf] + gdx:  # one tile form under a math mode; no conv1d_small_kernel
            assert lib.sdt_conv_taps_variant(g) // 10 == 64064 and lib.sdt_conv_dw_variant(gf) // 10 == 64064
            assert lib.sdt_conv1d_small_used(g, 1, ops._splitk_hint(lib, g)) == 0
        if tag in SPLITK_1D:
            assert all(ops._splitk_hint(lib, g) > 1 for g in [gf] + gdx), "%s: expected split-K launches" % tag
        if tag == "3x3-unsplit":
            assert ops._splitk_hint(lib, gf) == 1 and ops._splitk_hint(lib, gdx[0]) > 1
        if tag == "dw-m1000":  # more than one row range
            assert lib.sdt_conv_dw_workspace_bytes(gf) // (4 * c[5] * c[6] * c[7] * c[8]) > 1
        got = launch(ops, tag, accumulate=tag in ACCUMULATE)
    finally:
        ops.set_conv_math("f32")
    _compare(tag, mode, "y", fwd_on, got.y, base.y, emu["y"], f64["y"], TOL_Y)
    shape = (1, -1) + (1,) * (got.y.dim() - 2)
    b64 = bias.double().reshape(shape)
    _compare(tag, mode, "y+bias", fwd_on, got.yb, base.yb, emu["y"] + b64, f64["y"] + b64, TOL_Y)
    _compare(tag, mode, "dx", dx_on, got.dx, base.dx, emu["dx"], f64["dx"], TOL_DX)
    dead = _unreachable(c)
    if bool(dead.any()):
        z = got.dx[..., dead]
        assert bool((z == 0).all()) and not bool(torch.signbit(z).any()), "%s %s: unreachable input pixels are not exactly +0" % (tag, mode)
    # dW: fp32 atomics under every mode -- by tolerance only, also where it falls back (the 'f32'-mode gradient is the ordered one)
    _compare(tag, mode, "dW", dw_on, got.dw, base.dw, emu["dw"], f64["dw"], TOL_DW, bits=False)
    if got.dw2 is not None:
        ref = emu["dw"] if dw_on else f64["dw"]
        fill = _fill(f64["dw"]).double()
        _row(tag, mode, "dW x2", dw_on, rel_err(got.dw2, 2.0 * emu["dw"]), rel_err(got.dw2, 2.0 * f64["dw"]))
        check("%s %s dW, second call adds" % (tag, mode), got.dw2, 2.0 * ref, TOL_DW)
        _row(tag, mode, "dW onto fill", dw_on, rel_err(got.dwfill, fill + emu["dw"]), rel_err(got.dwfill, fill + f64["dw"]))
        check("%s %s dW onto a pre-filled .grad" % (tag, mode), got.dwfill, fill + ref, TOL_DW)


def _holder(ops, c, groups, seed):
    nd, B, Hi, Wi, Cin = dims(c)[:5]
    g = torch.Generator().manual_seed(seed)
    h = ops.NormBwdHolder()
    h.y = torch.randn(B, Hi, Wi, Cin, generator=g).to(DEV)
    h.mean, h.rstd = torch.randn(groups * Cin, generator=g).to(DEV), (0.5 + torch.rand(groups * Cin, generator=g)).to(DEV)
    if groups == 1:
        h.gamma, h.beta = (1.0 + 0.1 * torch.randn(Cin, generator=g)).to(DEV), (0.1 * torch.randn(Cin, generator=g)).to(DEV)
    h.groups, h.slope = groups, 0.2
    return h


@pytest.mark.parametrize("tag", HOLDER_CASES)
@pytest.mark.parametrize("mode", MODES)
def test_holder_is_not_filled_under_a_math_mode(ops, mode, tag):  # noqa: F811
    """conv_input_grad with a NormBwdHolder: 'f32' mode fuses the backward statistics into the launch; a math mode launches class by class
    without them -- the holder stays empty (the normalisation's backward computes its own sums), dX is bit-identical to the call without a
    holder and meets the emulation's bar; asked directly, the library refuses the fused launch under a mode."""
    from speechdrivestemplates_amd import _lib
    lib = _lib.load()
    c = CASE[tag]
    nd, B, Hi, Wi, Cin, Cout, kh, kw, s, p, Ho, Wo = dims(c)
    _x, w, gy, _bias = operands(tag)
    gyd = _dev(ops, gy)
    wd = torch.nn.Parameter(ops.to_weight_layout(w).to(DEV))
    xs = (B, Hi, Wi, Cin)
    h32 = _holder(ops, c, 1, 5)
    dx32 = ops.conv_input_grad(gyd, wd, xs, s, p, h32)
    torch.cuda.synchronize()
    assert h32.sums is not None, "%s: 'f32' mode does not fuse the statistics here -- the case shows nothing" % tag
    check("%s f32 dx with a holder vs float64" % tag, ops.cf_view(dx32), reference(tag, "f64")["dx"], TOL_DX)
    prev = ops.set_conv_math(mode)
    try:
        assert prev == "f32"
        h = _holder(ops, c, 1, 5)
        _poison((Cin, kh * kw, Cout), xs)
        dxh = ops.conv_input_grad(gyd, wd, xs, s, p, h)
        _poison((Cin, kh * kw, Cout), xs)
        dx0 = ops.conv_input_grad(gyd, wd, xs, s, p)
        torch.cuda.synchronize()
        assert h.sums is None and h.dx_id is None, "%s %s: the holder was filled under a math mode" % (tag, mode)
        assert torch.equal(dxh, dx0)
        check("%s %s dx with a holder vs emulation" % (tag, mode), ops.cf_view(dxh), reference(tag, mode)["dx"], TOL_DX)
        # the library itself: a fused-statistics launch under a math mode is an argument error, not another arithmetic
        arr, n, _gs = ops.dx_pack(B, Hi, Wi, Cin, Cout, kh, kw, s, p, False)
        sums = torch.zeros(2 * Cin, dtype=torch.float64, device=DEV)
        nb = _lib.NormBwd(h.y.data_ptr(), h.mean.data_ptr(), h.rstd.data_ptr(), h.gamma.data_ptr(), h.beta.data_ptr(), sums.data_ptr(), 0.2, 1)
        wt = ops.weight_storage(wd.detach()).permute(2, 1, 0).contiguous()
        out = torch.zeros(xs, device=DEV)
        st = ops._stream()
        assert lib.sdt_conv_taps_multi_f32(gyd.data_ptr(), wt.data_ptr(), out.data_ptr(), arr, 1, 1, None, nb, st) != 0
        if n > 1:
            assert lib.sdt_conv_taps_multi_f32(gyd.data_ptr(), wt.data_ptr(), out.data_ptr(), arr, n, 1, None, None, st) != 0
        torch.cuda.synchronize()
        assert float(out.abs().max()) == 0.0 and float(sums.abs().max()) == 0.0  # refused before any launch
    finally:
        ops.set_conv_math("f32")


def _convfn_bits(ops, tag):
    c = CASE[tag]
    x, w, gy, bias = operands(tag)
    xd = _dev(ops, x).requires_grad_(True)
    wd = torch.nn.Parameter(ops.to_weight_layout(w).to(DEV))
    bd = torch.nn.Parameter(bias.to(DEV))
    y = ops.ConvFn.apply(xd, wd, bd, c[9], c[10])
    y.backward(_dev(ops, gy))
    torch.cuda.synchronize()
    return [t.detach().cpu().clone() for t in (y, xd.grad, wd.grad, bd.grad)]


@pytest.fixture(scope="module", autouse=True)
def before_the_sweep(ops):  # noqa: F811
    """a default-mode ConvFn call, taken before the first test of this module switches the arithmetic"""
    assert ops.set_conv_math("f32") == "f32"
    return _convfn_bits(ops, STATE_CASE)


def test_no_state_left_behind(ops, before_the_sweep):  # noqa: F811
    """After the sweep (and after one more round through the three modes here, so that the test stands alone): the mode in force is 'f32'
    and a default-mode ConvFn call reproduces its pre-sweep bits -- nothing process-wide leaked out of a mode."""
    for mode in MODES:
        assert ops.set_conv_math(mode) == "f32"
        try:
            launch(ops, STATE_CASE)
        finally:
            assert ops.set_conv_math("f32") == mode
    assert ops.set_conv_math("f32") == "f32"
    from speechdrivestemplates_amd import _lib
    assert _lib.load().sdt_get_conv_math() == 0 and ops._CONV_MATH_NOW[0] == 0
    for name, a, b in zip(("y", "dx", "dW", "dbias"), _convfn_bits(ops, STATE_CASE), before_the_sweep):
        assert torch.equal(a, b), "default-mode %s changed across the sweep" % name
