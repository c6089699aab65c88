"""Edge-shape float64 parity of the resampling kernels of csrc/misc.hip (resize_concat_fwd_kernel, resize_bwd_kernel,
code_scatter_bwd_kernel, upsample_add_fwd_kernel, upsample_bwd_kernel): the backward candidate window at strong up- and down-sampling, the
clamped ends of src_index (W = 1, Ti = 1, T = 1), every height (ly = 0.5 for even H, H = 1), code widths and B x D that fill no whole
workgroup, time slices left empty or ragged (T < 8), the second trip of the grid-stride loops, and To < Ti.

References are F.interpolate on the CPU, in float64 on fp32-representable inputs (and in fp32 for the forward of resize: ATen computes the
source index in fp32 by the formula of src_index).  Tolerances are the stated ones of the same quantity in test_ops_gpu.py.  Where a shape
needs more, the tolerance is 4x the error of the SAME torch formula in fp32 on the CPU against float64 on the same input (4x: the
accumulation order differs); those measured fp32-reference errors are the FP32_REF_ERR table below -- never anything a kernel produced.

Every case additionally checks, on the kernels' own outputs taken to float64:
  * the adjoint identity <fwd(x), g> = <x, bwd(g)> (relative to |fwd(x)| |g|; bar: 4x the same quantity of fp32 torch on the CPU, floored
    at 1e-6) -- a dropped or doubled window contribution shows here whatever the elementwise tolerance;
  * gout = 1: the gradient of each clip sums to (frames x channels), since the weights of every output frame sum to 1;
  * a second run, through the C ABI into NaN-filled buffers, is bit-identical and leaves no element unwritten."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_edge_shapes_gpu import check, f32

pytestmark = pytest.mark.gpu

DEV = "cuda"
ADJ_FLOOR = 1e-6
ONES_TOL = 1e-6


@pytest.fixture(scope="module")
def ops():
    from speechdrivestemplates_amd import ops as o
    return o


# Measured on the CPU: rel-max-err of the same torch formula in fp32 against float64, on the very inputs of the named check, for the checks
# where that error misses the inherited tolerance (tolerance used: 4x the figure).  All other checks keep the inherited tolerance.
# Produced by:  python -c "import sys; sys.path[:0] = ['tests', '.']; import test_resample_edge_shapes_gpu as t; t.print_fp32_ref_err()"
FP32_REF_ERR = {
}


def tol_for(key, inherited):
    e32 = FP32_REF_ERR.get(key)
    return inherited if e32 is None else 4.0 * e32


def _rel(got, ref):
    return ((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30)).item()


def _adjoint_gap(out, g, pairs):
    """|<out, g> - sum <x, dx>| / (|out| |g|), everything taken to float64"""
    out, g = out.detach().double().cpu(), g.detach().double().cpu()
    lhs = (out * g).sum()
    rhs = sum((a.detach().double().cpu() * b.detach().double().cpu()).sum() for a, b in pairs)
    return (abs(lhs - rhs) / (out.norm() * g.norm()).clamp_min(1e-300)).item()


# =============================================================================================================================
# 1. resize + code concat
# =============================================================================================================================
# (B, H, W, C, T, D)
RESIZE_CASES = (
    [(2, H, 7, 8, 9, 4) for H in (1, 2, 4, 5)]                                       # heights: ly = 0 | 0.5 | 0.5 | 0
    + [(2, 5, 3, 8, 360, 0), (1, 5, 1, 4, 64, 4), (3, 5, 2, 12, 33, 36)]             # strong upsampling (W = 1: every frame reads column 0)
    + [(2, 5, 283, 8, 5, 4), (2, 5, 51, 8, 1, 0), (2, 5, 427, 4, 3, 32)]             # strong downsampling (T = 1)
    + [(2, 5, 17, 8, 17, 4), (2, 5, 16, 8, 17, 4), (2, 5, 17, 8, 16, 4)]             # identity and next to it
    + [(33, 5, 51, 256, 64, 32), (3, 5, 51, 256, 40, 32)]                            # production-like with odd sizes
    # code scatter: B x D fills no whole workgroup of 32 pairs; T < 8 leaves time slices empty, T = 13 ragged
    + [(B, 2, 5, 8, T, D) for D in (4, 36, 100) for B in (1, 3, 9) for T in (1, 5, 8, 13)]
    + [(16, 1, 40, 256, 1024, 32),     # forward: 1 179 648 vectors, a grid holds 4096 x 256 = 1 048 576
       (16, 5, 283, 256, 8, 0)]        # backward over B H W C / 4 = 1 448 960 vectors
)
assert all((B * D) % 32 for (B, H, W, C, T, D) in RESIZE_CASES if (H, W, C) == (2, 5, 8))
assert 16 * 1024 * (256 + 32) // 4 > 4096 * 256 and 16 * 5 * 283 * 256 // 4 > 4096 * 256


def _rid(case):
    return "B%d-H%d-W%d-C%d-T%d-D%d" % case


@functools.lru_cache(maxsize=None)
def _resize_data(case):
    B, H, W, C, T, D = case
    g = torch.Generator().manual_seed(sum(p * v for p, v in zip((1, 3, 7, 11, 13, 17), case)))
    x = f32(torch.randn(B, C, H, W, generator=g, dtype=torch.float64))
    code = f32(torch.randn(B, D, generator=g, dtype=torch.float64)) if D else None
    gr = f32(torch.randn(B, C + D, T, generator=g, dtype=torch.float64))
    return x, code, gr


def _resize_torch(case, dtype):
    """the reference operator (generator.py:41-42,110-111) in ``dtype`` on the CPU -> out (B, C + D, T), dx, dcode"""
    B, H, W, C, T, D = case
    x, code, gr = _resize_data(case)
    x = x.to(dtype).clone().requires_grad_(True)  # (clone: .to() of the same dtype hands back the shared input itself)
    code = code.to(dtype).clone().requires_grad_(True) if D else None
    r = F.interpolate(x, (1, T), mode="bilinear").squeeze(2)
    if D:
        r = torch.cat([r, code.unsqueeze(2).repeat(1, 1, T)], 1)
    r.backward(gr.to(dtype))
    return r.detach(), x.grad, (code.grad if D else None)


@functools.lru_cache(maxsize=None)
def _resize_ref(case):
    return _resize_torch(case, torch.float64)


def _resize_checks(case):
    """[(name, inherited tolerance, index into (out, dx, dcode))]"""
    B, H, W, C, T, D = case
    tag = _rid(case)
    rows = [("resize+concat fwd " + tag, 5e-5, 0), ("resize bwd dx " + tag, 5e-5, 1)]
    if D:
        rows.append(("resize bwd dcode " + tag, 1e-5, 2))
    return rows


def _resize_fp32_cpu(case):
    """fp32 torch on the CPU against float64: {check name: error}, and the adjoint gap of the fp32 run"""
    B, H, W, C, T, D = case
    x, code, gr = _resize_data(case)
    r32, r64 = _resize_torch(case, torch.float32), _resize_ref(case)
    errs = {name: _rel(r32[k], r64[k]) for name, _t, k in _resize_checks(case)}
    gap = _adjoint_gap(r32[0], gr, [(x, r32[1])] + ([(code, r32[2])] if D else []))
    return errs, gap


@pytest.mark.parametrize("case", RESIZE_CASES, ids=_rid)
def test_resize_concat_edge_shapes(ops, case):
    from speechdrivestemplates_amd import _lib
    B, H, W, C, T, D = case
    x, code, gr = _resize_data(case)
    out64, dx64, dcode64 = _resize_ref(case)
    xd = ops.cl(x.float()).to(DEV).requires_grad_(True)
    cd = code.float().to(DEV).requires_grad_(True) if D else None
    gd = ops.cl(gr.float()).to(DEV)
    rd = ops.ResizeConcatFn.apply(xd, cd, T)
    rd.backward(gd)
    assert rd.shape == (B, T, C + D) and xd.grad.shape == (B, H, W, C)
    got = (ops.cf_view(rd), ops.cf_view(xd.grad), cd.grad if D else None)

    # forward against ATen in fp32 (same source-index formula), then everything against float64
    r32 = F.interpolate(x.float(), (1, T), mode="bilinear").squeeze(2)
    check("resize fwd vs fp32 ref " + _rid(case), got[0][:, :C], r32, 2e-6)
    for name, tol, k in _resize_checks(case):
        check(name, got[k], (out64, dx64, dcode64)[k], tol_for(name, tol))
    if D:  # the code columns are copies
        assert torch.equal(rd[:, :, C:].cpu(), code.float().unsqueeze(1).expand(B, T, D))

    # adjoint identity on the kernels' own outputs
    _e32, gap32 = _resize_fp32_cpu(case)
    gap = _adjoint_gap(got[0], gr, [(x, got[1])] + ([(code, got[2])] if D else []))
    bar = max(4.0 * gap32, ADJ_FLOOR)
    print("  adjoint gap %.3e (fp32 torch on the CPU %.3e, bar %.1e)" % (gap, gap32, bar))
    assert gap <= bar, "adjoint identity: %.3e > %.1e" % (gap, bar)

    # a second run through the C ABI into NaN-filled buffers: bit-identical, nothing left unwritten
    lib = _lib.load()
    idx = torch.arange(B, device=DEV, dtype=torch.int64) if D else None
    xc, cc = xd.detach().contiguous(), (cd.detach().contiguous() if D else None)
    out2 = torch.full((B, T, C + D), float("nan"), device=DEV)
    _lib.check(lib.sdt_resize_concat_fwd_f32(ops._p(xc), ops._p(cc), ops._p(idx), ops._p(out2), B, H, W, C, T, D, ops._stream()))
    dx2 = torch.full((B, H, W, C), float("nan"), device=DEV)
    dcode2 = torch.zeros((B, D), device=DEV) if D else None  # (accumulated into: zero on entry, as ResizeConcatFn hands it over)
    _lib.check(lib.sdt_resize_concat_bwd_f32(ops._p(gd), ops._p(idx), ops._p(dx2), ops._p(dcode2), B, H, W, C, T, D, ops._stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(out2).all() and torch.isfinite(dx2).all()
    assert torch.equal(out2, rd.detach()) and torch.equal(dx2, xd.grad)
    if D:
        assert torch.isfinite(dcode2).all() and torch.equal(dcode2, cd.grad)

    # gout = 1: the weights of every output frame sum to 1, so each clip's dx sums to T x C (and dcode is T everywhere)
    ones = torch.ones((B, T, C + D), device=DEV)
    dx1 = torch.full((B, H, W, C), float("nan"), device=DEV)
    dcode1 = torch.zeros((B, D), device=DEV) if D else None
    _lib.check(lib.sdt_resize_concat_bwd_f32(ops._p(ones), ops._p(idx), ops._p(dx1), ops._p(dcode1), B, H, W, C, T, D, ops._stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(dx1).all()
    per_clip = dx1.double().sum(dim=(1, 2, 3)).cpu()
    worst = ((per_clip - T * C).abs().max() / (T * C)).item()
    assert worst <= ONES_TOL, "sum of dx per clip for gout = 1: %s, expected %d" % (per_clip.tolist(), T * C)
    if D:
        assert torch.equal(dcode1.cpu(), torch.full((B, D), float(T)))


# =============================================================================================================================
# 2. upsample (+ skip)
# =============================================================================================================================
# (B, Ti, To, C)
UPSAMPLE_SHAPES = [(2, 1, 7, 8), (2, 1, 1, 4), (2, 2, 5, 8), (3, 5, 11, 12), (2, 7, 8, 256),
                   (2, 16, 33, 256), (2, 23, 47, 256), (2, 3, 6, 4), (2, 17, 17, 8),  # (17 -> 17: identity)
                   (2, 23, 10, 8), (2, 64, 1, 4)]                                       # To < Ti
UPSAMPLE_BIG = (9, 256, 512, 1024)  # forward: 1 179 648 vectors; backward 589 824 (one trip: bounded by the input)
UPSAMPLE_CASES = [s + (skip,) for s in UPSAMPLE_SHAPES for skip in (True, False)] + [UPSAMPLE_BIG + (True,)]
assert 9 * 512 * 1024 // 4 > 4096 * 256


def _uid(case):
    return "B%d-Ti%d-To%d-C%d-%s" % (case[:4] + ("skip" if case[4] else "noskip",))


@functools.lru_cache(maxsize=None)
def _upsample_data(case):
    B, Ti, To, C, skip = case
    g = torch.Generator().manual_seed(sum(p * v for p, v in zip((1, 3, 7, 11, 13), case)))
    prev = f32(torch.randn(B, C, Ti, generator=g, dtype=torch.float64))
    sk = f32(torch.randn(B, C, To, generator=g, dtype=torch.float64)) if skip else None
    gr = f32(torch.randn(B, C, To, generator=g, dtype=torch.float64))
    return prev, sk, gr


def _upsample_torch(case, dtype):
    """generator.py:79-83 in ``dtype`` on the CPU -> out (B, C, To), dprev, dskip"""
    B, Ti, To, C, skip = case
    prev, sk, gr = _upsample_data(case)
    prev = prev.to(dtype).clone().requires_grad_(True)
    sk = sk.to(dtype).clone().requires_grad_(True) if skip else None
    r = F.interpolate(prev, To, mode="linear")
    if skip:
        r = r + sk
    r.backward(gr.to(dtype))
    return r.detach(), prev.grad, (sk.grad if skip else None)


@functools.lru_cache(maxsize=None)
def _upsample_ref(case):
    return _upsample_torch(case, torch.float64)


def _upsample_checks(case):
    tag = _uid(case)
    rows = [("upsample+add fwd " + tag, 5e-6, 0), ("upsample bwd dprev " + tag, 5e-5, 1)]
    if case[4]:
        rows.append(("upsample bwd dskip " + tag, 1e-6, 2))
    return rows


def _upsample_fp32_cpu(case):
    prev, sk, gr = _upsample_data(case)
    r32, r64 = _upsample_torch(case, torch.float32), _upsample_ref(case)
    errs = {name: _rel(r32[k], r64[k]) for name, _t, k in _upsample_checks(case)}
    gap = _adjoint_gap(r32[0], gr, [(prev, r32[1])] + ([(sk, r32[2])] if case[4] else []))
    return errs, gap


@pytest.mark.parametrize("case", UPSAMPLE_CASES, ids=_uid)
def test_upsample_add_edge_shapes(ops, case):
    from speechdrivestemplates_amd import _lib
    B, Ti, To, C, skip = case
    prev, sk, gr = _upsample_data(case)
    ref = _upsample_ref(case)
    pd = ops.cl(prev.float()).to(DEV).requires_grad_(True)
    sd = ops.cl(sk.float()).to(DEV).requires_grad_(True) if skip else None
    gd = ops.cl(gr.float()).to(DEV)
    rd = ops.UpsampleAddFn.apply(pd, sd, To)
    rd.backward(gd)
    assert rd.shape == (B, To, C) and pd.grad.shape == (B, Ti, C)
    got = (ops.cf_view(rd), ops.cf_view(pd.grad), ops.cf_view(sd.grad) if skip else None)
    for name, tol, k in _upsample_checks(case):
        check(name, got[k], ref[k], tol_for(name, tol))
    if not skip:  # no gradient for an absent skip, and the forward is the interpolation alone
        r32 = F.interpolate(prev.float(), To, mode="linear")
        check("upsample alone vs fp32 ref " + _uid(case), got[0], r32, 2e-6)
    else:
        assert torch.equal(sd.grad, gd)

    _e32, gap32 = _upsample_fp32_cpu(case)
    gap = _adjoint_gap(got[0], gr, [(prev, got[1])] + ([(sk, got[2])] if skip else []))
    bar = max(4.0 * gap32, ADJ_FLOOR)
    print("  adjoint gap %.3e (fp32 torch on the CPU %.3e, bar %.1e)" % (gap, gap32, bar))
    assert gap <= bar, "adjoint identity: %.3e > %.1e" % (gap, bar)

    lib = _lib.load()
    pc, sc = pd.detach().contiguous(), (sd.detach().contiguous() if skip else None)
    out2 = torch.full((B, To, C), float("nan"), device=DEV)
    _lib.check(lib.sdt_upsample_add_fwd_f32(ops._p(pc), ops._p(sc), ops._p(out2), B, Ti, To, C, ops._stream()))
    dp2 = torch.full((B, Ti, C), float("nan"), device=DEV)
    _lib.check(lib.sdt_upsample_add_bwd_f32(ops._p(gd), ops._p(dp2), B, Ti, To, C, ops._stream()))
    ones = torch.ones((B, To, C), device=DEV)
    dp1 = torch.full((B, Ti, C), float("nan"), device=DEV)
    _lib.check(lib.sdt_upsample_add_bwd_f32(ops._p(ones), ops._p(dp1), B, Ti, To, C, ops._stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(out2).all() and torch.isfinite(dp2).all() and torch.isfinite(dp1).all()
    assert torch.equal(out2, rd.detach()) and torch.equal(dp2, pd.grad)
    per_clip = dp1.double().sum(dim=(1, 2)).cpu()
    worst = ((per_clip - To * C).abs().max() / (To * C)).item()
    assert worst <= ONES_TOL, "sum of dprev per clip for gout = 1: %s, expected %d" % (per_clip.tolist(), To * C)


# =============================================================================================================================
# 3. arguments the vector accesses cannot serve are refused before any launch
# =============================================================================================================================
def _sentinel(*shape):
    return torch.full(shape, -77.0, device=DEV)


def test_channel_counts_that_are_no_multiple_of_four_are_refused(ops, monkeypatch):
    """C % 4 != 0 (both resize entry points, both upsample entry points) and D % 4 != 0 (resize forward): status != 0 with sdt_last_error set,
    and no kernel has run -- the outputs keep what they held.  Through the autograd functions the refusal surfaces as a RuntimeError."""
    from speechdrivestemplates_amd import _lib
    lib = _lib.load()
    st = ops._stream()
    B, H, W, T = 2, 5, 7, 9

    def refused(status, entry, *outs):
        torch.cuda.synchronize()
        assert status != 0, entry
        msg = lib.sdt_last_error().decode()
        assert entry in msg, msg
        for o in outs:
            assert bool((o == -77.0).all()), "%s wrote into its output although it refused the call" % entry

    for C, D in ((6, 4), (8, 6), (3, 0), (8, 2)):
        x, code, idx = torch.zeros(B, H, W, C, device=DEV), torch.zeros(B, max(D, 1), device=DEV), torch.arange(B, device=DEV)
        out = _sentinel(B, T, C + D)
        refused(lib.sdt_resize_concat_fwd_f32(ops._p(x), ops._p(code), ops._p(idx), ops._p(out), B, H, W, C, T, D, st),
                "sdt_resize_concat_fwd_f32", out)
    for C in (6, 3, 254):
        dout, dx, dcode = torch.zeros(B, T, C + 4, device=DEV), _sentinel(B, H, W, C), _sentinel(B, 4)
        idx = torch.arange(B, device=DEV)
        refused(lib.sdt_resize_concat_bwd_f32(ops._p(dout), ops._p(idx), ops._p(dx), ops._p(dcode), B, H, W, C, T, 4, st),
                "sdt_resize_concat_bwd_f32", dx, dcode)
        prev, out = torch.zeros(B, 5, C, device=DEV), _sentinel(B, 11, C)
        refused(lib.sdt_upsample_add_fwd_f32(ops._p(prev), None, ops._p(out), B, 5, 11, C, st), "sdt_upsample_add_fwd_f32", out)
        dout, dprev = torch.zeros(B, 11, C, device=DEV), _sentinel(B, 5, C)
        refused(lib.sdt_upsample_add_bwd_f32(ops._p(dout), ops._p(dprev), B, 5, 11, C, st), "sdt_upsample_add_bwd_f32", dprev)

    # through the autograd functions: the entry point is reached once, answers with its status, and the wrapper raises
    seen = []

    def recording(name):
        real = getattr(lib, name)

        def call(*a):
            seen.append((name, real(*a)))
            return seen[-1][1]
        monkeypatch.setattr(lib, name, call)
    for name in ("sdt_resize_concat_fwd_f32", "sdt_upsample_add_fwd_f32"):
        recording(name)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.ResizeConcatFn.apply(torch.zeros(B, H, W, 6, device=DEV), torch.zeros(B, 4, device=DEV), T)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.ResizeConcatFn.apply(torch.zeros(B, H, W, 8, device=DEV), torch.zeros(B, 6, device=DEV), T)
    with pytest.raises(RuntimeError, match="sdt_upsample_add_fwd_f32"):
        ops.UpsampleAddFn.apply(torch.zeros(B, 5, 6, device=DEV), None, 11)
    assert [n for n, _s in seen] == ["sdt_resize_concat_fwd_f32"] * 2 + ["sdt_upsample_add_fwd_f32"] and all(s != 0 for _n, s in seen)


# =============================================================================================================================
def print_fp32_ref_err():
    """CPU only: the FP32_REF_ERR entries (fp32 torch against float64 where it misses the inherited tolerance) and the fp32 adjoint gaps"""
    rows, gaps = [], []
    for cases, fp32_cpu, checks, ident in ((RESIZE_CASES, _resize_fp32_cpu, _resize_checks, _rid),
                                           (UPSAMPLE_CASES, _upsample_fp32_cpu, _upsample_checks, _uid)):
        for case in cases:
            errs, gap = fp32_cpu(case)
            gaps.append((ident(case), gap))
            for name, tol, _k in checks(case):
                if errs[name] >= tol:
                    rows.append((name, errs[name], tol))
    for name, e, tol in rows:
        print('    "%s": %.2e,  # inherited %.0e' % (name, e, tol))
    print("largest fp32 adjoint gap: %s" % (max(gaps, key=lambda r: r[1]),))
