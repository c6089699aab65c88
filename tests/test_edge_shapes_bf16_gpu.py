"""Edge-shape parity of the bf16-storage instantiations of csrc/norm.hip and csrc/l0.hip (colstats_kernel / colnorm_apply_{fwd,bwd}_kernel with
__bf16 tensors, l0_fwd_kernel<__bf16>, l0_bwd_sums_kernel<__bf16>: 8-byte vector accesses, the ld4 / st4 / l0_cvt bit tricks, the
global_load_dwordx2 queue), and of the first block in fp32 at the shapes test_ops_gpu.py leaves out.  Conventions, builders and float64
references are those of test_edge_shapes_gpu.py (imported, not copied).

Inputs are float64 tensors holding bf16-representable values (y, dz; the affine parameters, the mel image and the weights are fp32 tensors
in either storage mode and stay fp32-representable): exactly what the kernels are given.  Quantisation changes two things, both handled by
the builder and asserted in each test: an input on the activation's kink is moved by whole bf16 steps (`off_kink_bf16`: the fp32 builder's
2.4e-3 is less than one step at |y| ~ 3 and would round back), alternately up and down along the rows, which also separates the exact ties
that two rows per statistic produce (variance 0, every pre-activation 0); no statistic over more than one row has zero variance.

The bar of a bf16 OUTPUT, per element:   |got - ref| <= 2^-8 |ref| + tol max|ref|
  2^-8 |ref|  half a bf16 step, what round-to-nearest-even may add to arithmetic that is fp32 on identical inputs -- derived, not measured;
  tol         the fp32 tolerance of the same quantity and shape in test_edge_shapes_gpu.py / test_ops_gpu.py, or 4x the error of the same
              formula in fp32 torch on the CPU against float64 on the very inputs of the check where that is more (FP32_REF_ERR below,
              printed by `python tests/test_edge_shapes_bf16_gpu.py`; never anything a kernel produced).
The largest ratio over the elements goes through the calibrated check with stated tolerance 1.0.  fp32 outputs of the bf16 path keep the plain
rel-max-err bar.  test_bf16_bar_discriminates (host only) shows what the bar rejects: truncation, swapped halves of a 32-bit pair, a lost row.

Bit agreement: the bf16-store and fp32-store kernels run the same source on the same values, so the stored bf16 must be the fp32 partner's
output rounded to nearest even, bit for bit.  A differing element is tolerated only if the two differ by one bf16 step and the partner's fp32
value lies within 2^-21 |x| of the midpoint between them (a differently contracted FMA); the count is printed per check (expected: 0)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_edge_shapes_gpu import DEV, EPS, KINK, NORM_TOL, SLOPES, _colnorm_cases, check, colnorm_data, colnorm_ref, f32

BF = torch.bfloat16
HALF_STEP = 2.0 ** -8  # half a bf16 step relative to the value (8 significant bits), at the bottom of a binade


@pytest.fixture()
def ops():
    from speechdrivestemplates_amd import ops as _ops
    prev = _ops.STORAGE
    yield _ops
    _ops.set_storage(prev)
    assert not _ops.streamk_error_codes()


def bf16r(x):
    """float64 tensor holding bf16-representable values"""
    return x.to(BF).double()


def off_kink_bf16(y, pre_acts, margin=KINK, exempt=None, spread=None):
    """_off_kink for bf16-representable y (G, R, C): an input whose float64 pre-activation lies within 2 x margin of the kink moves by 1, 2, 4, ...
    bf16 steps (doubling each time the same element is found again), up in even rows and down in odd ones -- two equal values of a two-row
    statistic (variance 0, both pre-activations exactly 0, or beta under BatchNorm) move apart instead of together."""
    moved = torch.zeros(y.shape, dtype=torch.int64)
    sign = (1.0 - 2.0 * (torch.arange(y.shape[1]) % 2)).reshape(1, -1, 1).double()
    for _ in range(40):
        bad = torch.zeros_like(y, dtype=torch.bool)
        for u in pre_acts(y):
            bad |= u.abs() < 2.0 * margin
        if y.shape[1] > 1:  # a statistic whose rows are all equal (with an affine beta its pre-activations are beta, off the kink)
            bad |= (y.max(1, keepdim=True).values == y.min(1, keepdim=True).values).expand_as(bad)
        if exempt is not None:
            bad &= ~exempt
        if not bool(bad.any()):
            return y
        step = torch.ldexp(torch.ones_like(y), torch.frexp(y)[1] - 8)  # |y| in [2^(e-1), 2^e): one bf16 step is 2^(e-8)
        y = bf16r(torch.where(bad, y + sign * step * 2.0 ** moved.double(), y))
        moved += bad
    raise AssertionError("inputs still on the kink")


def colnorm_bf16_data(kind, C, R, rho=None):
    return colnorm_data(kind, C, R, rho, KINK, bf16r, off_kink_bf16)


def assert_bf16_inputs(d, ref, kind):
    """what the builder promises: bf16-representable y / dz, clear of the kink, no statistic over more than one row with zero variance"""
    y = d["y"]
    assert torch.equal(y, bf16r(y)) and torch.equal(d["gz"], bf16r(d["gz"]))
    assert float(ref["u"].abs().min()) >= KINK and (kind == "IN" or float(ref["ue"].abs().min()) >= KINK)
    if y.shape[1] > 1:
        assert float(y.var(1, unbiased=False).min()) > 0.0


# Measured on the CPU (`python tests/test_edge_shapes_bf16_gpu.py`): rel-max-err of the same torch formula in fp32 against float64 on the
# very inputs of the named quantity, listed where 4x that error exceeds the inherited tolerance (tolerance used: 4x the figure).
FP32_REF_ERR = {
    # two rows / two pixels per statistic: the two values can lie close together (see test_edge_shapes_gpu.py)
    "IN C=4 R=2 slope=0.2 dy": 5.93e-04,
    "IN C=4 R=2 slope=0.0 dy": 1.88e-04,
    "BN C=4 R=2 slope=0.2 dy": 1.01e-04,
    "BN C=4 R=2 slope=0.0 dy": 1.62e-04,
    "IN C=12 R=2 slope=0.2 dy": 5.01e-04,
    "IN C=12 R=2 slope=0.0 dy": 2.78e-04,
    "BN C=12 R=2 slope=0.2 dy": 1.08e-04,
    "BN C=12 R=2 slope=0.0 dy": 4.24e-05,
    "IN C=36 R=2 slope=0.2 z": 7.14e-06,
    "IN C=36 R=2 slope=0.0 z": 7.14e-06,
    "BN C=36 R=2 slope=0.2 dy": 1.37e-05,
    "IN C=288 R=2 slope=0.2 z": 7.52e-06,
    "IN C=288 R=2 slope=0.0 z": 7.52e-06,
    "IN C=1020 R=2 slope=0.2 z": 1.49e-05,
    "IN C=1020 R=2 slope=0.0 z": 1.49e-05,
    "IN C=1024 R=2 slope=0.2 z": 1.20e-05,
    "IN C=1024 R=2 slope=0.0 z": 1.20e-05,
    "L0 IN (2, 1, 2) dW": 7.16e-03,
    "L0 IN (2, 2, 1) z": 7.27e-06,
    "L0 IN (2, 2, 1) dW": 1.74e-03,
}


def tol_for(key, inherited):
    e32 = FP32_REF_ERR.get(key)
    return inherited if e32 is None else max(inherited, 4.0 * e32)


def bf16_ratio(got, ref, tol):
    """max over the elements of |got - ref| / (2^-8 |ref| + tol max|ref|)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "non-finite values in kernel output"
    allowed = HALF_STEP * ref.abs() + tol * ref.abs().max()
    return ((got - ref).abs() / allowed.clamp_min(1e-300)).max().item()


def check_bf16(name, got, ref, tol):
    """The bar of a bf16 output through the calibrated check: stated tolerance 1.0 on the ratio, and 10x the ratio recorded in margins.json."""
    from conftest import calibrated_bound
    assert got.dtype == BF, got.dtype
    e = bf16_ratio(got, ref, tol)
    bound = calibrated_bound(name, e, 1.0)
    print("  %-52s bf16 bar ratio %.3f (fp32 tol %.1e, held to %.3f)" % (name, e, tol, bound))
    assert e <= bound, "%s: %.3f of half a bf16 step + %.1e of max > %.3f" % (name, e, tol, bound)


def bit_agreement(kernel, name, got, partner):
    """got (bf16) against partner (fp32, from the fp32-store instantiation) rounded to nearest even; -> number of tolerated differences"""
    assert got.dtype == BF and partner.dtype == torch.float32 and got.shape == partner.shape
    got, partner = got.detach().cpu().contiguous(), partner.detach().cpu().contiguous()
    want = partner.to(BF)
    a, b = got.view(torch.int16).int(), want.view(torch.int16).int()
    diff = a != b
    n = int(diff.sum())
    print("  bit agreement %-40s %-36s differing elements: %d of %d" % (kernel, name, n, got.numel()))
    if n:
        x, lo, hi = partner[diff].double(), got[diff].double(), want[diff].double()
        one_step = (a[diff] - b[diff]).abs() == 1  # sign-magnitude patterns: neighbours of the same sign
        at_tie = (x - 0.5 * (lo + hi)).abs() <= 2.0 ** -21 * x.abs()
        ok = one_step & at_tie
        assert bool(ok.all()), "%s %s: %d of %d differing elements are no rounding tie, first: fp32 %r stored %r" % (
            kernel, name, int((~ok).sum()), n, float(x[~ok][0]), float(lo[~ok][0]))
    return n


def same_bits(a, b):
    return a.dtype == b.dtype == torch.float32 and torch.equal(a.detach().cpu().contiguous().view(torch.int32),
                                                                b.detach().cpu().contiguous().view(torch.int32))


# =============================================================================================================================
# 0. the bar itself (host only)
# =============================================================================================================================
def test_bf16_bar_discriminates():
    """On the float64 reference of IN C = 12, R = 4 rpp + 1 = 341: round-to-nearest-even passes; truncation, the two halves of every 32-bit
    pair swapped, and the last (4 rpp + 1-th) row left at zero all fail."""
    kind, C, R = "IN", 12, 4 * (256 // 3) + 1
    d = colnorm_bf16_data(kind, C, R)
    ref = colnorm_ref(kind, d, 0.2)
    assert_bf16_inputs(d, ref, kind)
    z, tol = ref["z"], NORM_TOL[kind]["z"]
    rne = z.float().to(BF)
    assert bf16_ratio(rne, z, tol) <= 1.0
    trunc = (z.float().view(torch.int32) & -65536).view(torch.float32)
    assert torch.equal(trunc, trunc.to(BF).float())
    assert bf16_ratio(trunc.to(BF), z, tol) > 1.0
    swapped = rne.view(torch.int16).reshape(-1, 2).flip(1).reshape(z.shape).view(BF)
    assert bf16_ratio(swapped, z, tol) > 1.0
    lost = rne.clone()
    lost[:, R - 1] = 0
    assert bf16_ratio(lost, z, tol) > 1.0
    # and the tie rule of the bit agreement: a neighbour is tolerated only at a rounding tie
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -22, 1.25], dtype=torch.float32)  # a tie of 1 and 1 + 2^-7 (within four fp32 steps); no tie
    up = x.to(BF)
    down = (up.view(torch.int16) - 1).view(BF)
    assert bit_agreement("host", "tie", torch.stack([down[0], up[1]]), x) == 1
    with pytest.raises(AssertionError):
        bit_agreement("host", "no tie", down, x)


# =============================================================================================================================
# 1. norm.hip with bf16 y
# =============================================================================================================================
COMBOS = ("bf16", "mixed", "f32")  # (i) bf16 z and dz; (ii) out_f32: fp32 z and dz, bf16 y and dy; (iii) the fp32 kernels on y.float()
FWD_KERNEL = {"bf16": "colnorm_apply_fwd<bf16,bf16>"}
BWD_KERNEL = {"bf16": "colnorm_apply_bwd<bf16,bf16,bf16>", "mixed": "colnorm_apply_bwd<float,bf16,bf16>"}


def run_colnorm(ops, kind, d, slope, combo, backward=True):
    C = d["y"].shape[-1]
    ydt = torch.float32 if combo == "f32" else BF
    yd = d["y"].to(ydt).to(DEV).requires_grad_(True)
    out_f32 = combo == "mixed"
    got = {}
    if kind == "IN":
        zd = ops.ColNormActFn.apply(yd, None, None, None, None, None, d["G"], slope, None, None, out_f32)
    else:
        gd, bd = torch.nn.Parameter(d["gamma"].float().to(DEV)), torch.nn.Parameter(d["beta"].float().to(DEV))
        rmd, rvd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        zd = ops.ColNormActFn.apply(yd, gd, bd, rmd, rvd, nbt, 1, slope, None, None, out_f32)
    assert zd.dtype == (BF if combo == "bf16" else torch.float32)
    got["z"] = zd.detach()
    if backward:
        zd.backward(d["gz"].to(zd.dtype).to(DEV))
        assert yd.grad.dtype == ydt
        got["dy"] = yd.grad
    torch.cuda.synchronize()
    if kind == "BN":
        got.update(rm=rmd, rv=rvd, nbt=int(nbt.item()))
        if backward:
            got.update(dgamma=gd.grad, dbeta=bd.grad)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C,R", _colnorm_cases(), ids=lambda v: str(v))
def test_colnorm_bf16_edge_shapes(ops, kind, C, R):
    d = colnorm_bf16_data(kind, C, R)
    for slope in SLOPES:
        ref = colnorm_ref(kind, d, slope)
        assert_bf16_inputs(d, ref, kind)
        got = {combo: run_colnorm(ops, kind, d, slope, combo) for combo in COMBOS}
        tag = "%s C=%d R=%d slope=%.1f" % (kind, C, R, slope)
        tol = {q: tol_for(tag + " " + q, t) for q, t in NORM_TOL[kind].items()}
        for combo in ("bf16", "mixed"):
            g = got[combo]
            if combo == "bf16":
                check_bf16("bf16 %s z" % tag, g["z"], ref["z"], tol["z"])
            else:
                check("mixed %s z" % tag, g["z"], ref["z"], tol["z"])
            if R == 1:
                # one row: dy is exactly 0 in the reference; the kernel may keep the one fp32 rounding of g = dz act'(u) (test_edge_shapes_gpu.py),
                # and storing such a value as bf16 adds at most half a step of it
                assert float(ref["dy"].abs().max()) == 0.0
                bound = (1.0 + HALF_STEP) * 2.0 ** -24 * float(d["gz"].abs().max() * d["gamma"].abs().max()) / math.sqrt(EPS)
                e = float(g["dy"].double().abs().max())
                print("  %-52s max-abs %.3e (bound %.1e)" % ("%s %s dy" % (combo, tag), e, bound))
                assert math.isfinite(e) and e <= bound, (combo, tag, e, bound)
            else:
                check_bf16("%s %s dy" % (combo, tag), g["dy"], ref["dy"], tol["dy"])
            if kind == "BN":
                assert g["nbt"] == 1
                for q in ("dgamma", "dbeta", "rm", "rv"):
                    check("%s %s %s" % (combo, tag, q), g[q], ref[q], tol[q])
        f = got["f32"]
        bit_agreement(FWD_KERNEL["bf16"], tag + " z", got["bf16"]["z"], f["z"])
        assert same_bits(got["mixed"]["z"], f["z"]), "colnorm_apply_fwd<bf16,float> %s: z differs from the fp32 kernel's" % tag
        for combo in ("bf16", "mixed"):
            bit_agreement(BWD_KERNEL[combo], tag + " dy", got[combo]["dy"], f["dy"])


@pytest.mark.gpu
@pytest.mark.parametrize("rho", [0, 8])
@pytest.mark.parametrize("kind,R", [("IN", 1000), ("BN", 8520)])
def test_colnorm_bf16_large_mean_over_std(ops, kind, R, rho):
    """As test_colnorm_large_mean_over_std on bf16 inputs (forward): at rho = 8 they carry 8 bits against a mean of 8 std, and the quantised
    data keeps the intended |mean| / std within 10 % in every channel."""
    d = colnorm_bf16_data(kind, 64, R, float(rho))
    ref = colnorm_ref(kind, d, 0.2)
    assert_bf16_inputs(d, ref, kind)
    if rho:
        ratio = d["y"].mean(1).abs() / d["y"].std(1, unbiased=False)
        assert float((ratio - rho).abs().max()) <= 0.1 * rho, (float(ratio.min()), float(ratio.max()))
    tol = max(1e-5, 4.0 * 2.0 ** -24 * (1 + rho * rho))
    got = {combo: run_colnorm(ops, kind, d, 0.2, combo, backward=False) for combo in COMBOS}
    tag = "%s R=%d rho=%d fwd" % (kind, R, rho)
    check_bf16("bf16 " + tag, got["bf16"]["z"], ref["z"], tol)
    check("mixed " + tag, got["mixed"]["z"], ref["z"], tol)
    bit_agreement(FWD_KERNEL["bf16"], tag, got["bf16"]["z"], got["f32"]["z"])
    assert same_bits(got["mixed"]["z"], got["f32"]["z"])


# =============================================================================================================================
# 2. l0.hip, fp32 and bf16 storage
# =============================================================================================================================
# (B, H, W): one row / one column; W = 15 | 16 | 17 (len = (W + 15) / 16 steps from 1 to 2: a dead thread segment | none | seven of them and a
# half-filled one); B = 1 (groups == B == 1: InstanceNorm through the BatchNorm branch); the (7, 5) and B = 33 shapes of test_ops_gpu.py for the
# bf16 kernels; H * B = 3872: three image rows per workgroup of the backward kernel, the last workgroup of a clip has one
L0_SHAPES = [(2, 1, 2), (2, 2, 1), (3, 3, 15), (3, 3, 16), (3, 3, 17), (1, 4, 6), (3, 7, 5), (33, 81, 37), (32, 121, 9)]
L0_SMALL = 20000  # output elements up to which the seed keeps every pre-activation off the kink


def l0_ref(d, norm, dtype=torch.float64, clips=None):
    """the first block in torch: Conv2d(1, 64, k3, s1, p1) + InstanceNorm2d | BatchNorm2d(train) + LeakyReLU(0.2); channels-first outputs"""
    idx = list(range(d["mel"].shape[0])) if clips is None else clips
    mel = d["mel"][idx].to(dtype)
    w = d["w"].to(dtype).clone().requires_grad_(True)
    y = F.conv2d(mel.unsqueeze(1), w, None, 1, 1)
    out = {}
    if norm == "IN":
        u = F.instance_norm(y, eps=EPS)
    else:
        gamma, beta = d["gamma"].to(dtype).clone().requires_grad_(True), d["beta"].to(dtype).clone().requires_grad_(True)
        rm, rv = torch.zeros(64, dtype=dtype), torch.ones(64, dtype=dtype)
        u = F.batch_norm(y, rm, rv, gamma, beta, True, 0.1, EPS)
        out.update(rm=rm, rv=rv)
    z = F.leaky_relu(u, 0.2)
    z.backward(d["gz"][idx].to(dtype))
    out.update(u=u.detach(), z=z.detach(), dW=w.grad)
    if norm == "BN":
        out.update(dgamma=gamma.grad, dbeta=beta.grad)
    return out


@functools.lru_cache(maxsize=None)
def l0_data(B, H, W, norm, silent=None):
    """mel as in test_fused_first_block (non-negative, heavy tail), fp32-representable; the gradient bf16-representable (the same values go to
    both storages).  Small shapes: the first seed from the shape's own at which no float64 pre-activation lies within 2 x KINK of the kink
    (the all-zero clip ``silent`` is on it by construction and exempt)."""
    small = B * H * W * 64 <= L0_SMALL
    base = 1000 * B + H * W + (0 if norm == "IN" else 500000)
    for seed in range(base, base + (64 if small else 1)):
        g = torch.Generator().manual_seed(seed)
        d = {"mel": f32(torch.rand(B, H, W, generator=g, dtype=torch.float64) ** 3 * 40.0),
             "w": f32(torch.randn(64, 1, 3, 3, generator=g, dtype=torch.float64) * (2.0 / 9) ** 0.5),
             "gamma": f32(1 + 0.1 * torch.randn(64, generator=g, dtype=torch.float64)),
             "beta": f32(0.1 * torch.randn(64, generator=g, dtype=torch.float64)),
             "gz": bf16r(torch.randn(B, 64, H, W, generator=g, dtype=torch.float64)), "seed": seed}
        live = list(range(B))
        if silent is not None:
            d["mel"][silent] = 0.0
            live.remove(silent)
        if not small or float(l0_ref(d, norm)["u"][live].abs().min()) >= 2.0 * KINK:
            return d
    raise AssertionError("no seed keeps the pre-activations off the kink")


def run_l0(ops, d, norm, storage, affine=True):
    ops.set_storage(storage)
    B = d["mel"].shape[0]
    wd = torch.nn.Parameter(ops.to_weight_layout(d["w"].float()).to(DEV))
    mel = d["mel"].float().to(DEV)
    got = {}
    if norm == "IN":
        zd = ops.L0BlockFn.apply(mel, wd, None, None, None, None, None, B, 0.2)
    else:
        gd = torch.nn.Parameter(d["gamma"].float().to(DEV)) if affine else None
        bd = torch.nn.Parameter(d["beta"].float().to(DEV)) if affine else None
        rmd, rvd = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        zd = ops.L0BlockFn.apply(mel, wd, gd, bd, rmd, rvd, nbt, 1, 0.2)
    assert zd.dtype == (BF if storage == "bf16" else torch.float32) and zd.shape == (B,) + tuple(d["mel"].shape[1:]) + (64,)
    zd.backward(ops.cl(d["gz"]).to(zd.dtype).to(DEV))
    torch.cuda.synchronize()
    ops.set_storage("f32")
    got.update(z=zd.detach(), dW=wd.grad.detach().clone())
    if norm == "BN":
        got.update(rm=rmd, rv=rvd, nbt=int(nbt.item()))
        if affine:
            got.update(dgamma=gd.grad, dbeta=bd.grad)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["IN", "BN"])
@pytest.mark.parametrize("shape", L0_SHAPES, ids=str)
def test_first_block_edge_shapes(ops, shape, norm):
    """Two pixels per statistic, (2, 1, 2) and (2, 2, 1) under InstanceNorm, missed the forward bar by a decade (2.9e-4 / 1.4e-4 of max) while
    l0_moments_kernel formed the second moments from fp32 products; images of at most four pixels carry them in fp64 since."""
    B, H, W = shape
    d = l0_data(B, H, W, norm)
    ref = l0_ref(d, norm)
    small = B * H * W * 64 <= L0_SMALL
    if small:
        assert float(ref["u"].abs().min()) >= KINK
    tag = "L0 %s %s" % (norm, shape)
    # The two large shapes: gradient sums over up to 6.3 M elements, of which some always have a pre-activation within fp32 rounding of the
    # LeakyReLU kink and may take the other slope than in the float64 reference (a 0.8 |dz| change of one term): the 2e-3 of
    # test_fused_first_block.  The small shapes have no such element (asserted above) and are held to the forward bar.
    grad_tol = 2e-5 if small else 2e-3
    f, b = run_l0(ops, d, norm, "f32"), run_l0(ops, d, norm, "bf16")
    ztol = tol_for(tag + " z", 2e-5)
    check(tag + " f32 z", ops.cf_view(f["z"]), ref["z"], ztol)
    check_bf16(tag + " bf16 z", ops.cf_view(b["z"]), ref["z"], ztol)
    for q in ("dW", "dgamma", "dbeta") if norm == "BN" else ("dW",):
        t = tol_for("%s %s" % (tag, q), grad_tol)
        check("%s f32 %s" % (tag, q), f[q], ref[q], t)
        check("%s bf16 %s" % (tag, q), b[q], ref[q], t)  # float64 on the same rounded gradient
    check(tag + " dW, bf16 gradient vs the fp32 kernel", b["dW"], f["dW"], 1e-5)
    if norm == "BN":
        for st, g in (("f32", f), ("bf16", b)):
            assert g["nbt"] == 1
            check("%s %s running_mean" % (tag, st), g["rm"], ref["rm"], 1e-5)
            check("%s %s running_var" % (tag, st), g["rv"], ref["rv"], 1e-5)
    bit_agreement("l0_fwd<bf16>", tag + " z", b["z"], f["z"])
    if B == 1 and norm == "IN":
        # groups == B == 1: the InstanceNorm call takes the kernels' BatchNorm branch; so does BatchNorm without affine parameters
        for st, g in (("f32", f), ("bf16", b)):
            n = run_l0(ops, d, "BN", st, affine=False)
            assert n["nbt"] == 1
            assert torch.equal(n["z"].view(torch.int16 if st == "bf16" else torch.int32), g["z"].view(torch.int16 if st == "bf16" else torch.int32))
            assert same_bits(n["dW"], g["dW"])


@pytest.mark.gpu
def test_first_block_silent_clip(ops):
    """InstanceNorm with clip 1 all zeros: variance 0, rstd = 1 / sqrt(eps), every pre-activation of the clip exactly 0.  Zero inputs contribute
    zero to dW whichever slope is taken at u = 0, so dW is the float64 reference's with the clip left out."""
    B, H, W = 3, 5, 17
    d = l0_data(B, H, W, "IN", 1)
    assert not bool(d["mel"][1].any())
    assert bool((l0_ref(d, "IN")["u"][1] == 0).all())
    ref = l0_ref(d, "IN", clips=[0, 2])
    assert float(ref["u"].abs().min()) >= KINK
    tag = "L0 IN %s silent clip" % ((B, H, W),)
    ztol, wtol = tol_for(tag + " z", 2e-5), tol_for(tag + " dW", 2e-5)
    got = {st: run_l0(ops, d, "IN", st) for st in ("f32", "bf16")}
    for st, g in got.items():
        assert bool((g["z"][1] == 0).all()), "%s: the silent clip's output is not exactly 0" % st
        assert bool(torch.isfinite(g["z"].float()).all()) and bool(torch.isfinite(g["dW"]).all())
        (check_bf16 if st == "bf16" else check)("%s %s z" % (tag, st), ops.cf_view(g["z"][[0, 2]]), ref["z"], ztol)
        check("%s %s dW" % (tag, st), g["dW"], ref["dW"], wtol)
    check(tag + " dW, bf16 gradient vs the fp32 kernel", got["bf16"]["dW"], got["f32"]["dW"], 1e-5)
    bit_agreement("l0_fwd<bf16>", tag + " z", got["bf16"]["z"], got["f32"]["z"])


# =============================================================================================================================
# 3. argument checks of the _t entry points
# =============================================================================================================================
@pytest.mark.gpu
def test_bf16_entry_points_refuse_before_any_launch(ops):
    """Element-type combinations that are not built, unknown element-type codes and a mel image too wide for the backward kernel's LDS:
    RuntimeError from the library, and every output buffer keeps its fill value."""
    from speechdrivestemplates_amd import _lib
    lib, p, st = _lib.load(), ops._p, ops._stream()
    F32, BF16, BAD = _lib.F32, _lib.BF16, 7
    G, R, C, FILL = 2, 5, 8, 3.0
    outs = []

    def buf(n, dtype=torch.float32, fill=FILL):
        t = torch.full((n,), fill, dtype=dtype, device=DEV)
        outs.append((t, fill))
        return t

    n = G * R * C
    a32, a16 = buf(n), buf(n, BF)          # y / dz
    o32, o16 = buf(n), buf(n, BF)          # z / dy
    sums, mean, rstd = buf(2 * G * C, torch.float64, 0.0), buf(G * C), buf(G * C)

    def cn_fwd(y, ydt, z, zdt):
        return lib.sdt_colnorm_fwd_t(p(y), ydt, p(z), zdt, p(sums), p(mean), p(rstd), None, None, None, None, None, G, R, C, EPS, 0.1, 0.2, 0, st)

    def cn_bwd(dz, zdt, y, ydt, dy, ddt):
        return lib.sdt_colnorm_bwd_t(p(dz), zdt, p(y), ydt, p(dy), ddt, p(sums), p(mean), p(rstd), None, None, None, None, G, R, C, 0.2, 0, st)

    B, H, W = 1, 1, 3412  # (rows + 2) x (W + 2) floats of LDS: 3 x 3414 x 4 = 40 968 > 40 960
    mel, w0 = buf(B * H * W, fill=0.0), buf(64 * 9)
    z0, gz0 = buf(B * H * W * 64, BF), buf(B * H * W * 64, BF, 0.0)
    mom, sums0 = buf(54 * B, torch.float64, 0.0), buf(11 * 64, torch.float64, 0.0)
    mean0, rstd0, dw0 = buf(64), buf(64), buf(64 * 9)

    def l0_fwd(zdt, w=8):
        return lib.sdt_l0_block_fwd_t(p(mel), p(w0), p(z0), zdt, p(mom), p(mean0), p(rstd0), None, None, None, None, None, B, H, w, B, EPS, 0.1, 0.2, st)

    def l0_bwd(zdt, w=8):
        return lib.sdt_l0_block_bwd_t(p(gz0), zdt, p(mel), p(w0), p(mean0), p(rstd0), None, None, p(mom), p(sums0), p(dw0), None, None, B, H, w, B, 0.2, st)

    calls = {"colnorm fwd: fp32 y, bf16 z": lambda: cn_fwd(a32, F32, o16, BF16),
             "colnorm bwd: bf16 dz, fp32 y": lambda: cn_bwd(a16, BF16, a32, F32, o32, F32),
             "colnorm fwd: unknown y type": lambda: cn_fwd(a16, BAD, o16, BF16),
             "colnorm fwd: unknown z type": lambda: cn_fwd(a16, BF16, o16, BAD),
             "colnorm bwd: unknown dz type": lambda: cn_bwd(a16, BAD, a16, BF16, o16, BF16),
             "colnorm bwd: unknown y type": lambda: cn_bwd(a16, BF16, a16, BAD, o16, BF16),
             "colnorm bwd: unknown dy type": lambda: cn_bwd(a16, BF16, a16, BF16, o16, BAD),
             "first block fwd: unknown z type": lambda: l0_fwd(BAD),
             "first block bwd: unknown dz type": lambda: l0_bwd(BAD),
             "first block bwd: W = 3412": lambda: l0_bwd(BF16, W)}
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="libsdt_hip"):
            _lib.check(call())
        torch.cuda.synchronize()
        for t, fill in outs:
            assert bool((t == fill).all()), "%s: a kernel ran" % name


# =============================================================================================================================
# FP32_REF_ERR: `python tests/test_edge_shapes_bf16_gpu.py` checks every builder on the CPU (termination, kink, variance: the reference alone
# passes them) and prints the table's entries
# =============================================================================================================================
def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def _measure_fp32_ref_err():
    rows = []
    for kind, C, R in _colnorm_cases():
        d = colnorm_bf16_data(kind, C, R)
        for slope in SLOPES:
            r64, r32 = colnorm_ref(kind, d, slope), colnorm_ref(kind, d, slope, torch.float32)
            assert_bf16_inputs(d, r64, kind)
            for q, t in NORM_TOL[kind].items():
                if q != "ze" and float(r64[q].abs().max()) > 0.0:
                    rows.append(("%s C=%d R=%d slope=%.1f %s" % (kind, C, R, slope, q), _rel(r32[q], r64[q]), t))
    for kind, R in (("IN", 1000), ("BN", 8520)):
        for rho in (0, 8):
            d = colnorm_bf16_data(kind, 64, R, float(rho))
            assert_bf16_inputs(d, colnorm_ref(kind, d, 0.2), kind)
    cases = [(s, norm, None) for s in L0_SHAPES for norm in ("IN", "BN") if s[0] * s[1] * s[2] * 64 <= L0_SMALL] + [((3, 5, 17), "IN", 1)]
    for (B, H, W), norm, silent in cases:
        d = l0_data(B, H, W, norm, silent)
        clips = None if silent is None else [b for b in range(B) if b != silent]
        r64, r32 = l0_ref(d, norm, clips=clips), l0_ref(d, norm, torch.float32, clips=clips)
        assert float(r64["u"].abs().min()) >= KINK
        tag = "L0 %s %s" % (norm, (B, H, W)) + (" silent clip" if silent is not None else "")
        print("# %s: seed %d" % (tag, d["seed"]))
        for q in ("z", "dW", "dgamma", "dbeta") if norm == "BN" else ("z", "dW"):
            rows.append(("%s %s" % (tag, q), _rel(r32[q], r64[q]), 2e-5))
    for key, e, t in rows:
        if 4.0 * e > t:
            print('    "%s": %.2e,' % (key, e))


if __name__ == "__main__":
    _measure_fp32_ref_err()
