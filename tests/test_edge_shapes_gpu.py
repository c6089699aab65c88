"""Edge-shape float64 parity of the small kernels that every train / validation step runs (csrc/misc.hip, csrc/norm.hip): the
grid-stride second trip, partly filled and single workgroups, scalar tails, idle lanes, masked rows of the unrolled loads, repeated and
out-of-range row indices.  Every comparison is against a float64 CPU statement of the reference operator on fp32-representable inputs.

Inputs.  Where the reference goes through LeakyReLU / ReLU the inputs are built so that no float64 pre-activation lies within KINK = 1e-4
of the kink (asserted in each such test): an fp32 kernel cannot land on the other side for such inputs, so no element is excluded from
any comparison.  Small cases get there by their seed; for the cases with 1e5..3e6 elements (where some element always falls inside) the
few offending inputs are moved by a fixed fraction of the input's spread, deterministically (`_off_kink`).

Tolerances are the stated ones of the same quantity in test_ops_gpu.py.  Where a shape needs more, the tolerance is 4x the error of the
SAME formula evaluated with fp32 torch on the CPU against float64 on the same input (4x: the accumulation order differs); those measured
fp32-reference errors are the FP32_REF_ERR table below -- never anything a kernel produced."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
KINK = 1e-4
EPS = 1e-5


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "non-finite values in kernel output"
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def check(name, got, ref, tol):
    """As test_ops_gpu.check: the stated tolerance, and 10x the error recorded in tests/golden/margins.json."""
    from conftest import calibrated_bound
    e = rel_err(got, ref)
    bound = calibrated_bound(name, e, tol)
    print("  %-44s rel-max-err %.3e (tol %.1e, held to %.1e)" % (name, e, tol, bound))
    assert e < bound, "%s: %.3e >= %.1e (stated tolerance %.1e)" % (name, e, bound, tol)


@pytest.fixture(scope="module")
def ops():
    from speechdrivestemplates_amd import ops as o
    return o


def f32(x):
    """float64 tensor holding fp32-representable values (what the kernel is given, exactly)"""
    return x.float().double()


# Measured on the CPU: rel-max-err of the same torch formula in fp32 against float64, on the very inputs of the named check, for the checks
# where 4x that error exceeds the inherited tolerance (tolerance used: 4x the figure).  All other checks keep the inherited tolerance.
FP32_REF_ERR = {
    # two rows per statistic: the two values can lie close together, |mean| / std is large and the normalised output ill-conditioned
    "code table grad D=24 B=3": 8.82e-06,
    "IN C=4 R=2 slope=0.2 dy": 2.23e-03,
    "IN C=4 R=2 slope=0.0 dy": 2.64e-03,
    "BN C=4 R=2 slope=0.2 dy": 1.14e-04,
    "BN C=4 R=2 slope=0.0 dy": 1.66e-04,
    "IN C=12 R=2 slope=0.2 dy": 2.44e-04,
    "IN C=12 R=2 slope=0.0 dy": 3.94e-04,
    "BN C=12 R=2 slope=0.2 dy": 2.82e-04,
    "BN C=12 R=2 slope=0.0 dy": 1.28e-04,
    "IN C=36 R=2 slope=0.2 z": 3.93e-05,
    "IN C=36 R=2 slope=0.0 z": 3.93e-05,
    "BN C=36 R=2 slope=0.2 dy": 3.93e-04,
    "BN C=36 R=2 slope=0.0 dy": 5.37e-04,
    "IN C=100 R=2 slope=0.2 z": 4.88e-06,
    "IN C=100 R=2 slope=0.2 dy": 2.20e-05,
    "IN C=100 R=2 slope=0.0 z": 4.88e-06,
    "IN C=100 R=2 slope=0.0 dy": 2.68e-05,
    "BN C=100 R=2 slope=0.2 z": 1.27e-05,
    "BN C=100 R=2 slope=0.2 dy": 5.91e-04,
    "BN C=100 R=2 slope=0.0 z": 1.27e-05,
    "BN C=100 R=2 slope=0.0 dy": 5.78e-04,
    "IN C=288 R=2 slope=0.2 z": 1.20e-05,
    "IN C=288 R=2 slope=0.2 dy": 2.62e-04,
    "IN C=288 R=2 slope=0.0 z": 1.20e-05,
    "IN C=288 R=2 slope=0.0 dy": 2.35e-04,
    "BN C=288 R=2 slope=0.2 dy": 1.32e-04,
    "BN C=288 R=2 slope=0.0 dy": 1.33e-04,
    "IN C=1020 R=2 slope=0.2 z": 2.64e-05,
    "IN C=1020 R=2 slope=0.2 dy": 1.74e-05,
    "IN C=1020 R=2 slope=0.0 z": 2.64e-05,
    "IN C=1020 R=2 slope=0.0 dy": 1.80e-05,
    "BN C=1020 R=2 slope=0.2 z": 2.35e-05,
    "BN C=1020 R=2 slope=0.2 dy": 4.67e-05,
    "BN C=1020 R=2 slope=0.0 z": 2.35e-05,
    "BN C=1020 R=2 slope=0.0 dy": 4.97e-05,
    "IN C=1024 R=2 slope=0.2 z": 3.05e-05,
    "IN C=1024 R=2 slope=0.2 dy": 2.00e-05,
    "IN C=1024 R=2 slope=0.0 z": 3.05e-05,
    "IN C=1024 R=2 slope=0.0 dy": 1.83e-05,
    "BN C=1024 R=2 slope=0.2 z": 1.57e-05,
    "BN C=1024 R=2 slope=0.0 z": 1.57e-05,
    "BN C=1024 R=2 slope=0.0 dy": 2.75e-05,
}


def tol_for(key, inherited):
    e32 = FP32_REF_ERR.get(key)
    return inherited if e32 is None else 4.0 * e32


def _off_kink(y, pre_acts, margin=KINK, exempt=None, spread=None):
    """Moves the inputs whose float64 pre-activation (any of ``pre_acts(y)``, each shaped like y) lies within 2 x margin of the activation's
    kink by 8 x margin x ``spread`` (the spread of the values that share a statistic; default: of all of y), i.e. the pre-activation by about
    8 x margin; a few rounds, since the statistics move a little with them."""
    if spread is None:
        spread = max(float(y.std()) if y.numel() > 1 else 0.0, 1.0)
    step = 8.0 * margin * spread
    for _ in range(50):
        bad = torch.zeros_like(y, dtype=torch.bool)
        for u in pre_acts(y):
            bad |= u.abs() < 2.0 * margin
        if exempt is not None:
            bad &= ~exempt
        if not bool(bad.any()):
            return y
        y = f32(torch.where(bad, y + step, y))
    raise AssertionError("inputs still on the kink")


# =============================================================================================================================
# 1. misc.hip
# =============================================================================================================================
ADAM_BIG = 4 * 1048576 + 4 * 4099 + 2  # 1 052 675 vectors: 4099 of them in the second grid-stride trip, and a 2-element scalar tail


def _adam_data(n, steps, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), [torch.randn(n, generator=g) for _ in range(steps)]


def adam_ref(p0, grads, lrs, dtype=torch.float64, wd=0.0, gscale=1.0, eps=1e-8):
    pr = p0.to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=lrs[0], weight_decay=wd, eps=eps)
    for lr, gr in zip(lrs, grads):
        opt.param_groups[0]["lr"] = lr
        pr.grad = gr.to(dtype) * gscale  # the reference gets the gradient already scaled
        opt.step()
    return pr.detach()


def _adam_gpu(ops, p0, grads, lrs, wd=0.0, gscale=1.0, eps=1e-8, m0=None, v0=None, step0=0):
    """-> (parameters after len(grads) kernel steps, step counter); asserts that the padding past n is untouched in all four buffers"""
    n = p0.numel()
    npad = (n + 3) // 4 * 4 + 8
    fill = {"p": 7.0, "g": 11.0, "m": 5.0, "v": 3.0}
    buf = {k: torch.full((npad,), s, device=DEV) for k, s in fill.items()}
    buf["p"][:n] = p0.to(DEV)
    buf["m"][:n] = 0.0 if m0 is None else m0.to(DEV)
    buf["v"][:n] = 0.0 if v0 is None else v0.to(DEV)
    lr = torch.zeros(1, device=DEV)
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    state[0] = step0
    for lr_k, gr in zip(lrs, grads):
        lr.fill_(lr_k)  # changed on the device between steps (what a scheduler does)
        buf["g"][:n] = gr.to(DEV)
        ops.adam_step(buf["p"][:n], buf["g"][:n], buf["m"][:n], buf["v"][:n], lr, state, eps=eps, weight_decay=wd, grad_scale=gscale)
    torch.cuda.synchronize()
    for k, s in fill.items():
        assert bool((buf[k][n:] == s).all()), "Adam wrote past n into the %s buffer" % k
    return buf["p"][:n], int(state[0].item())


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1027, ADAM_BIG])
def test_adam_sizes(ops, n):
    p0, grads = _adam_data(n, 3, 80 + n % 1000)
    got, step = _adam_gpu(ops, p0, grads, [1e-3] * 3)
    assert step == 3
    check("Adam n=%d" % n, got, adam_ref(p0, grads, [1e-3] * 3), tol_for("Adam n=%d" % n, 1e-6))


@pytest.mark.parametrize("variant", ["weight_decay", "grad_scale", "lr_changes"])
def test_adam_options(ops, variant):
    n = 1027
    p0, grads = _adam_data(n, 3, 91)
    kw = {"weight_decay": dict(wd=1e-2), "grad_scale": dict(gscale=0.5, eps=1e-2), "lr_changes": {}}[variant]
    # (Adam is invariant to the gradient's scale up to eps: eps = 1e-2 makes grad_scale count)
    lrs = [1e-3, 3e-3, 5e-4] if variant == "lr_changes" else [1e-3] * 3
    got, step = _adam_gpu(ops, p0, grads, lrs, **kw)
    assert step == 3
    check("Adam " + variant, got, adam_ref(p0, grads, lrs, **kw), tol_for("Adam " + variant, 1e-6))
    if variant != "lr_changes":  # the option is not a no-op: it moves the parameters by far more than the tolerance
        plain = adam_ref(p0, grads, lrs, eps=kw.get("eps", 1e-8))
        assert rel_err(plain, adam_ref(p0, grads, lrs, **kw)) > 1e-5


def test_adam_bias_correction_at_step_1000(ops):
    """Steps 1000..1002 (bias corrections 1 - 0.9^t ~ 1, 1 - 0.999^t ~ 0.63): the state of a float64 Adam that has run 999 steps on a
    1027-element problem, rounded to fp32 on both sides, then three steps of each."""
    n = 1027
    p0, grads = _adam_data(n, 1002, 97)
    pr = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=1e-3)
    for gr in grads[:999]:
        pr.grad = gr.double()
        opt.step()
    st = opt.state[pr]
    assert int(st["step"]) == 999
    with torch.no_grad():
        for t in (pr, st["exp_avg"], st["exp_avg_sq"]):
            t.copy_(f32(t))
    start, m0, v0 = pr.detach().float(), st["exp_avg"].float(), st["exp_avg_sq"].float()
    for gr in grads[999:]:
        pr.grad = gr.double()
        opt.step()
    got, step = _adam_gpu(ops, start, grads[999:], [1e-3] * 3, m0=m0, v0=v0, step0=999)
    assert step == 1002
    check("Adam steps 1000-1002", got, pr.detach(), tol_for("Adam steps 1000-1002", 1e-6))


# ---------------------------------------------------------------------------------------------
L1_LAM, L1_UP = 0.7, 1.7


@functools.lru_cache(maxsize=None)
def l1_data(n):
    g = torch.Generator().manual_seed(500 + n % 997)
    pred, gt = torch.randn(n, generator=g), torch.randn(n, generator=g)
    k = min(5, n // 2)
    gt[:k] = pred[:k]  # exact ties: sign(0) = 0
    return pred, gt


def l1_ref(pred, gt, dtype=torch.float64):
    pr = pred.to(dtype).clone().requires_grad_(True)
    loss = (torch.abs(pr - gt.to(dtype)) * L1_LAM).mean()
    (loss * L1_UP).backward()
    return loss.detach(), pr.grad


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65536 + 777, 1048576 + 513])
def test_l1_sizes(ops, n):
    pred, gt = l1_data(n)
    loss, grad = l1_ref(pred, gt)
    pd = pred.to(DEV).requires_grad_(True)
    ld = ops.L1LossFn.apply(pd, gt.to(DEV), L1_LAM)
    (ld * L1_UP).backward()
    check("L1 loss n=%d" % n, ld, loss, tol_for("L1 loss n=%d" % n, 1e-6))
    check("L1 grad n=%d" % n, pd.grad, grad, tol_for("L1 grad n=%d" % n, 1e-6))
    k = min(5, n // 2)
    assert bool((pd.grad[:k] == 0).all())


# ---------------------------------------------------------------------------------------------
MSE_LAM, MSE_UP = 0.5, 1.5


@functools.lru_cache(maxsize=None)
def mse_data(n):
    return torch.randn(n, generator=torch.Generator().manual_seed(600 + n % 997))


def mse_ref(s, target, dtype=torch.float64):
    sr = s.to(dtype).clone().requires_grad_(True)
    loss = F.mse_loss(sr, torch.full_like(sr, target)) * MSE_LAM
    (loss * MSE_UP).backward()
    return loss.detach(), sr.grad


@pytest.mark.parametrize("target", [0.0, 1.0])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000, 1048576 + 513])
def test_mse_const_sizes(ops, n, target):
    s = mse_data(n)
    loss, grad = mse_ref(s, target)
    sd = s.to(DEV).requires_grad_(True)
    out = ops.MseConstFn.apply(sd, target, MSE_LAM)
    (out * MSE_UP).backward()
    tag = "n=%d target=%g" % (n, target)
    check("MSE-const loss " + tag, out.reshape(1), loss.reshape(1), tol_for("MSE-const loss " + tag, 1e-6))
    check("MSE-const grad " + tag, sd.grad, grad, tol_for("MSE-const grad " + tag, 1e-6))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2, 1), (2, 2, 242), (3, 5, 3), (5, 1000, 242)], ids=str)
def test_time_diff_shapes(ops, shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g).double().requires_grad_(True)
    y = x[:, 1:] - x[:, :-1]
    gy = f32(torch.randn(y.shape, generator=g, dtype=torch.float64))
    y.backward(gy)
    xd = x.detach().float().to(DEV).requires_grad_(True)
    yd = ops.TimeDiffFn.apply(xd)
    yd.backward(gy.float().to(DEV))
    check("time diff fwd %s" % (shape,), yd, y, 1e-6)
    check("time diff bwd %s" % (shape,), xd.grad, x.grad, 1e-6)


# ---------------------------------------------------------------------------------------------
KL_N, KL_LAM, KL_UP = 50, 0.1, 1.3


@functools.lru_cache(maxsize=None)
def kl_data(D, B):
    g = torch.Generator().manual_seed(1000 * D + B)
    table = f32(torch.randn(KL_N, D, generator=g, dtype=torch.float64) * 0.7)
    if B <= KL_N:
        idx = torch.randperm(KL_N, generator=g)[:B]
        if B == 3:
            idx[2] = idx[0]  # the same clip twice in a batch: its gradient rows add up
    else:
        idx = torch.randint(0, KL_N, (B,), generator=g)  # B > N: the indices necessarily repeat
    return table, idx, f32(torch.randn(B, D, generator=g, dtype=torch.float64))


def kl_ref(table, idx, gcode, dtype=torch.float64):
    from oracle import sdt_oracle as O
    tr = table.to(dtype).clone().requires_grad_(True)
    code = tr[idx]
    kl = O.clip_code_kl(code, KL_LAM)
    (kl * KL_UP + (code * gcode.to(dtype)).sum()).backward()
    return code.detach(), kl.detach(), tr.grad


@pytest.mark.parametrize("B", [2, 3, 65, 300])
@pytest.mark.parametrize("D", [1, 3, 24, 33, 100, 256])
def test_code_gather_kl_shapes(ops, D, B):
    table, idx, gcode = kl_data(D, B)
    code, kl, grad = kl_ref(table, idx, gcode)
    td = torch.nn.Parameter(table.float().to(DEV))
    cd, kd, valid = ops.CodeGatherKLFn.apply(td, idx.to(DEV), KL_LAM)
    (kd * KL_UP + (cd * gcode.float().to(DEV)).sum()).backward()
    assert int(valid.item()) == 1
    tag = "D=%d B=%d" % (D, B)
    check("code gather " + tag, cd, code, 1e-7)
    check("code KL " + tag, kd.reshape(1), kl.reshape(1), tol_for("code KL " + tag, 1e-5))
    check("code table grad " + tag, td.grad, grad, tol_for("code table grad " + tag, 1e-5))


def test_code_kl_rejects_more_than_256_dimensions(ops):
    td = torch.zeros(KL_N, 257, device=DEV)
    with pytest.raises(RuntimeError, match="libsdt_hip"):
        ops.CodeGatherKLFn.apply(td, torch.tensor([0, 1, 2], device=DEV), KL_LAM)


def test_rows_scatter_add_drops_rows_outside_the_table(ops):
    """B * D = 259 (a second, partly filled workgroup), two clips that appear twice, one index past the table and one negative: both are
    dropped.  The table is a slice of a larger buffer whose other elements (8 rows on either side) must keep their fill value."""
    from speechdrivestemplates_amd import _lib
    N, B, D, G = 20, 7, 37, 8
    g = torch.Generator().manual_seed(77)
    src = f32(torch.randn(B, D, generator=g, dtype=torch.float64))
    idx = torch.tensor([5, N + 2, 5, 0, -2, 19, 0])
    buf = torch.full(((N + 2 * G) * D,), 3.0, device=DEV)
    dst = buf[G * D:(G + N) * D]
    dst.zero_()
    sd, idd = src.float().to(DEV), idx.to(DEV)
    _lib.check(_lib.load().sdt_rows_scatter_add_f32(ops._p(sd), ops._p(idd), ops._p(dst), N, B, D, ops._stream()))
    torch.cuda.synchronize()
    ref = torch.zeros(N, D, dtype=torch.float64)
    ok = (idx >= 0) & (idx < N)
    ref.index_add_(0, idx[ok], src[ok])
    # a row appears at most twice: 0 + a is exact and a + b is one fp32 rounding, 2^-24 |a + b| <= 6e-8 max|ref|
    check("rows scatter-add", dst.reshape(N, D), ref, 1e-7)
    assert bool((buf[:G * D] == 3.0).all()) and bool((buf[(G + N) * D:] == 3.0).all())


# ---------------------------------------------------------------------------------------------
def _metric_inputs(B, T, K, seed):
    g = torch.Generator().manual_seed(seed)
    pred, gt = torch.randn(B, T, 2, K, generator=g), torch.randn(B, T, 2, K, generator=g)
    stat = {"mean": torch.randn(B, 2 * K, generator=g, dtype=torch.float64) * 50.0,
            "std": torch.rand(B, 2 * K, generator=g, dtype=torch.float64) * 20.0 + 5.0,
            "scale_factor": torch.rand(B, generator=g, dtype=torch.float64) + 0.5}
    return pred, gt, stat


def _metrics_gpu(ops, pred, gt, stat, hier, want_final=True):
    return ops.final_metrics(pred.to(DEV), gt.to(DEV), stat["mean"].to(DEV), stat["std"].to(DEV), stat["scale_factor"].to(DEV), hier,
                             want_final=want_final)


@pytest.mark.parametrize("B,T", [(1, 1), (1, 5), (33, 13), (70, 8), (4, 64)])
def test_final_metrics_hierarchical_batches(ops, B, T):
    from oracle import sdt_oracle as O
    pred, gt, stat = _metric_inputs(B, T, 121, 7000 + 100 * B + T)
    fp, fg = O.get_final_results(pred.clone(), stat, True), O.get_final_results(gt.clone(), stat, True)
    m = O.evaluate_step(fp, fg)
    dfp, dfg, dm = _metrics_gpu(ops, pred, gt, stat, True)
    tag = " B=%d T=%d" % (B, T)
    check("final pred" + tag, dfp, fp, 1e-12)
    check("final gt" + tag, dfg, fg, 1e-12)
    check("L2_dist" + tag, dm[0], m["L2_dist"], 1e-10)
    check("lip_sync_error_n" + tag, dm[1], m["lip_sync_error_n"], 1e-10)
    n0, n1, dm2 = _metrics_gpu(ops, pred, gt, stat, True, want_final=False)
    assert n0 is None and n1 is None and torch.equal(dm2, dm)


@pytest.mark.parametrize("K", [1, 64, 75, 76, 128])
def test_final_metrics_plain_keypoint_counts(ops, K):
    """Not hierarchical, B = 33 > the 32 clips of one reduce trip, T = 13: de-normalise, scale, mean keypoint distance in float64.  The lip
    term needs landmarks 71 and 75: the kernel documents 0 for K <= 75 (the reference's evaluate_step would raise IndexError there)."""
    from oracle import sdt_oracle as O
    B, T = 33, 13
    pred, gt, stat = _metric_inputs(B, T, K, 7100 + K)
    sd, mu = stat["std"].reshape(B, 1, 2, K), stat["mean"].reshape(B, 1, 2, K)
    sc = stat["scale_factor"].reshape(B, 1, 1, 1)
    fp, fg = (pred.double() * sd + mu) * sc, (gt.double() * sd + mu) * sc
    l2 = ((fp - fg) ** 2).sum(2).sqrt().mean()
    dfp, dfg, dm = _metrics_gpu(ops, pred, gt, stat, False)
    tag = " K=%d" % K
    check("final pred" + tag, dfp, fp, 1e-12)
    check("final gt" + tag, dfg, fg, 1e-12)
    check("L2_dist" + tag, dm[0], l2, 1e-10)
    if K > 75:
        m = O.evaluate_step(fp, fg)
        check("L2_dist vs evaluate_step" + tag, dm[0], m["L2_dist"], 1e-10)
        check("lip_sync_error_n" + tag, dm[1], m["lip_sync_error_n"], 1e-10)
    else:
        assert float(dm[1].item()) == 0.0
    n0, n1, dm2 = _metrics_gpu(ops, pred, gt, stat, False, want_final=False)
    assert n0 is None and n1 is None and torch.equal(dm2, dm)


def test_final_metrics_argument_checks(ops):
    with pytest.raises(RuntimeError, match="libsdt_hip"):
        _metrics_gpu(ops, *_metric_inputs(2, 3, 129, 1), False)
    with pytest.raises(RuntimeError, match="libsdt_hip"):
        _metrics_gpu(ops, *_metric_inputs(2, 3, 64, 2), True)


# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mel_consts(ops):
    from oracle import sdt_oracle as O
    return {"basis": ops.dft_basis(O.mel_window()).to(DEV), "fb": O.mel_filterbank().to(DEV),
            "w64": O.mel_window(torch.float64), "fb64": O.mel_filterbank(torch.float64)}


@functools.lru_cache(maxsize=None)
def mel_audio(L):
    audio = 0.1 * torch.randn(3, L, generator=torch.Generator().manual_seed(L))
    t = torch.arange(L) / 16000.0
    audio[1] += 0.3 * torch.sin(2 * math.pi * (200 + 1500 * t) * t)  # chirp
    return audio


# F = 1 + L // 160: 2, 3, 4, 15 (F % 16 = 15), 16 (0), 17 (1), 101, 313
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", [257, 400, 512, 2399, 2400, 2560, 16000, 50001])
def test_mel_lengths(ops, mel_consts, L, B):
    from oracle import sdt_oracle as O
    audio = mel_audio(L)[:B]
    ref = O.mel_spectrogram(audio.double(), mel_consts["w64"], mel_consts["fb64"])
    mel = ops.mel_spectrogram(audio.to(DEV), mel_consts["basis"], mel_consts["fb"])
    assert mel.shape == (B, 80, 1 + L // 160)
    check("mel L=%d B=%d" % (L, B), mel, ref, tol_for("mel L=%d B=%d" % (L, B), 2e-5))
    zero = ops.mel_spectrogram(torch.zeros(B, L, device=DEV), mel_consts["basis"], mel_consts["fb"])
    assert int(torch.count_nonzero(zero)) == 0


def test_mel_rejects_clips_not_longer_than_the_reflect_pad(ops, mel_consts):
    with pytest.raises(RuntimeError, match="libsdt_hip"):
        ops.mel_spectrogram(torch.zeros(2, 256, device=DEV), mel_consts["basis"], mel_consts["fb"])


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", [1, 255, 16385, 68267])
def test_rows_gather_columns(ops, n_cols):
    from speechdrivestemplates_amd import _lib
    N, G = 6, 2
    big = torch.randn(N + 2 * G, n_cols, generator=torch.Generator().manual_seed(n_cols))
    bigd = big.to(DEV)
    src, srcd = big[G:G + N], bigd[G:G + N]  # rows on either side belong to the same allocation
    idx = torch.tensor([4, 0, 4, 5, 1, 3, 2, 2])
    got = ops.rows_gather(srcd, idx.to(DEV))
    assert torch.equal(got.cpu(), src[idx])
    # an index outside the store never touches memory: its destination row keeps what it held
    bad = torch.tensor([3, N + 1, 0, -1])
    dst = torch.full((4, n_cols), -77.0, device=DEV)
    badd = bad.to(DEV)
    _lib.check(_lib.load().sdt_rows_gather_f32(ops._p(srcd), ops._p(badd), ops._p(dst), N, 4, n_cols, ops._stream()))
    torch.cuda.synchronize()
    want = torch.full((4, n_cols), -77.0)
    want[0], want[2] = src[3], src[0]
    assert torch.equal(dst.cpu(), want)


@pytest.mark.parametrize("hier", [0, 1])
@pytest.mark.parametrize("extra", [0, 7])
def test_clip_poses_prepare_layouts(ops, extra, hier):
    """B = 3 with one clip twice, stored clips of T or T + 7 frames: bit-identical to the host transforms of GestureDataset.__getitem__
    (the bar tests/test_dataset.py holds DeviceClipStore to)."""
    from speechdrivestemplates_amd import _lib
    from speechdrivestemplates_amd.config import get_cfg_defaults
    from speechdrivestemplates_amd.core.datasets.gesture_dataset import GestureDataset
    N, T, G = 4, 6, 1
    Ts = T + extra
    g = torch.Generator().manual_seed(10 * extra + hier)
    big = torch.randn(N + 2 * G, Ts, 3, 137, generator=g) * 100.0 + 300.0
    mean, std = torch.randn(242, generator=g) * 20.0, torch.rand(242, generator=g) * 30.0 + 5.0
    raw = big[G:G + N]
    ds = GestureDataset(root_dir=None, cfg=get_cfg_defaults())

    def host(i):
        p = ds.absolute_to_relative(ds.remove_unuesd_kp(raw[i, :T].clone()))
        if hier:
            p = ds.global_to_parted(p)
        return (p[:, :2, :] - mean.reshape(1, 2, 121)) / std.reshape(1, 2, 121), p[:, 2:, :].repeat(1, 2, 1)

    idx = torch.tensor([2, 0, 2])
    rawd = big.to(DEV)[G:G + N]
    poses, score = ops.clip_poses_prepare(rawd, idx.to(DEV), mean.to(DEV), std.to(DEV), T, hier)
    for j, i in enumerate(idx.tolist()):
        hp, hs = host(i)
        assert torch.equal(poses[j].cpu(), hp) and torch.equal(score[j].cpu(), hs), (j, i)
    # an index outside the store: that clip's output rows keep what they held
    bad = torch.tensor([N, 1, -1]).to(DEV)
    po, so = torch.full((3, T, 2, 121), -77.0, device=DEV), torch.full((3, T, 2, 121), -55.0, device=DEV)
    md, sdv = mean.to(DEV), std.to(DEV)
    _lib.check(_lib.load().sdt_clip_poses_prepare_f32(ops._p(rawd), ops._p(bad), ops._p(md), ops._p(sdv), ops._p(po), ops._p(so),
                                                      N, Ts, 3, T, hier, ops._stream()))
    torch.cuda.synchronize()
    hp, hs = host(1)
    assert torch.equal(po[1].cpu(), hp) and torch.equal(so[1].cpu(), hs)
    assert bool((po[[0, 2]] == -77.0).all()) and bool((so[[0, 2]] == -55.0).all())


def test_resize_concat_needs_one_code_row_per_clip(ops, monkeypatch):
    """ResizeConcatFn builds its own row index arange(B) (no clip index reaches resize_concat_fwd_kernel, which has no guard), so the
    only way to make it read past the code is a code with fewer rows than clips: refused on the host, before any launch."""
    from speechdrivestemplates_amd import _lib
    lib = _lib.load()

    def no_launch(*a):
        raise AssertionError("launched")
    monkeypatch.setattr(lib, "sdt_resize_concat_fwd_f32", no_launch)
    x = torch.zeros(3, 2, 5, 8, device=DEV)
    for code in (torch.zeros(2, 4, device=DEV), torch.zeros(4, 4, device=DEV), torch.zeros(12, device=DEV)):
        with pytest.raises(ValueError, match="one code row per clip"):
            ops.ResizeConcatFn.apply(x, code, 4)


# =============================================================================================================================
# 2. norm.hip (fp32 tensors)
# =============================================================================================================================
NORM_C = [4, 12, 36, 100, 288, 1020, 1024]
SLOPES = (0.2, 0.0)


def _act(u, slope):
    return F.leaky_relu(u, slope) if slope else F.relu(u)


def _colnorm_cases():
    """(kind, C, R): R in {1 (BatchNorm only), 2, 3, 4, 5, rpp - 1, 4 rpp + 1, 1000} with rpp = 256 // (C / 4) rows per pass of a workgroup,
    without the values that repeat an earlier one (or are < 1)"""
    out = []
    for C in NORM_C:
        rpp = 256 // (C // 4)
        seen = []
        for R in (1, 2, 3, 4, 5, rpp - 1, 4 * rpp + 1, 1000):  # 4 | 5: colstats_kernel's fp64 | fp32 partial sums
            if R < 1 or R in seen:
                continue
            seen.append(R)
            out += [(kind, C, R) for kind in ("IN", "BN") if not (kind == "IN" and R == 1)]
    return out


def in_pre(y):
    """y (G, R, C) channels-last -> InstanceNorm2d output (statistics per (g, c) over R)"""
    return F.instance_norm(y.permute(0, 2, 1), eps=EPS).permute(0, 2, 1)


def bn_pre(y, gamma, beta, rm, rv):
    """training-mode BatchNorm of y (1, R, C) channels-last; rm / rv are updated in place.  One row: F.batch_norm refuses it; the kernel
    documents biased variance 0 and the unbiased factor R / (R - 1) replaced by 1."""
    R = y.shape[1]
    if R > 1:
        return F.batch_norm(y.permute(0, 2, 1), rm, rv, gamma, beta, True, 0.1, EPS).permute(0, 2, 1)
    mean, var = y.mean((0, 1)), y.var((0, 1), unbiased=False)
    with torch.no_grad():
        rm.mul_(0.9).add_(0.1 * mean)
        rv.mul_(0.9).add_(0.1 * var)
    return (y - mean) / torch.sqrt(var + EPS) * gamma + beta


def bn_eval(y, gamma, beta, rm, rv):
    return F.batch_norm(y.permute(0, 2, 1), rm, rv, gamma, beta, False, 0.1, EPS).permute(0, 2, 1)


@functools.lru_cache(maxsize=None)
def colnorm_data(kind, C, R, rho=None, margin=KINK, rnd=f32, off_kink=_off_kink):
    """Inputs of one column-norm case (float64, fp32-representable, clear of the kink).  ``rho``: per-channel mean = rho x std.
    ``rnd`` / ``off_kink``: the rounding of y and dz (the affine parameters stay fp32) and the matching way off the kink (test_edge_shapes_bf16_gpu.py: bf16-representable
    inputs, moved by whole bf16 steps)."""
    G = 1 if kind == "BN" else (3 if rho is None else 2)
    g = torch.Generator().manual_seed(7 * C + R + (0 if kind == "IN" else 100000) + (0 if rho is None else 1000 * int(rho) + 17))
    y = torch.randn(G, R, C, generator=g, dtype=torch.float64)
    if rho is None:
        y = y * 3.0 + 1.5
    else:
        sd = 0.5 + torch.rand(C, generator=g, dtype=torch.float64) * 2.0
        y = (y + rho) * sd
    y = rnd(y)
    gz = rnd(torch.randn(G, R, C, generator=g, dtype=torch.float64))
    d = {"y": y, "gz": gz, "G": G}
    if kind == "BN":
        d["gamma"] = f32(1 + 0.1 * torch.randn(C, generator=g, dtype=torch.float64))
        b = torch.randn(C, generator=g, dtype=torch.float64)
        d["beta"] = f32(torch.sign(b) * (0.02 + 0.1 * b.abs()))  # |beta| >= 0.02: with one row the pre-activation IS beta

        def pre(yy):
            rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
            u = bn_pre(yy, d["gamma"], d["beta"], rm, rv)
            return u, bn_eval(yy, d["gamma"], d["beta"], rm, rv)
    else:
        def pre(yy):
            return (in_pre(yy),)
    d["y"] = off_kink(y, pre, margin, spread=None if rho is None else 2.5)
    return d


def colnorm_ref(kind, d, slope, dtype=torch.float64):
    """-> dict of the reference's outputs for one slope (z, dy; BatchNorm: dgamma, dbeta, running statistics, eval output, and the
    pre-activations u / ue for the kink assertion)"""
    y = d["y"].to(dtype).clone().requires_grad_(True)
    C = y.shape[-1]
    if kind == "IN":
        u = in_pre(y)
        z = _act(u, slope)
        z.backward(d["gz"].to(dtype))
        return {"u": u.detach(), "z": z.detach(), "dy": y.grad}
    gamma, beta = d["gamma"].to(dtype).clone().requires_grad_(True), d["beta"].to(dtype).clone().requires_grad_(True)
    rm, rv = torch.zeros(C, dtype=dtype), torch.ones(C, dtype=dtype)
    u = bn_pre(y, gamma, beta, rm, rv)
    z = _act(u, slope)
    z.backward(d["gz"].to(dtype))
    ue = bn_eval(y.detach(), gamma.detach(), beta.detach(), rm, rv)
    return {"u": u.detach(), "ue": ue, "z": z.detach(), "dy": y.grad, "dgamma": gamma.grad, "dbeta": beta.grad, "rm": rm, "rv": rv,
            "ze": F.leaky_relu(ue, slope)}


# inherited: norm forward / running statistics / eval 1e-5, InstanceNorm backward 2e-5, BatchNorm backward 5e-5
NORM_TOL = {"IN": {"z": 1e-5, "dy": 2e-5},
            "BN": {"z": 1e-5, "dy": 5e-5, "dgamma": 5e-5, "dbeta": 5e-5, "rm": 1e-5, "rv": 1e-5, "ze": 1e-5}}


@pytest.mark.parametrize("kind,C,R", _colnorm_cases(), ids=lambda v: str(v))
def test_colnorm_edge_shapes(ops, kind, C, R):
    """Two and three rows per statistic are where the one-pass variance is at its worst (among C random pairs some lie close together, mean/std
    = 60 ... 20 000): with fp32 squares these cases missed the forward bar by up to two decades (9.5e-3 at C = 1020, R = 2); colstats_kernel
    carries the sums of at most four rows in fp64 since."""
    d = colnorm_data(kind, C, R)
    G = d["G"]
    for slope in SLOPES:
        ref = colnorm_ref(kind, d, slope)
        assert float(ref["u"].abs().min()) >= KINK and (kind == "IN" or float(ref["ue"].abs().min()) >= KINK)
        yd = d["y"].float().to(DEV).requires_grad_(True)
        got = {}
        if kind == "IN":
            zd = ops.ColNormActFn.apply(yd, None, None, None, None, None, G, slope)
        else:
            gd, bd = torch.nn.Parameter(d["gamma"].float().to(DEV)), torch.nn.Parameter(d["beta"].float().to(DEV))
            rmd, rvd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
            nbt = torch.zeros((), dtype=torch.int64, device=DEV)
            zd = ops.ColNormActFn.apply(yd, gd, bd, rmd, rvd, nbt, 1, slope)
        zd.backward(d["gz"].float().to(DEV))
        got["z"], got["dy"] = zd, yd.grad
        if kind == "BN":
            assert int(nbt.item()) == 1
            got.update(dgamma=gd.grad, dbeta=bd.grad, rm=rmd, rv=rvd,
                       ze=ops.colnorm_eval(yd.detach(), gd.detach(), bd.detach(), rmd, rvd, slope))
        for q, tol in NORM_TOL[kind].items():
            key = "%s C=%d R=%d slope=%.1f %s" % (kind, C, R, slope, q)
            if R == 1 and q == "dy":
                # one row: dy = gamma rstd (g - mean(g)) is exactly 0 in the reference, so there is no magnitude to be relative to;
                # the kernel may keep the one fp32 rounding of g = dz act'(u): |dy| <= 2^-24 max|dz| max|gamma| / sqrt(eps)
                assert float(ref[q].abs().max()) == 0.0
                bound = 2.0 ** -24 * float(d["gz"].abs().max() * d["gamma"].abs().max()) / math.sqrt(EPS)
                e = float(got[q].abs().max())
                print("  %-44s max-abs %.3e (bound %.1e)" % (key, e, bound))
                assert math.isfinite(e) and e <= bound, (key, e, bound)
                continue
            check(key, got[q], ref[q], tol_for(key, tol))


# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rownorm_data(C, rows):
    g = torch.Generator().manual_seed(31 * C + rows)
    y = f32(torch.randn(1, rows, C, generator=g, dtype=torch.float64) * 2 + 0.3)
    const = torch.zeros(1, rows, C, dtype=torch.bool)
    if rows >= 3:
        y[0, 1] = -0.75  # an exactly constant row: variance 0, pre-activation exactly 0 (on the kink by construction: exempt below)
        const[0, 1] = True
    y = _off_kink(y, lambda yy: (F.instance_norm(yy, eps=EPS),), exempt=const)
    return y, f32(torch.randn(1, rows, C, generator=g, dtype=torch.float64)), const


def rownorm_ref(y, gz, dtype=torch.float64, slope=0.2):
    yr = y.to(dtype).clone().requires_grad_(True)
    u = F.instance_norm(yr, eps=EPS)  # (1, rows, C): the reference's InstanceNorm1d on the permuted tensor, per row over C
    z = _act(u, slope)
    z.backward(gz.to(dtype))
    return u.detach(), z.detach(), yr.grad


@pytest.mark.parametrize("rows", [1, 3, 257])
@pytest.mark.parametrize("C", NORM_C)
def test_rownorm_edge_shapes(ops, C, rows):
    y, gz, const = rownorm_data(C, rows)
    u, z, dy = rownorm_ref(y, gz)
    assert float(u[~const].abs().min()) >= KINK
    yd = y.float().to(DEV).requires_grad_(True)
    zd = ops.RowNormActFn.apply(yd, 0.2)
    zd.backward(gz.float().to(DEV))
    tag = "C=%d rows=%d" % (C, rows)
    check("rownorm fwd " + tag, zd, z, tol_for("rownorm fwd " + tag, 1e-5))
    check("rownorm bwd " + tag, yd.grad, dy, tol_for("rownorm bwd " + tag, 2e-5))
    if rows >= 3:
        # the constant row: the mean of C equal values is that value, so the output is exactly 0 and the gradient takes the slope of u = 0
        assert bool((u[0, 1] == 0).all()) and bool((zd[0, 1] == 0).all())
        assert bool(torch.isfinite(yd.grad[0, 1]).all())
        check("rownorm bwd, constant row " + tag, yd.grad[0, 1], dy[0, 1], tol_for("rownorm bwd const " + tag, 2e-5))


@functools.lru_cache(maxsize=None)
def slabs_data(nslab, C, rows=5):
    g = torch.Generator().manual_seed(13 * nslab + C)
    part = f32(torch.randn(nslab, rows, C, generator=g, dtype=torch.float64))
    pre = lambda p: (F.instance_norm(p.sum(0, keepdim=True), eps=EPS).expand(nslab, rows, C),)  # noqa: E731
    return _off_kink(part, pre)


@pytest.mark.parametrize("C", [12, 256])
@pytest.mark.parametrize("nslab", [1, 2, 64])
def test_rownorm_slabs(ops, nslab, C):
    """sdt_rownorm_slabs_fwd_f32 = RowNormActFn on the sum of the split-K slabs; it also stores that sum (slab order, fp32)."""
    from speechdrivestemplates_amd import _lib
    rows = 5
    part = slabs_data(nslab, C)
    u = F.instance_norm(part.sum(0, keepdim=True), eps=EPS)
    assert float(u.abs().min()) >= KINK
    pd = part.float().to(DEV)
    y, z = torch.empty(rows, C, device=DEV), torch.empty(rows, C, device=DEV)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    _lib.check(_lib.load().sdt_rownorm_slabs_fwd_f32(ops._p(pd), nslab, ops._p(y), ops._p(z), ops._p(mean), ops._p(rstd), rows, C, EPS, 0.2,
                                                     ops._stream()))
    torch.cuda.synchronize()
    acc = part[0].float()
    for s in range(1, nslab):
        acc = acc + part[s].float()
    assert torch.equal(y.cpu(), acc)  # summed in slab order
    tag = "nslab=%d C=%d" % (nslab, C)
    # a sequential fp32 sum of n terms is within (n - 1) 2^-24 sum|x_i| of the exact one
    ysum_tol = (nslab - 1) * 2.0 ** -24 * float(part.abs().sum(0).max() / part.sum(0).abs().max()) + 1e-12
    check("slabs summed y " + tag, y, part.sum(0), ysum_tol)
    check("slabs rownorm fwd " + tag, z.reshape(1, rows, C), F.leaky_relu(u, 0.2), tol_for("slabs rownorm fwd " + tag, 1e-5))
    z2 = ops.RowNormActFn.apply(y.reshape(1, rows, C), 0.2)
    assert torch.equal(z2.reshape(rows, C), z)


# ---------------------------------------------------------------------------------------------
# One-pass variance q/R - m^2 with fp32 per-thread partials: its first-order error relative to the variance is 2^-24 (1 + rho^2) per
# rounding, rho = |mean| / std.  Bound asserted for rho in {0, 8}: max(inherited 1e-5, 4 x 2^-24 x (1 + rho^2)) (1.6e-5 at rho = 8);
# rho = 64 is recorded only (DESIGN.md states the measured figure as the kernel's limit).
@pytest.mark.parametrize("rho", [0, 8, 64])
@pytest.mark.parametrize("kind,R", [("IN", 1000), ("BN", 8520)])
def test_colnorm_large_mean_over_std(ops, kind, R, rho):
    C = 64
    d = colnorm_data(kind, C, R, rho=float(rho), margin=2e-3 if rho == 64 else KINK)
    ref = colnorm_ref(kind, d, 0.2)
    assert float(ref["u"].abs().min()) >= KINK
    yd = d["y"].float().to(DEV).requires_grad_(True)
    if kind == "IN":
        zd = ops.ColNormActFn.apply(yd, None, None, None, None, None, d["G"], 0.2)
    else:
        zd = ops.ColNormActFn.apply(yd, d["gamma"].float().to(DEV), d["beta"].float().to(DEV), torch.zeros(C, device=DEV),
                                    torch.ones(C, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV), 1, 0.2)
    rstd = zd.grad_fn.saved_tensors[2]
    assert bool(torch.isfinite(zd).all()) and bool(torch.isfinite(rstd).all()) and bool((rstd > 0).all())
    e = rel_err(zd, ref["z"])
    print("  colnorm %s R=%d mean = %d x std: forward rel-max-err %.3e" % (kind, R, rho, e))
    if rho != 64:
        check("%s R=%d rho=%d fwd" % (kind, R, rho), zd, ref["z"], max(1e-5, 4.0 * 2.0 ** -24 * (1 + rho * rho)))
    else:
        from conftest import calibrated_bound
        calibrated_bound("%s R=%d rho=64 fwd (recorded)" % (kind, R), e, float("inf"))


def test_norm_argument_checks(ops):
    for C in (6, 1028):
        x = torch.zeros(2, 4, C, device=DEV)
        with pytest.raises(RuntimeError, match="libsdt_hip"):
            ops.RowNormActFn.apply(x, 0.2)
        with pytest.raises(RuntimeError, match="libsdt_hip"):
            ops.ColNormActFn.apply(x, None, None, None, None, None, 2, 0.2)
        with pytest.raises(RuntimeError, match="libsdt_hip"):
            ops.colnorm_eval(x, None, None, torch.zeros(C, device=DEV), torch.ones(C, device=DEV), 0.2)
    # affine gradients with more than one statistics group
    y = torch.randn(3, 5, 8, device=DEV).requires_grad_(True)
    gamma, beta = torch.nn.Parameter(torch.ones(8, device=DEV)), torch.nn.Parameter(torch.zeros(8, device=DEV))
    z = ops.ColNormActFn.apply(y, gamma, beta, None, None, None, 3, 0.2)
    with pytest.raises(RuntimeError, match="libsdt_hip"):
        z.backward(torch.ones_like(z))
