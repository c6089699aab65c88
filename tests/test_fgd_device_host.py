"""The device FGD's contract (csrc/fgd.hip) restated in float64 numpy -- shifted moments, Chan's pairwise merge, the
symmetric eigen route -- and held against (1) the reference's own outputs in tests/golden/fgd.npz at the bar test_geometry.py uses for that
fixture and (2) compute_fgd (scipy sqrtm) on the seeded full-rank sets of tests/golden/synth_fgd_sets.py.  No GPU needed.

The restatement's error against compute_fgd per case is recorded in profiles/r09_fgd_host_error.txt (SDT_RECORD_FGD=1 rewrites it);
tests/test_fgd_gpu.py holds the kernels, which differ from the restatement by summation order and Jacobi-vs-LAPACK only, to 100 x that error.

HOST_BAR: both routes are backward-stable float64 algorithms on matrices of order <= 64; tr (C_A C_B)^(1/2) = sum sqrt(mu_i) moves by
|d mu_i| / (2 sqrt(mu_i)), so a backward error of order 64 eps ||C_A|| ||C_B|| shows up amplified by at most sqrt(cond) of the product, about
1e2 for these sets (column scales 1.5 .. 0.5 on both sides, mild mixing): 64 x 2.2e-16 x 1e2 ~ 1.4e-12 of the scale tr C_A + tr C_B + gap^2.
The bar allows 1e-10 of that scale: two decades over the estimate, five below the fixture bar.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO

sys.path.insert(0, GOLDEN)
import synth_fgd_sets as S  # noqa: E402

HOST_ERROR_FILE = os.path.join(REPO, "profiles", "r09_fgd_host_error.txt")
HOST_BAR = 1e-10
FIXTURE_TAGS = ("n200_d32", "n20_d32", "n500_d32", "n64_d64")


# -- the contract in numpy --------------------------------------------------------------------------------------------------------------------------
def contract_state(x, state=None):
    """rows of the float32 (n, d) array ``x`` added to a state {n, shift, s1, s2}: moments about the first row the state ever saw"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    if state is None:
        state = dict(n=0, shift=x[0].copy(), s1=np.zeros(x.shape[1]), s2=np.zeros((x.shape[1], x.shape[1])))
    c = x - state["shift"]
    return dict(n=state["n"] + x.shape[0], shift=state["shift"], s1=state["s1"] + c.sum(0), s2=state["s2"] + c.T @ c)


def contract_merge(states, dim_used=None):
    """Chan's pairwise update of (n, mean, M2) over the states in order -> n, mean, covariance (ddof 1) of the leading block"""
    n, mean, m2 = 0, None, None
    for st in states:
        if st["n"] == 0:
            continue
        k = slice(0, dim_used)
        ns, s1 = st["n"], st["s1"][k]
        mean_s = st["shift"][k] + s1 / ns
        m2_s = st["s2"][k, k] - np.outer(s1, s1) / ns
        if n == 0:
            n, mean, m2 = ns, mean_s, m2_s
            continue
        delta = mean_s - mean
        m2 = m2 + m2_s + np.outer(delta, delta) * (n * ns / (n + ns))
        mean = mean + delta * (ns / (n + ns))
        n += ns
    return n, mean, m2 / (n - 1)


def contract_fgd(states_a, states_b, dim_used=None):
    """-> {'fgd', 'mean_gap_sq', 'trace_a', 'trace_b', 'trace_sqrt', 'min_eig_a', 'min_eig_m'}"""
    _, mean_a, c_a = contract_merge(states_a, dim_used)
    _, mean_b, c_b = contract_merge(states_b, dim_used)
    lam, v = np.linalg.eigh(c_a)
    s = (v * np.sqrt(np.maximum(lam, 0.0))) @ v.T
    m = s @ c_b @ s
    mu = np.linalg.eigvalsh(0.5 * (m + m.T))
    gap = mean_a - mean_b
    out = dict(mean_gap_sq=float(gap @ gap), trace_a=float(np.trace(c_a)), trace_b=float(np.trace(c_b)),
               trace_sqrt=float(np.sqrt(np.maximum(mu, 0.0)).sum()), min_eig_a=float(lam.min()), min_eig_m=float(mu.min()))
    out["fgd"] = out["mean_gap_sq"] + out["trace_a"] + out["trace_b"] - 2.0 * out["trace_sqrt"]
    return out


def contract_fgd_of_sets(a, b, dim_used=None):
    return contract_fgd([contract_state(a)], [contract_state(b)], dim_used)


def scale_of(res):
    return res["trace_a"] + res["trace_b"] + res["mean_gap_sq"]


_HOST = {}


def host_fgd(case):
    """compute_fgd of a synthetic case in float64, computed once"""
    if case not in _HOST:
        from speechdrivestemplates_amd.fgd import compute_fgd
        a, b = S.case_pair(case)
        _HOST[case] = compute_fgd(a, b)
    return _HOST[case]


def read_host_errors(path=HOST_ERROR_FILE):
    """{case: recorded abs error of the numpy restatement against compute_fgd}"""
    rec = {}
    for line in open(path):
        f = line.split()
        if len(f) >= 2 and not line.startswith("#"):
            rec[f[0]] = float(f[1])
    return rec


def device_bar(case, scale):
    """100 x the restatement's recorded error, floor 1e-12 x (tr C_A + tr C_B + gap^2): the factor and floor of tests/test_code_pca_gpu.py"""
    return max(100.0 * read_host_errors()[case], 1e-12 * scale)


def fixture():
    return dict(np.load(os.path.join(GOLDEN, "fgd.npz")))


# -- tests ------------------------------------------------------------------------------------------------------------------------------------------
def test_config_key_exists_and_defaults_to_off():
    from speechdrivestemplates_amd.config import get_cfg_defaults
    assert get_cfg_defaults().SYS.DEVICE_FGD is False


def test_restatement_matches_the_reference_fixture():
    g = fixture()
    for tag in FIXTURE_TAGS:
        ref = float(g[tag + "/fgd_ab"][0])
        got = contract_fgd_of_sets(g[tag + "/a"], g[tag + "/b"])["fgd"]
        print("%s restatement %.9f reference %.9f error %.3e bar %.3e" % (tag, got, ref, abs(got - ref), 2e-6 * abs(ref) + 1e-6))
        assert abs(got - ref) <= 2e-6 * abs(ref) + 1e-6, tag
        if tag + "/fgd_aa" in g:
            assert abs(contract_fgd_of_sets(g[tag + "/a"], g[tag + "/a"])["fgd"]) <= 1e-5, tag


def test_restatement_matches_compute_fgd_and_records_its_error():
    lines = ["# numpy restatement of csrc/fgd.hip (tests/test_fgd_device_host.py) against compute_fgd (scipy sqrtm, float64) on the sets of",
             "# tests/golden/synth_fgd_sets.py: case abs_error error_over_scale scale(tr C_A + tr C_B + gap^2) fgd"]
    worst = 0.0
    for case in S.CASES:
        res = contract_fgd_of_sets(*S.case_pair(case))
        err, scale = abs(res["fgd"] - host_fgd(case)), scale_of(res)
        lines.append("%s %.3e %.3e %.9g %.12g" % (case, err, err / scale, scale, res["fgd"]))
        print(lines[-1])
        worst = max(worst, err / scale)
    if os.environ.get("SDT_RECORD_FGD"):
        with open(HOST_ERROR_FILE, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert worst <= HOST_BAR, "restatement vs compute_fgd: worst error / scale %.3e" % worst
    assert set(read_host_errors()) == set(S.CASES), "profiles/r09_fgd_host_error.txt is out of date: re-record it"


def test_chunking_merging_and_sub_block_of_the_restatement():
    a, b = S.case_pair("chunks")
    whole = contract_fgd_of_sets(a, b)
    bar = 1e-12 * scale_of(whole)

    def chunked(x, cuts):
        st, lo = None, 0
        for n in cuts:
            st, lo = contract_state(x[lo:lo + n], st), lo + n
        assert lo == x.shape[0]
        return st
    cuts = (1, 31, 32, 136)
    assert abs(contract_fgd([chunked(a, cuts)], [chunked(b, cuts)])["fgd"] - whole["fgd"]) <= bar
    parts = ((0, 70), (70, 71), (71, 200))  # three "ranks", each with its own shift
    merged = contract_fgd([contract_state(a[lo:hi]) for lo, hi in parts], [contract_state(b[lo:hi]) for lo, hi in parts])
    assert abs(merged["fgd"] - whole["fgd"]) <= bar
    sub = contract_fgd_of_sets(a, b, dim_used=32)
    assert abs(sub["fgd"] - contract_fgd_of_sets(a[:, :32], b[:, :32])["fgd"]) <= bar
    assert abs(sub["fgd"] - host_fgd("chunks_mu")) <= HOST_BAR * scale_of(sub)


def test_shifted_moments_keep_their_digits_under_a_large_offset():
    a, b = S.case_pair("offset")
    assert abs(a.mean() - 1e3) < 1.0 and a.std(0).max() < 0.1
    res = contract_fgd_of_sets(a, b)
    assert abs(res["fgd"] - host_fgd("offset")) <= HOST_BAR * scale_of(res)
    # what the contract forbids: raw second moments minus n mean mean^T lose every digit of this covariance
    x = a.astype(np.float64)
    raw = (x.T @ x - x.shape[0] * np.outer(x.mean(0), x.mean(0))) / (x.shape[0] - 1)
    assert np.abs(raw - np.cov(x, rowvar=False)).max() > 1e3 * HOST_BAR * scale_of(res)


def test_c_abi_checks_sizes_before_launching():
    """sdt_fgd_*: the state size query and the argument checks (they return before touching the GPU)"""
    from speechdrivestemplates_amd import _lib
    lib = _lib.load()
    assert lib.sdt_fgd_state_bytes(64) == (2 + 2 * 64 + 2080) * 8 and lib.sdt_fgd_state_bytes(2) == (2 + 4 + 3) * 8
    assert lib.sdt_fgd_state_bytes(1) == 0 and lib.sdt_fgd_state_bytes(65) == 0 and lib.sdt_fgd_state_bytes(0) == 0
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its checks
    sb = lib.sdt_fgd_state_bytes(64)
    ok = dict(x0=p, d0=32, x1=p, d1=32, rows=32, sb=sb, base=0)

    def acc(**kw):
        a = dict(ok, **kw)
        return lib.sdt_fgd_accumulate(a["x0"], a["d0"], a["x1"], a["d1"], a["rows"], p, a["sb"], a["base"], None)
    for bad in (dict(d0=1, d1=0, x1=None), dict(d0=64, d1=1), dict(d0=65, d1=0, x1=None), dict(sb=sb - 8), dict(rows=0), dict(x1=None),
                dict(d1=0), dict(base=-1), dict(x0=None), dict(d0=0, d1=32)):
        assert acc(**bad) == -1, bad
        assert b"sdt_fgd_accumulate" in lib.sdt_last_error()
    one = (ctypes.c_void_p * 1)(4096)
    many = (ctypes.c_void_p * 65)(*([4096] * 65))
    okf = dict(a=one, b=one, ns=1, dim=64, used=64, sweeps=30, tol=1e-15, out=p, err=p)

    def fin(**kw):
        a = dict(okf, **kw)
        return lib.sdt_fgd_finalize(a["a"], a["b"], a["ns"], a["dim"], a["used"], a["sweeps"], a["tol"], a["out"], a["err"], None)
    for bad in (dict(dim=1, used=1), dict(dim=65, used=64), dict(used=65), dict(used=1), dict(ns=0), dict(a=many, b=many, ns=65), dict(sweeps=0),
                dict(tol=-1.0), dict(out=None), dict(a=(ctypes.c_void_p * 1)(None)), dict(b=(ctypes.c_void_p * 1)(4100))):
        assert fin(**bad) == -1, bad
        assert b"sdt_fgd_finalize" in lib.sdt_last_error()


def test_accumulator_has_no_cpu_fallback():
    from speechdrivestemplates_amd.fgd import FGDAccumulator
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FGDAccumulator(32, "cpu")
    with pytest.raises(ValueError):
        FGDAccumulator(65, "cuda")
