"""Host side of the clip-code figure (speechdrivestemplates_amd/code_pca.py): a float64 numpy restatement of the
kernels' arithmetic (moments, cyclic Jacobi, the sign rule, projection, axis limits, binning, compositing), checked against
scikit-learn's float64 PCA recorded in tests/golden/code_pca_reference.npz and against hand-counted pixels.  No GPU needed.

The restatement's error against the fixture says what the ALGORITHM costs in float64; tests/test_code_pca_gpu.py holds the kernels,
which differ from it by summation order only, to 100 x that error (read from profiles/r08_code_pca_host_error.txt).
Re-record after changing the algorithm or the cases:  SDT_RECORD_CODE_PCA=1 python -m pytest tests/test_code_pca_host.py
"""
import math
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO

sys.path.insert(0, GOLDEN)
import synth_code_tables as S  # noqa: E402

from speechdrivestemplates_amd import code_pca as CP  # noqa: E402

FIXTURE = os.path.join(GOLDEN, "code_pca_reference.npz")
HOST_ERROR_FILE = os.path.join(REPO, "profiles", "r08_code_pca_host_error.txt")
QUANTITIES = ("mean", "components", "explained_variance", "explained_variance_ratio", "X")
# float64 against float64: the eigenvectors of a symmetric matrix move by about eps * ||C|| / gap under rounding, the gaps of the
# cases are >= 0.02 relative, and a sum over D = 64 terms grows the error by at most D: 2.2e-16 / 0.02 * 64 = 7e-13.  One decade of room.
HOST_BAR = 1e-11
_Z, _FITS = [], {}


def fx():
    if not _Z:
        _Z.append(np.load(FIXTURE))
    return _Z[0]


# -- the contract in numpy (shared with tests/test_code_pca_gpu.py) --------------------------------------------------------------
def contract_moments(table):
    x = np.asarray(table, dtype=np.float64)
    n = x.shape[0]
    mean = x.sum(axis=0) / n
    xc = x - mean
    return mean, xc.T @ xc / (n - 1)


def contract_jacobi(cov, max_sweeps=CP.MAX_SWEEPS, rel_tol=CP.REL_TOL):
    """row-cyclic Jacobi as csrc/code_pca.hip runs it -> (diagonal, V^T with eigenvector k in row k, sweeps, final off norm)"""
    A = np.array(cov, dtype=np.float64)
    D = A.shape[0]
    Vt = np.eye(D)
    tol = rel_tol * math.sqrt(float((A * A).sum()))
    sweeps = 0
    while True:
        off = math.sqrt(float(((A - np.diag(np.diag(A))) ** 2).sum()))
        if off <= tol:
            break
        assert sweeps < max_sweeps, "Jacobi did not converge: off %.3e after %d sweeps" % (off, sweeps)
        for p in range(D - 1):
            for q in range(p + 1, D):
                apq = float(A[p, q])
                if apq == 0.0:
                    continue
                app, aqq = float(A[p, p]), float(A[q, q])
                theta = (aqq - app) / (2.0 * apq)
                t = math.copysign(1.0, theta) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                rp, rq = A[p].copy(), A[q].copy()
                A[p] = A[:, p] = c * rp - s * rq
                A[q] = A[:, q] = s * rp + c * rq
                A[p, p], A[q, q] = app - t * apq, aqq + t * apq
                A[p, q] = A[q, p] = 0.0
                vp, vq = Vt[p].copy(), Vt[q].copy()
                Vt[p], Vt[q] = c * vp - s * vq, s * vp + c * vq
        sweeps += 1
    return np.diag(A).copy(), Vt, sweeps, off


def contract_components(lam, Vt, k=2):
    """eigenvalues descending (ties: the lower index first); component = eigenvector signed so that its entry of largest magnitude
    (first of equals) is positive"""
    order = sorted(range(len(lam)), key=lambda i: (-lam[i], i))
    comps = []
    for i in order[:k]:
        v = Vt[i]
        comps.append(-v if v[int(np.argmax(np.abs(v)))] < 0 else v.copy())
    return np.asarray([lam[i] for i in order]), np.asarray(comps)


def axis_limits(mn, mx):
    pad = 0.05 * (mx - mn)
    lo, hi = mn - pad, mx + pad
    return (lo, hi) if hi > lo else (mn - 0.5, mx + 0.5)


def contract_fit(table):
    t = np.asarray(table)
    x = t.reshape(-1, t.shape[-1])
    mean, cov = contract_moments(x)
    lam, Vt, sweeps, off = contract_jacobi(cov)
    lam_sorted, comps = contract_components(lam, Vt)
    X = (x.astype(np.float64) - mean) @ comps.T
    limits = axis_limits(X[:, 0].min(), X[:, 0].max()) + axis_limits(X[:, 1].min(), X[:, 1].max())
    return {"mean": mean, "components": comps, "explained_variance": lam_sorted[:2], "explained_variance_ratio": lam_sorted[:2] / np.trace(cov),
            "X": X, "limits": limits, "sweeps": sweeps, "offdiag": off, "cov": cov}


def contract_counts(X, limits, ph, pw, marker_px=2):
    """the count pass: every operation rounded on its own (numpy never fuses a multiply with an add) -> (ph, pw) int64"""
    X = np.asarray(X, dtype=np.float64)
    lo0, hi0, lo1, hi1 = (np.float64(v) for v in limits)
    keep = (X[:, 0] >= lo0) & (X[:, 0] <= hi0) & (X[:, 1] >= lo1) & (X[:, 1] <= hi1)
    sx, sy = np.float64(pw) / (hi0 - lo0), np.float64(ph) / (hi1 - lo1)
    col = np.minimum(np.floor((X[keep, 0] - lo0) * sx).astype(np.int64), pw - 1)
    row = ph - 1 - np.minimum(np.floor((X[keep, 1] - lo1) * sy).astype(np.int64), ph - 1)
    counts = np.zeros((ph, pw), np.int64)
    first = (marker_px - 1) // 2
    for dy in range(marker_px):
        for dx in range(marker_px):
            cc, rr = col - first + dx, row - first + dy
            ok = (cc >= 0) & (cc < pw) & (rr >= 0) & (rr < ph)
            np.add.at(counts, (rr[ok], cc[ok]), 1)
    return counts


def contract_image(counts, table, canvas, margin=CP.MARGIN_PX):
    h, w = canvas
    ph, pw = counts.shape
    assert (ph, pw) == (h - 2 * margin, w - 2 * margin)
    img = np.full((h, w, 3), 255, np.uint8)
    img[margin - 1:margin + ph + 1, margin - 1:margin + pw + 1] = 0
    img[margin:margin + ph, margin:margin + pw] = table[np.minimum(counts, len(table) - 1)]
    return img


def case_fit(case):
    if case not in _FITS:
        _FITS[case] = contract_fit(S.case_table(case))
    return _FITS[case]


def errors_against_fixture(case, got):
    """{quantity: (max abs difference to the scikit-learn fixture, max abs value of the fixture's quantity)}; ``got['X']`` has every row"""
    z = fx()
    out = {}
    for q in QUANTITIES:
        ref = z[case + "/" + q]
        g = np.asarray(got[q], dtype=np.float64)
        if q == "X":
            g = g[S.subsample_rows(case, g.shape[0])]
            scale = float(z[case + "/max_abs_X"])
        else:
            scale = float(np.abs(ref).max())
        out[q] = (float(np.abs(g - ref).max()), scale)
    return out


def read_host_errors(path=HOST_ERROR_FILE):
    """{(case, quantity): recorded max abs error of the numpy restatement}"""
    rec = {}
    for line in open(path):
        f = line.split()
        if len(f) >= 3 and not line.startswith("#"):
            rec[(f[0], f[1])] = float(f[2])
    return rec


# -- tests -------------------------------------------------------------------------------------------------------------------------
def test_restatement_matches_scikit_learn_and_records_its_error():
    lines = ["# numpy restatement of csrc/code_pca.hip (tests/test_code_pca_host.py) against scikit-learn's float64 PCA",
             "# (tests/golden/code_pca_reference.npz): case quantity max_abs_error error_over_scale scale sweeps", ]
    worst = 0.0
    for case in S.CASES:
        fit = case_fit(case)
        for q, (err, scale) in errors_against_fixture(case, fit).items():
            lines.append("%s %s %.3e %.3e %.6g %d" % (case, q, err, err / scale, scale, fit["sweeps"]))
            print(lines[-1])
            worst = max(worst, err / scale)
    if os.environ.get("SDT_RECORD_CODE_PCA"):
        with open(HOST_ERROR_FILE, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert worst <= HOST_BAR, "restatement vs scikit-learn: worst error / scale %.3e" % worst
    rec = read_host_errors()
    assert set(rec) == {(c, q) for c in S.CASES for q in QUANTITIES}, "profiles/r08_code_pca_host_error.txt is out of date: re-record it"


def test_fixture_cases_have_clear_gaps_and_the_stated_shapes():
    z = fx()
    for case, spec in S.CASES.items():
        assert min(S.check_gaps(z[case + "/lambda3"])) >= S.MIN_GAP, case
        n = int(np.prod(spec["shape"][:-1]))
        assert z[case + "/X"].shape == (S.SUBSAMPLE.get(case, n), 2)
        assert z[case + "/components"].shape == (2, spec["shape"][-1])
    assert os.path.getsize(FIXTURE) < (1 << 20)
    t = S.case_table("constcol")
    assert (t[:, S.CONST_COL] == np.float32(S.CONST_VALUE)).all()


def test_jacobi_converges_quadratically_and_diagonalises():
    fit = case_fit("d64")
    assert fit["sweeps"] <= 12 and fit["offdiag"] <= 1e-15 * np.linalg.norm(fit["cov"])
    lam, Vt, _, _ = contract_jacobi(fit["cov"])
    np.testing.assert_allclose(Vt @ Vt.T, np.eye(64), atol=1e-13)
    np.testing.assert_allclose(Vt.T @ np.diag(lam) @ Vt, fit["cov"], atol=1e-13 * np.abs(fit["cov"]).max() * 64)
    np.testing.assert_allclose(np.sort(lam), np.linalg.eigvalsh(fit["cov"]), atol=1e-13 * lam.max())
    # a constant column: a zero row and column of the covariance, an exactly zero eigenvalue, a zero entry in every component
    fit = case_fit("constcol")
    assert (fit["cov"][S.CONST_COL] == 0).all() and (fit["components"][:, S.CONST_COL] == 0).all()
    # already diagonal: no sweep at all
    assert contract_jacobi(np.diag([3.0, 1.0, 2.0]))[2] == 0


def test_sign_rule_and_ordering():
    Vt = np.array([[0.6, -0.8, 0.0], [-0.5, 0.5, -0.70710678], [0.8, 0.6, 0.0]])
    lam = np.array([2.0, 5.0, 2.0])
    order, comps = contract_components(lam, Vt, k=3)
    assert order.tolist() == [5.0, 2.0, 2.0]
    assert comps[0].tolist() == [0.5, -0.5, 0.70710678]  # largest magnitude is the negative last entry: flipped
    assert comps[1].tolist() == [-0.6, 0.8, 0.0]  # the tie at 2.0 goes to index 0; |-0.8| is largest: flipped
    assert comps[2].tolist() == [0.8, 0.6, 0.0]
    assert contract_components(np.array([1.0, 1.0]), np.array([[-0.5, 0.5], [0.5, -0.5]]))[1].tolist() == [[0.5, -0.5], [0.5, -0.5]]  # first of equals
    # the fixture follows the same rule (scikit-learn >= 1.5): nothing is compared up to sign anywhere
    z = fx()
    for case in S.CASES:
        c = z[case + "/components"]
        assert (c[np.arange(2), np.abs(c).argmax(axis=1)] > 0).all()


def test_axis_limits():
    assert axis_limits(-2.0, 8.0) == (-2.5, 8.5)
    assert axis_limits(3.0, 3.0) == (2.5, 3.5)
    assert axis_limits(0.0, 0.0) == (-0.5, 0.5)


def test_colour_table_is_monotone_and_reaches_its_fixed_point():
    t = CP.colour_table()
    assert t.dtype == np.uint8 and t.shape[1] == 3
    assert t[0].tolist() == [255, 255, 255] and t[-1].tolist() == [31, 119, 180]
    assert t[1].tolist() == [210, 228, 240]  # 255 - 0.2 * (255 - c) = 210.2, 227.8, 240.0
    d = np.diff(t.astype(np.int64), axis=0)
    assert (d <= 0).all() and d[-1].sum() < 0  # never brighter again (plateaus occur before the end); the last entry is the first to reach the colour
    q = 0.8 ** (len(t) - 1)  # the fixed point: one more marker, or a million, change nothing
    for k in (len(t), len(t) + 1, 10 ** 6):
        assert [int(math.floor(255.0 * 0.8 ** k + c * (1.0 - 0.8 ** k) + 0.5)) for c in (31, 119, 180)] == t[-1].tolist()
    assert (255 - 31) * q < 0.5 <= (255 - 31) * q / 0.8
    assert CP.colour_table(alpha=1.0).tolist() == [[255, 255, 255], [31, 119, 180]]
    with pytest.raises(ValueError):
        CP.colour_table(alpha=0.0)
    with pytest.raises(ValueError):
        CP.colour_table(colour=(31, 119, 256))


def test_histogram_of_six_hand_placed_points():
    # axis 0 spans [0, 10] -> limits [-0.5, 10.5], 11 columns of width 1; axis 1 spans [0, 4] -> [-0.2, 4.2], 11 rows of height 0.4
    X = np.array([[0.0, 0.0],    # at both minima: column 0, bottom row (10); the 2 x 2 marker reaches row 11, clipped
                  [10.0, 4.0],   # at both maxima: column 10, top row (0); the marker reaches column 11, clipped
                  [10.0, 4.0],   # the same point again: counted twice
                  [5.0, 2.0],    # the centre: column 5; (2.0 + 0.2) * 2.5 = 5.5 -> bin 5 -> row 5
                  [4.5, 1.8],    # (4.5 + 0.5) * 1 = 5 exactly -> column 5; (1.8 + 0.2) * 2.5 = 5 -> row 5 (whatever rounding gives is recomputed below)
                  [9.6, 0.0]])   # column 10 at the bottom row: clipped on two sides, one pixel left
    limits = axis_limits(0.0, 10.0) + axis_limits(0.0, 4.0)
    assert limits[:2] == (-0.5, 10.5) and abs(limits[2] + 0.2) < 1e-15 and abs(limits[3] - 4.2) < 1e-15
    counts = contract_counts(X, limits, 11, 11, marker_px=2)
    row4 = 10 - int(math.floor((1.8 - limits[2]) * (11.0 / (limits[3] - limits[2]))))
    expect = np.zeros((11, 11), np.int64)
    expect[10, 0] += 1
    expect[10, 1] += 1
    expect[0, 10] += 2
    expect[1, 10] += 2
    for r, c in ((5, 5), (row4, 5)):
        expect[r:r + 2, c:c + 2] += 1
    expect[10, 10] += 1
    assert row4 in (4, 5, 6) and np.array_equal(counts, expect)
    assert counts.sum() == 2 + 2 + 2 + 4 + 4 + 1
    single = np.zeros((11, 11), np.int64)  # marker_px = 1: the bin itself
    for r, c in ((10, 0), (0, 10), (0, 10), (5, 5), (row4, 5), (10, 10)):
        single[r, c] += 1
    assert np.array_equal(contract_counts(X, limits, 11, 11, marker_px=1), single)
    # points outside the limits, or not finite, are not drawn
    out = contract_counts(np.array([[11.0, 2.0], [np.nan, 1.0], [5.0, -1.0]]), limits, 11, 11)
    assert out.sum() == 0
    # the picture: white margin, black ring, table colours inside
    table = CP.colour_table()
    img = contract_image(counts, table, (11 + 2 * CP.MARGIN_PX, 11 + 2 * CP.MARGIN_PX))
    m = CP.MARGIN_PX
    assert img[0, 0].tolist() == [255, 255, 255] and img[m - 1, m - 1].tolist() == [0, 0, 0] and img[m + 11, m + 3].tolist() == [0, 0, 0]
    assert img[m, m + 10].tolist() == table[2].tolist() and img[m + 10, m].tolist() == table[1].tolist() and img[m + 3, m + 3].tolist() == [255, 255, 255]


def test_public_functions_refuse_cpu_tensors_and_bad_shapes():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CP.fit_project(torch.zeros(8, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CP.render_scatter(torch.zeros(8, 2, dtype=torch.float64), (0, 1, 0, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CP.clip_code_figure(np.zeros((8, 32), np.float32))
    with pytest.raises(ValueError):
        CP.plot_rectangle((24, 640))
    assert CP.plot_rectangle((480, 640)) == (456, 616)


def test_config_key_defaults_to_off():
    from speechdrivestemplates_amd.config import get_cfg_defaults
    assert get_cfg_defaults().SYS.EPOCH_FIGURES is False


def test_save_png_round_trip(tmp_path):
    from PIL import Image
    img = np.random.default_rng(0).integers(0, 256, (20, 30, 3), dtype=np.uint8)
    meta = {"explained_variance_ratio": (0.25, 0.125), "limits": (-1.0, 1.0, -2.0, 2.0)}
    path = CP.save_png(str(tmp_path / "figures" / "a.png"), img, meta)
    with Image.open(path) as im:
        assert np.array_equal(np.asarray(im.convert("RGB")), img)
        assert eval(im.text["explained_variance_ratio"]) == (0.25, 0.125) and eval(im.text["limits"]) == (-1.0, 1.0, -2.0, 2.0)
    assert CP.describe(meta) == "evr=(0.250000, 0.125000) limits=(-1, 1, -2, 2)"
