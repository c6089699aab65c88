"""Host side of the template axes (speechdrivestemplates_amd/code_axes.py): the numpy contract models against LAPACK,
numpy's own quantile and a brute-force search, and the file the two demo modes read.  No GPU needed.

Bounds.  A symmetric eigenproblem solved in float64 has eigenvalue errors of a modest multiple of eps ||C||_F (backward stability of
Jacobi and of LAPACK alike) and eigenvector errors of that over the gap to the nearest other eigenvalue (Davis-Kahan); the multiple, 64,
is the widest table's dimension -- one rounding per accumulated term.  Both bounds are computed from the fixture, not from the results.
"""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from test_code_pca_host import HOST_BAR, contract_components, contract_jacobi, contract_moments

sys.path.insert(0, GOLDEN)
import synth_axes_tables as A  # noqa: E402

from speechdrivestemplates_amd import code_axes as CA  # noqa: E402

EPS = np.finfo(np.float64).eps
_FITS = {}


def model_fit(case):
    """the model's own fit of a case, computed once: mean, cov, eigenvalues, components, projections"""
    if case not in _FITS:
        t = A.case_table(case)
        mean, cov = contract_moments(t)
        lam, comps, sweeps, off = CA.model_components(cov)
        _FITS[case] = dict(mean=mean, cov=cov, lam=lam, comps=comps, sweeps=sweeps, off=off, P=CA.model_project(t, mean, comps))
    return _FITS[case]


def signed(v):
    return -v if v[int(np.argmax(np.abs(v)))] < 0 else v


@pytest.mark.parametrize("case", list(A.CASES))
def test_model_components_against_lapack(case):
    f = model_fit(case)
    cov, lam, comps = f["cov"], f["lam"], f["comps"]
    D = cov.shape[0]
    frob = np.linalg.norm(cov)
    w, V = np.linalg.eigh(cov)
    w, V = w[::-1], V[:, ::-1]
    err = np.abs(lam - w).max()
    print("code_axes %s: eigenvalues vs LAPACK %.3e, bound %.3e (%d sweeps, off %.2e)" % (case, err, 64 * EPS * frob, f["sweeps"], f["off"]))
    assert err <= 64 * EPS * frob
    assert comps.shape == (D, D) and (np.diff(lam) <= 0).all()
    assert (comps[np.arange(D), np.abs(comps).argmax(axis=1)] > 0).all()  # the sign rule
    np.testing.assert_allclose(comps @ comps.T, np.eye(D), atol=64 * EPS)
    # the shared device code keeps two of these: the model agrees with the two-component model of the code_pca tests
    lam2, Vt2, _, _ = contract_jacobi(cov)
    order2, comps2 = contract_components(lam2, Vt2, k=min(2, D))
    np.testing.assert_allclose(lam, order2, rtol=0, atol=64 * EPS * frob)
    np.testing.assert_allclose(comps[:2], comps2, rtol=0, atol=HOST_BAR)
    if case == "gapped":
        gaps = np.abs(w[:, None] - w[None, :]) + np.diag(np.full(D, np.inf))
        min_gap = gaps.min()
        bound = 64 * EPS * frob / min_gap
        worst = max(np.abs(comps[k] - signed(V[:, k])).max() for k in range(D))
        print("code_axes gapped: components vs LAPACK %.3e, bound %.3e (min gap %.3e)" % (worst, bound, min_gap))
        assert (w[:-1] / w[1:]).min() >= 1.5  # the fixture's promise
        assert worst <= bound


@pytest.mark.parametrize("case", ["n4096_d32", "n1000_d64", "gapped"])
def test_model_components_against_scikit_learn(case):
    decomposition = pytest.importorskip("sklearn.decomposition")
    f = model_fit(case)
    pca = decomposition.PCA(n_components=2, svd_solver="full").fit(A.case_table(case).astype(np.float64))
    ref = np.stack([signed(c) for c in pca.components_])
    err = np.abs(f["comps"][:2] - ref).max()
    print("code_axes %s: components[:2] vs scikit-learn %.3e, bar %.1e" % (case, err, HOST_BAR))
    assert err <= HOST_BAR * max(1.0, np.abs(ref).max())
    assert np.abs(f["lam"][:2] - pca.explained_variance_).max() <= HOST_BAR * pca.explained_variance_.max()


def test_model_project_is_the_centred_product():
    for case in A.CASES:
        f = model_fit(case)
        t = A.case_table(case).astype(np.float64)
        ref = (t - f["mean"]) @ f["comps"].T
        scale = np.abs(t - f["mean"]).max() * t.shape[1]
        assert np.abs(f["P"] - ref).max() <= 4 * EPS * scale, case
    f = model_fit("zeros_col")
    assert f["lam"][-1] == 0.0 and (f["P"][:, -1] == 0.0).all() and (f["comps"][:, A.CONST_COL] == 0.0)[:-1].all()


@pytest.mark.parametrize("case", list(A.CASES))
def test_model_quantiles_equal_numpy_lower(case):
    P = model_fit(case)["P"]
    n = P.shape[0]
    ranks = CA.quantile_ranks(A.QUANTILES, n)
    got = CA.model_quantiles(P, ranks)
    assert got.shape == (P.shape[1], 5) and ranks[0] == 0 and ranks[-1] == n - 1
    for k in range(P.shape[1]):
        for j, q in enumerate(A.QUANTILES):
            assert got[k, j] == np.quantile(P[:, k], q, method="lower"), (case, k, q)
    with pytest.raises(ValueError):
        CA.quantile_ranks([1.5], n)


def test_model_quantiles_on_signed_zeros_and_infinities():
    P = A.signed_zero_projections()
    got = CA.model_quantiles(P, list(range(64)))
    assert np.array_equal(got[0], np.sort(P[:, 0])) and (got[1] == 0.0).all()
    assert got[0, 0] == -np.inf and got[0, 63] == np.inf and got[0, 16] == -5e-324 and got[0, 47] == 5e-324


@pytest.mark.parametrize("case", list(A.CASES))
def test_model_nearest_equals_brute_force(case):
    t, q = A.case_table(case), A.case_queries(case)
    index, dist2 = CA.model_nearest(t, q)
    d2 = ((q[:, None, :] - t.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    ref = np.argmin(d2, axis=1)
    assert index.dtype == np.int64 and np.array_equal(index, ref)
    np.testing.assert_allclose(dist2, d2[np.arange(len(q)), ref], rtol=64 * EPS, atol=0)
    if case == "dups":
        assert index.tolist() == [A.DUP_ROWS[0]]
        assert len({d2[0, r] for r in A.DUP_ROWS}) == 1 and (np.delete(d2[0], list(A.DUP_ROWS)) > d2[0, 7]).all()
    else:  # the query that is a table row finds it (or a lower identical one) at distance zero
        assert dist2[9] == 0.0 and index[9] <= t.shape[0] // 2 and np.array_equal(t[index[9]], t[t.shape[0] // 2])


def test_public_functions_refuse_cpu_tensors_and_bad_sizes():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CA.fit_axes(torch.zeros(8, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CA.axis_quantiles(torch.zeros(8, 2, dtype=torch.float64), [0.5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CA.nearest_codes(torch.zeros(8, 32), torch.zeros(1, 32, dtype=torch.float64))


def _fake_fit(case):
    """a fit dict as ``fit_axes`` returns it, from the model, on the host (``traversal`` needs the device only for its quantiles)"""
    import torch
    f = model_fit(case)
    n, d = f["P"].shape
    return {"mean": torch.from_numpy(f["mean"]), "components": torch.from_numpy(f["comps"]), "explained_variance": torch.from_numpy(f["lam"]),
            "explained_variance_ratio": torch.from_numpy(f["lam"] / np.trace(f["cov"])), "projections": torch.from_numpy(f["P"]),
            "n_rows": n, "dim": d}


def test_traversal_and_write_axes_round_trip(tmp_path, monkeypatch):
    import torch
    case = "n257_d33"
    fit = _fake_fit(case)
    t_table = A.case_table(case)
    n, d = t_table.shape
    monkeypatch.setattr(CA, "axis_quantiles",  # the host stand-in of the device's order statistics, same contract
                        lambda P, q: torch.from_numpy(CA.model_quantiles(P.numpy(), CA.quantile_ranks(q, P.shape[0]))))
    trav = CA.traversal(fit, [0, 3, 32], 7, lo_q=0.01, hi_q=0.99)
    t, pts = trav["t"].numpy(), trav["points"].numpy()
    assert trav["axes"].tolist() == [0, 3, 32] and t.shape == (3, 7) and pts.shape == (3, 7, d) and pts.dtype == np.float64
    mean, comps, P = fit["mean"].numpy(), fit["components"].numpy(), fit["projections"].numpy()
    for i, k in enumerate([0, 3, 32]):
        assert t[i, 0] == np.quantile(P[:, k], 0.01, method="lower") and t[i, -1] == np.quantile(P[:, k], 0.99, method="lower")
        assert np.array_equal(t[i], np.linspace(t[i, 0], t[i, -1], 7))
        assert np.array_equal(pts[i], mean[None, :] + t[i][:, None] * comps[k][None, :])  # on the line mean + t components[k]
        back = (pts[i] - mean) @ comps[k]  # and its coordinate on that axis is t again
        np.testing.assert_allclose(back, t[i], atol=64 * EPS * np.abs(pts[i]).max() * d)
    assert CA.traversal(fit, 2, 3)["axes"].tolist() == [0, 1]
    for bad in (dict(axes=[d], steps=3), dict(axes=0, steps=3), dict(axes=2, steps=0), dict(axes=2, steps=3, lo_q=0.9, hi_q=0.1)):
        with pytest.raises(ValueError):
            CA.traversal(fit, **bad)
    index, dist2 = CA.model_nearest(t_table, pts)
    quantiles = CA.model_quantiles(P, CA.quantile_ranks(CA.FILE_QUANTILES, n))
    path = CA.write_axes(str(tmp_path / "sub" / "axes.npz"), fit, quantiles, trav, index.reshape(3, 7), dist2.reshape(3, 7))
    z = np.load(path)
    want = {"v": ((d, d), np.float32), "mean": ((d,), np.float64), "explained_variance": ((d,), np.float64),
            "explained_variance_ratio": ((d,), np.float64), "quantiles": ((d, 5), np.float64), "axes": ((3,), np.int64),
            "t": ((3, 7), np.float64), "points": ((3, 7, d), np.float64), "code_index": ((3, 7), np.int64), "code_dist2": ((3, 7), np.float64)}
    assert sorted(z.files) == sorted(want)
    for k, (shape, dtype) in want.items():
        assert z[k].shape == shape and z[k].dtype == dtype, k
    assert np.array_equal(z["v"], comps.astype(np.float32)) and np.array_equal(z["points"], pts)
    assert (z["code_index"] >= 0).all() and (z["code_index"] < n).all()
    assert np.array_equal(z["v"][2] * 10, (comps[2].astype(np.float32)) * 10)  # what DEMO.CODE_PATH's reader computes
    assert os.path.getsize(path) < (1 << 20)


def test_c_abi_refuses_unsupported_sizes_before_any_launch():
    """outside 2 <= N, 2 <= D <= 64, 1 <= Q <= 65536, 1 <= R <= 16 the workspace queries return 0 and the entry points SDT_ERR_UNSUPPORTED"""
    import ctypes as C

    from speechdrivestemplates_amd import _lib
    lib = _lib.load()
    assert lib.sdt_code_axes_quantiles_workspace_bytes(1000, 32, 5) == 32 * 5 * (16 + 1024)
    assert lib.sdt_code_axes_nearest_workspace_bytes(1000, 32, 28) > 0
    for n, d, r in ((1, 32, 5), (1000, 1, 5), (1000, 65, 5), (1000, 32, 0), (1000, 32, 17), ((1 << 30) + 1, 32, 5)):
        assert lib.sdt_code_axes_quantiles_workspace_bytes(n, d, r) == 0, (n, d, r)
    for n, d, q in ((1, 32, 5), (1000, 1, 5), (1000, 65, 5), (1000, 32, 0), (1000, 32, 65537)):
        assert lib.sdt_code_axes_nearest_workspace_bytes(n, d, q) == 0, (n, d, q)
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    assert lib.sdt_code_axes_eigh(p, 65, 30, 1e-15, p, p, p, p, None) == -3
    assert lib.sdt_code_axes_project(p, 1000, 1, p, p, p, None) == -3
    assert lib.sdt_code_axes_project(p, 1, 32, p, p, p, None) == -3
    assert lib.sdt_code_axes_quantiles(p, 1000, 32, p, 17, p, p, 1 << 20, None) == -3
    assert lib.sdt_code_axes_nearest(p, 1000, 32, p, 65537, p, p, p, p, 1 << 20, None) == -3
    assert lib.sdt_code_axes_nearest(p, 1000, 32, p, 8, p, p, p, p, 8, None) == -1  # workspace too small: an argument error
    assert b"sdt_code_axes_nearest" in lib.sdt_last_error()
    with pytest.raises(ValueError, match="dim"):
        CA._check(lib.sdt_code_axes_eigh(p, 1, 30, 1e-15, p, p, p, p, None))
