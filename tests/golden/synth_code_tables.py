"""Seeded clip-code tables for the code-PCA tests (speechdrivestemplates_amd/code_pca.py).

A table is anisotropic Gaussian noise, column scales linspace(2, 0.2, D), under a mild random mix (I + 0.1 G) and a per-column
offset, stored as float32 like the model's tables.  The spectrum has clear gaps at the top, so the two leading eigenvectors are
well conditioned: every case keeps (l1 - l2) / l1 and (l2 - l3) / l2 at or above MIN_GAP (check_gaps; make_code_pca_reference.py
refuses to record a case that does not).  Cases: the sizes a user meets (300 to 100000 rows of 32), the widest table (D = 64),
per-frame codes (N, F, D), and a table with one constant column (a zero row / column in the covariance).
"""
import numpy as np

MIN_GAP = 0.02
CONST_COL, CONST_VALUE = 7, 0.25

# case -> shape, seed, constant column or None
CASES = {
    "n4096": dict(shape=(4096, 32), seed=11, const_col=None),
    "n300": dict(shape=(300, 32), seed=12, const_col=None),
    "n100000": dict(shape=(100000, 32), seed=13, const_col=None),
    "d64": dict(shape=(512, 64), seed=14, const_col=None),
    "frames": dict(shape=(64, 5, 32), seed=15, const_col=None),
    "constcol": dict(shape=(1000, 32), seed=16, const_col=CONST_COL),
}
SUBSAMPLE = {"n100000": 2000}  # rows of X the fixture keeps for the large case (subsample_rows)


def make_table(shape, seed, const_col=None):
    """-> float32 array of ``shape`` ((N, D) or (N, F, D))"""
    rng = np.random.Generator(np.random.PCG64(seed))
    d = shape[-1]
    n = int(np.prod(shape[:-1]))
    z = rng.standard_normal((n, d)) * np.linspace(2.0, 0.2, d)
    mix = np.eye(d) + 0.1 * rng.standard_normal((d, d))
    x = z @ mix + rng.standard_normal(d)
    if const_col is not None:
        x[:, const_col] = CONST_VALUE
    return x.astype(np.float32).reshape(shape)


def case_table(case):
    return make_table(**CASES[case])


def subsample_rows(case, n_rows):
    """the fixed rows of X kept in the fixture: all of them, or SUBSAMPLE[case] evenly spaced ones"""
    k = SUBSAMPLE.get(case)
    return np.arange(n_rows) if k is None else np.linspace(0, n_rows - 1, k).astype(np.int64)


def check_gaps(eigenvalues):
    """relative gaps (l1 - l2) / l1 and (l2 - l3) / l2 of a descending spectrum"""
    lam = np.asarray(eigenvalues, dtype=np.float64)
    return (lam[0] - lam[1]) / lam[0], (lam[1] - lam[2]) / lam[1]
