"""Seeded code tables and queries for the template-axes tests (speechdrivestemplates_amd/code_axes.py).

The plain cases are synth_code_tables.make_table at the edge sizes of the kernels: the smallest table (2 x 2), an odd one (17 x 3), one
whose N is no multiple of 16, 32, 128 or 256 and whose D is no power of two (257 x 33), a several-workgroup one (4096 x 32) and the widest
(1000 x 64).  ``dups``: rows 7, 130 and 299 are identical and the nearest to the case's query, so the expected index is 7.
``zeros_col``: one constant column, so one eigenvalue and one whole column of the projections are exactly zero (the sums start at +0.0,
so no projection is ever -0.0: ``signed_zero_projections`` is the table with both signs of zero for the order statistics).
``gapped``: D = 8, independent columns with variances 2^-k under a random rotation, for the eigenvector bound of the host test.
"""
import numpy as np

import synth_code_tables as S

CONST_COL, CONST_VALUE = 2, 0.25
DUP_ROWS = (7, 130, 299)
QUANTILES = (0.0, 0.01, 0.5, 0.99, 1.0)

CASES = {
    "n2_d2": dict(shape=(2, 2), seed=31),
    "n17_d3": dict(shape=(17, 3), seed=32),
    "n257_d33": dict(shape=(257, 33), seed=33),
    "n4096_d32": dict(shape=(4096, 32), seed=34),
    "n1000_d64": dict(shape=(1000, 64), seed=35),
    "dups": dict(shape=(300, 8), seed=36),
    "zeros_col": dict(shape=(500, 5), seed=37),
    "gapped": dict(shape=(2000, 8), seed=38),
}
_TABLES = {}


def case_table(case):
    """-> float32 (N, D); built once per process, do not write to it"""
    if case not in _TABLES:
        spec = CASES[case]
        if case == "gapped":
            rng = np.random.Generator(np.random.PCG64(spec["seed"]))
            n, d = spec["shape"]
            z = rng.standard_normal((n, d)) * np.sqrt(2.0 ** -np.arange(d))
            rot, _ = np.linalg.qr(rng.standard_normal((d, d)))
            t = (z @ rot + rng.standard_normal(d)).astype(np.float32)
        else:
            t = S.make_table(spec["shape"], spec["seed"], CONST_COL if case == "zeros_col" else None).copy()
            if case == "zeros_col":
                t[:, CONST_COL] = np.float32(CONST_VALUE)
            if case == "dups":
                t[list(DUP_ROWS[1:])] = t[DUP_ROWS[0]]
        t.setflags(write=False)
        _TABLES[case] = t
    return _TABLES[case]


def case_queries(case):
    """-> float64 (Q, D).  ``dups``: the one query next to the three identical rows.  Otherwise 11 queries (no multiple of the kernel's
    query tile of 8): nine random points of the table's scale, then row N // 2 of the table itself and the table's mean."""
    t = case_table(case).astype(np.float64)
    rng = np.random.Generator(np.random.PCG64(CASES[case]["seed"] + 100))
    if case == "dups":
        return t[DUP_ROWS[0]][None, :] + 1e-3 * rng.standard_normal((1, t.shape[1]))
    q = t.mean(axis=0) + t.std(axis=0) * rng.standard_normal((9, t.shape[1]))
    return np.concatenate([q, t[t.shape[0] // 2][None, :], t.mean(axis=0)[None, :]])


def signed_zero_projections():
    """(64, 2) float64 with -0.0, +0.0, tiny values of both signs, and infinities: what the order-preserving key has to keep apart"""
    col = np.array([0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0, np.inf, -np.inf] * 8)
    other = np.where(np.arange(64) % 2 == 0, -0.0, 0.0)
    return np.stack([col, other], axis=1)
