"""Seeded code tables for the cluster tests (speechdrivestemplates_amd/code_clusters.py).  Generators only.

``separated_blobs``: Gaussian blobs of unit sigma whose centres are at least 20 sigma apart and whose sizes differ, rows shuffled: the
tables of the host test, on which plain brute-force Lloyd and the contract models must agree on every label.
``case_table``: the bit-for-bit cases of the GPU test.  Blobs 6 sigma apart (so Lloyd needs several iterations and still ends soon) at the
edge sizes of the kernels: the smallest table (2 x 2, k = 1 and 2), every row a seed (5 x 3, k = 5), a small odd one (17 x 3), one row past a
chunk of 1024 (1025 x 5), an odd D (2049 x 33), both caps at once (4096 x 64, k = 64) and more row tiles than the assignment has
workgroups (70001 x 4).  ``dups``: 300 rows that hold only 3 distinct values, k = 5: after three seeds no distance is left.
"""
import numpy as np

# case -> shape, k, blobs the table is drawn from, seed
CASES = {
    "n2_d2_k1": dict(shape=(2, 2), k=1, blobs=1, seed=61),
    "n2_d2_k2": dict(shape=(2, 2), k=2, blobs=2, seed=62),
    "n5_d3_k5": dict(shape=(5, 3), k=5, blobs=2, seed=63),
    "n17_d3_k4": dict(shape=(17, 3), k=4, blobs=4, seed=64),
    "n1025_d5_k3": dict(shape=(1025, 5), k=3, blobs=3, seed=65),
    "n2049_d33_k7": dict(shape=(2049, 33), k=7, blobs=7, seed=66),
    "n4096_d64_k64": dict(shape=(4096, 64), k=64, blobs=64, seed=67),
    "n70001_d4_k8": dict(shape=(70001, 4), k=8, blobs=8, seed=68),
    "dups": dict(shape=(300, 8), k=5, blobs=3, seed=69),
}
DUP_COUNTS = (150, 100, 50)
_TABLES = {}


def blob_sizes(n, blobs):
    """sizes proportional to 1, 2, .. blobs (every blob at least one row while n allows), summing to n"""
    w = np.arange(1, blobs + 1, dtype=np.float64)
    sizes = np.maximum(np.floor(n * w / w.sum()).astype(np.int64), 1 if n >= blobs else 0)
    while sizes.sum() > n:
        sizes[int(np.argmax(sizes))] -= 1
    sizes[-1] += n - sizes.sum()
    return sizes


def blob_centres(blobs, d, sep, rng):
    """``blobs`` points of dimension d, every pair at least ``sep`` apart: multiples of sep along the coordinate axes, then one shift"""
    c = np.zeros((blobs, d))
    for i in range(blobs):
        c[i, i % d] = sep * (1 + i // d)
    return c + rng.standard_normal(d)


def make_blobs(shape, blobs, seed, sep):
    """-> (float32 (N, D) table, the blob of every row)"""
    n, d = shape
    rng = np.random.Generator(np.random.PCG64(seed))
    centres = blob_centres(blobs, d, sep, rng)
    owner = np.repeat(np.arange(blobs), blob_sizes(n, blobs))
    x = centres[owner] + rng.standard_normal((n, d))
    perm = rng.permutation(n)
    return x[perm].astype(np.float32), owner[perm]


def separated_blobs(shape, blobs, seed):
    """blobs whose centres are at least 20 sigma apart (28 between axis neighbours) -> (table, the blob of every row)"""
    return make_blobs(shape, blobs, seed, 20.0)


def case_table(case):
    """-> float32 (N, D); built once per process, do not write to it"""
    if case not in _TABLES:
        spec = CASES[case]
        if case == "dups":
            rng = np.random.Generator(np.random.PCG64(spec["seed"]))
            values = rng.standard_normal((3, spec["shape"][1])).astype(np.float32)
            t = values[rng.permutation(np.repeat(np.arange(3), DUP_COUNTS))]
        else:
            t, _ = make_blobs(spec["shape"], spec["blobs"], spec["seed"], 6.0)
        t.setflags(write=False)
        _TABLES[case] = t
    return _TABLES[case]
