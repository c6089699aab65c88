"""Seeded feature sets for the device-FGD tests (speechdrivestemplates_amd/fgd.py, csrc/fgd.hip).

A set is anisotropic Gaussian noise, column scales linspace(1.5, 0.5, D), under a mild random mix (I + 0.1 G) plus a per-column mean,
times ``scale`` plus ``offset``, stored as float32 like the pose encoder's outputs.  The two sets of a pair come from one generator, so
they differ in mix and mean.  With n > D rows both covariances have full rank: scipy's sqrtm and the symmetric eigen route then agree to
round-off (on rank-deficient sets sqrtm itself is only good to about 1e-7, which is why those are held to the fixture bar instead).
"""
import numpy as np

# case -> rows, dim, seed, offset, scale.  full_d*: n = 4 d at the widths around the 32-row tile and the 64-lane wave; offset: a large common
# offset over a small spread (a raw-moment covariance loses every digit here); chunks: the set the chunking / merging / sub-block tests cut up;
# the n* cases are the sizes a validation epoch delivers.
CASES = {
    "full_d2": dict(n=8, d=2, seed=21),
    "full_d31": dict(n=124, d=31, seed=22),
    "full_d32": dict(n=128, d=32, seed=23),
    "full_d33": dict(n=132, d=33, seed=24),
    "full_d64": dict(n=256, d=64, seed=25),
    "offset": dict(n=256, d=64, seed=26, offset=1e3, scale=1e-2),
    "chunks": dict(n=200, d=64, seed=27),
    "chunks_mu": dict(n=200, d=64, seed=27, keep=32),  # the leading 32 columns of "chunks"
    "n256_d32": dict(n=256, d=32, seed=28),
    "n4096_d64": dict(n=4096, d=64, seed=29),
}
FULL_RANK = ("full_d2", "full_d31", "full_d32", "full_d33", "full_d64")


def make_pair(n, d, seed, offset=0.0, scale=1.0, keep=None):
    """-> two float32 (n, keep or d) arrays"""
    rng = np.random.Generator(np.random.PCG64(seed))

    def one():
        z = rng.standard_normal((n, d)) * np.linspace(1.5, 0.5, d)
        mix = np.eye(d) + 0.1 * rng.standard_normal((d, d))
        x = (z @ mix + 0.3 * rng.standard_normal(d)) * scale + offset
        return np.ascontiguousarray(x.astype(np.float32)[:, :keep])
    return one(), one()


def case_pair(case):
    return make_pair(**CASES[case])
