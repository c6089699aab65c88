"""Host side of the code clusters (speechdrivestemplates_amd/code_clusters.py): the numpy contract models against
plain brute force written here, on separated blobs; the seeding rules against np.cumsum and np.argmax; the numbering by count; the
float32 codes of the file; the argument checks and the sizes the C ABI refuses.  No GPU needed.  tests/test_code_clusters_gpu.py holds the
kernels to these models bit for bit.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import synth_cluster_tables as K  # noqa: E402

from speechdrivestemplates_amd import code_clusters as CC  # noqa: E402

U = 2.0 ** -53
BLOBS = {"n257_d3_k4": dict(shape=(257, 3), blobs=4, seed=71), "n4096_d32_k8": dict(shape=(4096, 32), blobs=8, seed=72)}
_BLOBS = {}


def blobs(case):
    if case not in _BLOBS:
        spec = BLOBS[case]
        _BLOBS[case] = K.separated_blobs(spec["shape"], spec["blobs"], spec["seed"])
    return _BLOBS[case]


def brute_lloyd(x, seeds, max_iter=100):
    """textbook Lloyd from the given seed rows, in numpy's own summation order -> (labels, centres, iterations)"""
    centres = x[seeds].copy()
    labels = None
    for it in range(1, max_iter + 1):
        new = np.argmin(((x[:, None, :] - centres[None, :, :]) ** 2).sum(axis=2), axis=1)
        same = labels is not None and np.array_equal(new, labels)
        labels = new
        for c in range(len(centres)):
            if (labels == c).any():
                centres[c] = x[labels == c].mean(axis=0)
        if same:
            break
    return labels, centres, it


def test_the_blobs_are_separated():
    for case, spec in BLOBS.items():
        t, owner = blobs(case)
        assert t.shape == spec["shape"] and t.dtype == np.float32
        mu = np.stack([t[owner == b].astype(np.float64).mean(axis=0) for b in range(spec["blobs"])])
        gaps = np.sqrt(((mu[:, None] - mu[None]) ** 2).sum(axis=2))[np.triu_indices(spec["blobs"], 1)]
        assert gaps.min() >= 20.0 - 1.0, gaps.min()  # (sample means of unit-sigma blobs around centres 20 apart and more)


@pytest.mark.parametrize("init", CC.INITS)
@pytest.mark.parametrize("case", list(BLOBS))
def test_model_fit_against_brute_force_lloyd(case, init):
    t, owner = blobs(case)
    x = t.astype(np.float64)
    k = BLOBS[case]["blobs"]
    history = []
    fit = CC.model_fit(t, k, seed=3, init=init, history=history)
    its = [h for h in history if h["stage"] == "iteration"]
    labels, centres, iterations = brute_lloyd(x, fit["seeds"])
    assert fit["converged"] and fit["iterations"] == iterations == len(its)
    assert np.array_equal(its[-1]["labels"], labels)  # (the loop's numbering: cluster c grew from seed c)
    # the centres: two summation orders of the same members, each within the worst-case rounding of an n-term float64 sum
    for c in range(k):
        members = x[labels == c]
        bound = 2 * (len(members) + 8) * U * np.abs(members).sum(axis=0) / max(len(members), 1)
        err = np.abs(its[-1]["centers"][c] - centres[c])
        print("code_clusters %s %s cluster %d: centre error / bound %.3e" % (case, init, c, (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
    # converged at iteration >= 2: the last update changed no bit, and the final pass repeats the loop's labels
    assert fit["iterations"] >= 2 and np.array_equal(its[-1]["centers"], its[-2]["centers"])
    assert np.array_equal(fit["order"][fit["labels"]], its[-1]["labels"])
    assert np.array_equal(fit["centers"], its[-1]["centers"][fit["order"]])
    if init == "farthest":  # one seed per blob, so the clusters are the blobs
        assert len(set(owner[fit["seeds"]].tolist())) == k
        assert all(len(set(owner[fit["labels"] == c].tolist())) == 1 for c in range(k)) and fit["empty_clusters"] == 0


@pytest.mark.parametrize("case", list(BLOBS) + ["n70001_d4_k8"])
def test_kmeanspp_picks_fall_where_the_cumulative_sum_says(case):
    t = blobs(case)[0] if case in BLOBS else K.case_table(case)
    n, k = t.shape[0], 8
    for seed in range(4):
        history = []
        seeds, m, rules = CC.model_seeds(t, k, seed=seed, init="kmeans++", history=history)
        u = CC.draw_uniforms(seed, k)
        assert seeds[0] == min(int(u[0] * n), n - 1) and len(set(seeds.tolist())) == k
        assert np.array_equal(m, history[-1]["m"]) and (m[seeds] == 0.0).all()
        for j in range(1, k):
            before = history[j - 1]["m"]
            cum = np.cumsum(before)
            T, s = cum[-1], int(seeds[j])
            tol = n * 2.0 ** -52 * T
            assert before[s] > 0.0 and rules[j] in CC.RULES
            assert (cum[s - 1] if s else 0.0) - tol <= u[j] * T <= cum[s] + tol, (case, seed, j)


def test_kmeanspp_fallback_rules():
    # r == T: no chunk passes, the table's last row with a distance (u == 1 only: for u < 1 the product rounds below T)
    m = np.zeros(3000)
    m[[5, 1030, 2500]] = (1.0, 2.0, 3.0)
    assert CC.model_seed_pick(m, "kmeans++", 1.0, [0]) == (2500, "table-last")
    assert CC.model_seed_pick(m, "kmeans++", 1.0 - 2.0 ** -53, [0]) == (2500, "walk")
    assert CC.model_seed_pick(m, "kmeans++", 0.0, [0]) == (5, "walk")
    assert CC.model_seed_pick(m, "kmeans++", 0.5, [0]) == (2500, "walk")  # P = 1, 3, 6; r = 3: chunk 2
    # the chunk's own sum passes r but the walk from P[c - 1] does not: the chunk's last row with a distance
    m = np.zeros(2048)
    m[0] = 2.0 ** 53
    m[1024:1027] = 1.0  # chunk sum 3: P[1] = 2^53 + 3 rounds to 2^53 + 4, but the walk adds 1.0 three times to 2^53 and stays there
    r_over_T = (2.0 ** 53 + 2.0) / (2.0 ** 53 + 4.0)
    T = np.cumsum(CC.chunk_sums(m))[-1]
    assert T == 2.0 ** 53 + 4.0 and r_over_T * T == 2.0 ** 53 + 2.0
    assert CC.model_seed_pick(m, "kmeans++", r_over_T, [0]) == (1026, "chunk-last")
    # no distance left: the lowest row that is no seed yet
    assert CC.model_seed_pick(np.zeros(10), "kmeans++", 0.3, [0, 1, 3]) == (2, "no-distance")
    assert CC.model_seed_pick(np.zeros(10), "farthest", 0.3, [2, 0]) == (1, "no-distance")


@pytest.mark.parametrize("case", list(BLOBS))
def test_farthest_is_the_argmax(case):
    t = blobs(case)[0]
    history = []
    seeds, m, rules = CC.model_seeds(t, 8, init="farthest", history=history)
    x = t.astype(np.float64)
    assert seeds[0] == np.argmin(((x - x.mean(axis=0)) ** 2).sum(axis=1))
    for j in range(1, 8):
        assert seeds[j] == np.argmax(history[j - 1]["m"]) and rules[j] == "farthest"
    ties = np.array([0.0, 3.0, 1.0, 3.0])
    assert CC.model_seed_pick(ties, "farthest", 0.0, [0]) == (1, "farthest")  # of equal maxima the lower row


def test_duplicates_leave_empty_clusters():
    t = K.case_table("dups")
    assert len(np.unique(t, axis=0)) == 3
    for init in CC.INITS:
        seeds, m, rules = CC.model_seeds(t, 5, seed=1, init=init)
        assert rules[3:] == ["no-distance", "no-distance"] and (m == 0.0).all() and len(set(seeds.tolist())) == 5
        assert len(np.unique(t[seeds[:3]], axis=0)) == 3
        fit = CC.model_fit(t, 5, seed=1, init=init)
        assert fit["counts"].tolist() == sorted(K.DUP_COUNTS, reverse=True) + [0, 0] and fit["empty_clusters"] == 2
        assert fit["code_index"][3:].tolist() == [-1, -1] and np.isinf(fit["code_dist2"][3:]).all()
        assert fit["inertia"] == 0.0 and (fit["within_ss"] == 0.0).all()
        for c in range(3):  # the medoid is the cluster's lowest row, at distance zero
            assert fit["code_index"][c] == np.nonzero(fit["labels"] == c)[0][0] and fit["code_dist2"][c] == 0.0


def test_numbering_by_count_and_the_final_pass():
    t, _ = blobs("n4096_d32_k8")
    x = t.astype(np.float64)
    fit = CC.model_fit(t, 8, seed=5)
    k, n = 8, len(t)
    assert sorted(fit["order"].tolist()) == list(range(k))
    counts = fit["counts"]
    assert (np.diff(counts) <= 0).all() and np.array_equal(np.bincount(fit["labels"], minlength=k), counts) and counts.sum() == n
    for i in range(k - 1):  # ties: the lower original number first
        assert counts[i] > counts[i + 1] or fit["order"][i] < fit["order"][i + 1]
    d2 = ((x[:, None, :] - fit["centers"][None]) ** 2).sum(axis=2)
    near = d2[np.arange(n), fit["labels"]]
    assert (near <= d2.min(axis=1) * (1 + 1e-12)).all()
    for c in range(k):
        members = np.nonzero(fit["labels"] == c)[0]
        if len(members) == 0:
            assert fit["code_index"][c] == -1
            continue
        assert fit["labels"][fit["code_index"][c]] == c
        assert fit["code_dist2"][c] == CC.model_d2(x[members], fit["centers"][c]).min()
        np.testing.assert_allclose(fit["within_ss"][c], near[members].sum(), rtol=1e-12)
    assert fit["inertia"] == np.cumsum(fit["within_ss"])[-1]
    # the same rows in reverse order: other cluster numbers on the way, the same sizes in the same (descending) order at the end
    assert CC.model_fit(t[::-1].copy(), 8, seed=5, init="farthest")["counts"].tolist() == CC.model_fit(t, 8, init="farthest")["counts"].tolist()


def test_max_iter_one_does_not_converge():
    t, _ = blobs("n257_d3_k4")
    fit = CC.model_fit(t, 4, seed=3, max_iter=1)
    assert fit["iterations"] == 1 and not fit["converged"]


def _exact_tenth(c):
    """the float32 nearest to c / 10 in exact arithmetic, ties to the even mantissa"""
    q = Fraction(c) / 10
    guess = np.float32(c / 10.0)
    cands = [guess, np.nextafter(guess, np.float32(np.inf)), np.nextafter(guess, np.float32(-np.inf))]
    return min(cands, key=lambda f: (abs(Fraction(float(f)) - q), int(f.view(np.uint32)) & 1))


def test_v_is_the_centres_over_ten_rounded_once(tmp_path):
    rng = np.random.Generator(np.random.PCG64(8))
    # centres whose tenth lies next to a float32 tie, where rounding twice (float64, then float32) could go wrong if it ever did
    a = rng.standard_normal(200).astype(np.float32)
    mid = (a.astype(np.float64) + np.nextafter(a, np.float32(np.inf)).astype(np.float64)) / 2
    ten = mid * 10.0  # (exact: 29 bits) so its float64 neighbours have a tenth just off the tie
    c = np.concatenate([np.nextafter(ten, np.inf), np.nextafter(ten, -np.inf), rng.standard_normal(200) * 7, [0.0, -0.0, 1e-44, 3e38]])
    v = CC.tenth_float32(c.reshape(4, -1))
    assert v.dtype == np.float32 and v.shape == (4, 151)
    want = np.array([_exact_tenth(ci) for ci in c.tolist()], np.float32)
    assert np.array_equal(v.reshape(-1).view(np.uint32), want.view(np.uint32))
    t, _ = blobs("n4096_d32_k8")
    fit = CC.model_fit(t, 8, seed=5)
    back = fit["v"].astype(np.float64) * 10.0  # what DEMO.CODE_PATH's reader decodes, in exact arithmetic
    assert (np.abs(back - fit["centers"]) <= 2.0 ** -24 * np.abs(fit["centers"])).all()  # one float32 rounding (no subnormals here)
    path = CC.write_clusters(str(tmp_path / "sub" / "clusters"), fit)  # (a path without .npz is written as given)
    z = np.load(path)
    want = {"centers": ((8, 32), np.float64), "v": ((8, 32), np.float32), "code_index": ((8,), np.int64), "code_dist2": ((8,), np.float64),
            "counts": ((8,), np.int32), "labels": ((4096,), np.int32), "within_ss": ((8,), np.float64), "inertia": ((), np.float64),
            "seeds": ((8,), np.int64), "order": ((8,), np.int32), "iterations": ((), np.int64), "converged": ((), np.bool_),
            "empty_clusters": ((), np.int64)}
    assert sorted(z.files) == sorted(want)
    for key, (shape, dtype) in want.items():
        assert z[key].shape == shape and z[key].dtype == dtype, key
    assert np.array_equal(z["v"], fit["v"]) and os.path.getsize(path) < (1 << 20)


def test_argument_checks():
    t, _ = blobs("n257_d3_k4")
    for bad in (dict(k=0), dict(k=65), dict(k=258), dict(k=2.0), dict(k=True), dict(k=4, init="random"), dict(k=4, max_iter=0), dict(k=4, max_iter=1.5)):
        with pytest.raises(ValueError):
            CC.model_fit(t, **bad)
    with pytest.raises(ValueError, match="2\\^24"):
        CC._check_args((1 << 24) + 1, 8, "kmeans++", 100)
    assert CC._check_args(1 << 24, 64, "farthest", 1) == (64, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a host tensor: there is no CPU path
        CC.fit_clusters(torch.from_numpy(t.copy()), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CC.choose_seeds(torch.from_numpy(t.copy()), 4)


def test_c_abi_refuses_unsupported_sizes_before_any_launch():
    """outside 2 <= N <= 2^24, 2 <= D <= 64, 1 <= k <= 64, k <= N the workspace queries return 0 and the entry points SDT_ERR_UNSUPPORTED"""
    import ctypes as C

    from speechdrivestemplates_amd import _lib
    lib = _lib.load()
    assert lib.sdt_code_clusters_seed_workspace_bytes(30000, 32) == 30 * 40
    assert lib.sdt_code_clusters_update_workspace_bytes(30000, 32, 8) == 30 * 8 * 32 * 8 + 30 * 8 * 4
    assert lib.sdt_code_clusters_update_workspace_bytes(1 << 24, 64, 64) == (1 << 14) * 64 * 64 * 8 + (1 << 14) * 64 * 4  # 512 MiB of partials
    assert lib.sdt_code_clusters_final_workspace_bytes(30000, 32, 8) >= 30000 * 8
    for n, d in ((1, 32), (1000, 1), (1000, 65), ((1 << 24) + 1, 32)):
        assert lib.sdt_code_clusters_seed_workspace_bytes(n, d) == 0, (n, d)
    for n, d, k in ((1, 32, 1), (1000, 1, 8), (1000, 65, 8), (1000, 32, 0), (1000, 32, 65), (5, 32, 6), ((1 << 24) + 1, 32, 8)):
        assert lib.sdt_code_clusters_update_workspace_bytes(n, d, k) == 0, (n, d, k)
        assert lib.sdt_code_clusters_final_workspace_bytes(n, d, k) == 0, (n, d, k)
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    assert lib.sdt_code_clusters_seed_update(p, 1000, 65, p, 0, 1, p, p, 1 << 20, None) == -3
    assert lib.sdt_code_clusters_seed_update(p, (1 << 24) + 1, 32, p, 0, 1, p, p, 1 << 20, None) == -3
    assert lib.sdt_code_clusters_seed_update(p, 1000, 32, p, 64, 0, p, p, 1 << 20, None) == -3
    assert lib.sdt_code_clusters_seed_pick(p, 1, 0, 0.5, p, 1, p, p, 1 << 20, None) == -3
    assert lib.sdt_code_clusters_seed_pick(p, 5, 0, 0.5, p, 5, p, p, 1 << 20, None) == -3
    assert lib.sdt_code_clusters_assign(p, 1000, 32, p, 65, p, 1, p, None) == -3
    assert lib.sdt_code_clusters_assign(p, 5, 32, p, 6, p, 1, p, None) == -3
    assert lib.sdt_code_clusters_update(p, 1000, 1, p, 8, p, p, p, 1 << 20, None) == -3
    assert lib.sdt_code_clusters_final(p, 1000, 32, p, 0, p, p, p, p, p, p, p, p, p, 1 << 20, None) == -3
    assert lib.sdt_code_clusters_seed_pick(p, 1000, 2, 0.5, p, 1, p, p, 1 << 20, None) == -1  # an unknown mode: an argument error
    assert lib.sdt_code_clusters_seed_pick(p, 1000, 0, 1.5, p, 1, p, p, 1 << 20, None) == -1
    assert lib.sdt_code_clusters_update(p, 1000, 32, p, 8, p, p, p, 8, None) == -1  # workspace too small
    assert b"sdt_code_clusters_update" in lib.sdt_last_error()
    with pytest.raises(ValueError, match="k must lie"):
        CC._check(lib.sdt_code_clusters_assign(p, 1000, 32, p, 0, p, 1, p, None))
