"""The code clusters on the GPU (csrc/code_clusters.hip, code_clusters.py) against the numpy contract models of the
same file: bit for bit.  Every stage rounds every operation on its own in a fixed order (rows ascending inside chunks of 1024, chunks
ascending) and the models restate that order, so nothing here is compared by a tolerance: the distances ``m`` after every seed, the
seeds and the rule that chose each, the labels, centres, counts and ``changed`` of every iteration, and everything the final pass writes.
One thing the models do not restate is the summation order of ``sdt_code_pca_moments`` (not new), whose mean names seed 0 of the farthest
seeding: the model is given the device's seed 0, and that seed is checked to be the row nearest to the device's mean.  Then the
fallback rules of the seeding, max_iter = 1, determinism, the loud failures, and both demo modes reading the file the command line writes.
"""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_code_axes_gpu import _demo_pipeline, _train, bits, dev

sys.path.insert(0, GOLDEN)
import synth_cluster_tables as K  # noqa: E402

pytestmark = pytest.mark.gpu

FINAL_KEYS = ("labels", "centers", "counts", "within_ss", "inertia", "code_index", "code_dist2", "order", "v", "seeds")
_RUNS = {}


def CC():
    from speechdrivestemplates_amd import code_clusters
    return code_clusters


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def same(a, b):
    """equal shapes, dtypes and bits"""
    a, b = host(a), host(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def runs(case, init, max_iter=100):
    """(device fit, its history, model fit, its history) of a case, computed once"""
    key = (case, init, max_iter)
    if key not in _RUNS:
        cc = CC()
        t, k = K.case_table(case), K.CASES[case]["k"]
        dh, mh = [], []
        fit = cc.fit_clusters(dev(t), k, seed=1, init=init, max_iter=max_iter, history=dh)
        first = int(fit["seeds"][0].item()) if init == "farthest" else None
        model = cc.model_fit(t, k, seed=1, init=init, max_iter=max_iter, first_seed=first, history=mh)
        _RUNS[key] = (fit, dh, model, mh)
    return _RUNS[key]


def check_against_model(case, init, max_iter=100):
    cc = CC()
    t, k = K.case_table(case), K.CASES[case]["k"]
    n = t.shape[0]
    fit, dh, model, mh = runs(case, init, max_iter)
    assert len(dh) == len(mh) and [h["stage"] for h in dh] == [h["stage"] for h in mh]
    if init == "farthest":  # seed 0: the row nearest to the device's mean (the existing kernels)
        from speechdrivestemplates_amd import _lib
        from speechdrivestemplates_amd.code_pca import _moments
        mean, _ = _moments(_lib.load(), dev(t), torch.cuda.current_stream().cuda_stream)
        assert dh[0]["seed"] == int(np.argmin(cc.model_d2(t.astype(np.float64), mean.cpu().numpy())))
    for a, b in zip(dh, mh):
        if a["stage"] == "seed":
            assert a["seed"] == b["seed"] and np.array_equal(bits(a["m"]), bits(b["m"])), (case, init, a["j"])
            if a["j"]:
                assert cc.RULES[int(a["info"][3])] == b["rule"], (case, init, a["j"])
        else:
            assert a["changed"] == b["changed"] and (a["iteration"] > 1 or a["changed"] == n), (case, init, a["iteration"])
            assert same(a["labels"], b["labels"]) and same(a["counts"], b["counts"]), (case, init, a["iteration"])
            assert np.array_equal(bits(a["centers"]), bits(b["centers"])), (case, init, a["iteration"])
    for key in FINAL_KEYS:
        assert same(fit[key], model[key]), (case, init, key)
    for key in ("iterations", "converged", "empty_clusters", "n_rows", "dim"):
        assert fit[key] == model[key], (case, init, key)
    print("code_clusters %s %s: %d iterations, converged %s, counts %s, inertia %.6g" % (
        case, init, fit["iterations"], fit["converged"], host(fit["counts"]).tolist()[:8], float(fit["inertia"])))
    return fit, dh


# -- (a) every stage against its model, both seedings ----------------------------------------------------------------------------------
@pytest.mark.parametrize("init", ["kmeans++", "farthest"])
@pytest.mark.parametrize("case", list(K.CASES))
def test_fit_clusters_equals_the_models(case, init):
    t, k = K.case_table(case), K.CASES[case]["k"]
    n, d = t.shape
    fit, dh = check_against_model(case, init)
    for key, shape, dtype in (("centers", (k, d), torch.float64), ("v", (k, d), torch.float32), ("code_index", (k,), torch.int64),
                              ("code_dist2", (k,), torch.float64), ("counts", (k,), torch.int32), ("labels", (n,), torch.int32),
                              ("within_ss", (k,), torch.float64), ("inertia", (), torch.float64), ("seeds", (k,), torch.int64),
                              ("order", (k,), torch.int32)):
        assert fit[key].shape == shape and fit[key].dtype == dtype and fit[key].is_cuda, key
    counts, labels, index = host(fit["counts"]), host(fit["labels"]), host(fit["code_index"])
    assert counts.sum() == n and (np.diff(counts) <= 0).all() and np.array_equal(np.bincount(labels, minlength=k), counts)
    assert all(index[c] == -1 if counts[c] == 0 else labels[index[c]] == c for c in range(k))
    its = [h for h in dh if h["stage"] == "iteration"]
    # converged at iteration >= 2: the last update changed no bit of the centres, and the final labels are the loop's
    assert fit["converged"] and fit["iterations"] >= 2
    assert np.array_equal(bits(its[-1]["centers"]), bits(its[-2]["centers"]))
    assert np.array_equal(host(fit["order"])[labels], its[-1]["labels"])
    assert np.array_equal(bits(fit["centers"]), bits(its[-1]["centers"][host(fit["order"])]))
    if case == "n5_d3_k5":  # every row a seed and its own centre
        assert sorted(host(fit["seeds"]).tolist()) == list(range(5)) and counts.tolist() == [1] * 5
        assert float(fit["inertia"]) == 0.0 and sorted(index.tolist()) == list(range(5))
    if case == "dups":  # after three seeds no distance is left; the repeated centres lose every tie to the lower cluster
        seeds = host(fit["seeds"])
        assert [CC().RULES[int(h["info"][3])] for h in dh[3:5]] == ["no-distance"] * 2 and len(set(seeds.tolist())) == 5
        assert counts.tolist() == sorted(K.DUP_COUNTS, reverse=True) + [0, 0] and fit["empty_clusters"] == 2
        assert index[3:].tolist() == [-1, -1] and float(fit["inertia"]) == 0.0
        assert sorted(host(fit["order"])[3:].tolist()) == [3, 4]


@pytest.mark.parametrize("init", ["kmeans++", "farthest"])
def test_max_iter_one_is_not_converged(init):
    fit, dh = check_against_model("n2049_d33_k7", init, max_iter=1)
    assert fit["iterations"] == 1 and not fit["converged"] and dh[-1]["changed"] == 2049


# -- (b) the rules of the k-means++ pick that no seeded table reaches -----------------------------------------------------------------------
def _pick(table, seed_row, u):
    """m after one seed, then one k-means++ pick with the given u -> (row, rule, m)"""
    from speechdrivestemplates_amd import _lib
    cc = CC()
    lib = _lib.load()
    x = dev(table)
    n, d = x.shape
    raw = torch.cuda.current_stream().cuda_stream
    p = cc._p
    ws_bytes = lib.sdt_code_clusters_seed_workspace_bytes(n, d)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device="cuda")
    seeds = torch.tensor([seed_row, -1], dtype=torch.int64, device="cuda")
    m, info = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(4, dtype=torch.float64, device="cuda")
    cc._check(lib.sdt_code_clusters_seed_update(p(x), n, d, p(seeds), 0, 1, p(m), p(ws), ws_bytes, raw))
    cc._check(lib.sdt_code_clusters_seed_pick(p(m), n, 0, C.c_double(u), p(seeds), 1, p(info), p(ws), ws_bytes, raw))
    return int(seeds[1].item()), cc.RULES[int(info[3].item())], m.cpu().numpy()


def test_seed_pick_fallback_rules():
    cc = CC()
    # r == T (u == 1; a u < 1 always rounds below T): no chunk passes, the table's last row with a distance
    t = np.zeros((3000, 2), np.float32)
    t[5, 0], t[1030, 0], t[2500, 1] = 1.0, 2.0, 1.5
    row, rule, m = _pick(t, 0, 1.0)
    assert (row, rule) == (2500, "table-last") == cc.model_seed_pick(m, "kmeans++", 1.0, [0])
    assert np.array_equal(m, cc.model_d2(t.astype(np.float64), np.zeros(2))) and m[[5, 1030, 2500]].tolist() == [1.0, 4.0, 2.25]
    row, rule, _ = _pick(t, 0, 0.5)  # P = 1, 5, 7.25; r = 3.625: chunk 1
    assert (row, rule) == (1030, "walk") == cc.model_seed_pick(m, "kmeans++", 0.5, [0])
    # the chunk's own sum passes r, the walk from P[c - 1] does not: 2^53 + 1.0 three times stays 2^53, while P[1] = 2^53 + 3 -> 2^53 + 4
    t = np.zeros((2048, 2), np.float32)
    t[0] = 2.0 ** 26
    t[1024:1027, 0] = 1.0
    u = (2.0 ** 53 + 2.0) / (2.0 ** 53 + 4.0)
    row, rule, m = _pick(t, 1, u)
    assert m[0] == 2.0 ** 53 and m[1] == 0.0
    assert (row, rule) == (1026, "chunk-last") == cc.model_seed_pick(m, "kmeans++", u, [1])


# -- (c) determinism -------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    cc = CC()
    t = dev(K.case_table("n2049_d33_k7"))
    a, b = cc.fit_clusters(t, 7, seed=1), cc.fit_clusters(t, 7, seed=1)
    for key in FINAL_KEYS:
        assert same(a[key], b[key]), key
    assert same(a["labels"], runs("n2049_d33_k7", "kmeans++")[0]["labels"]) and a["iterations"] == b["iterations"]
    assert not same(a["seeds"], cc.fit_clusters(t, 7, seed=2)["seeds"])  # (the seed does reach the draw)


# -- (d) loud failures: argument checks and error words, never an out-of-range access ---------------------------------------------------------
def test_loud_failures():
    from speechdrivestemplates_amd import _lib
    cc = CC()
    t = K.case_table("n2049_d33_k7")
    u = t.copy()
    u[123, 5] = np.nan
    u[2000, 0] = np.inf  # a later bad row does not change the one that is named
    for init in cc.INITS:
        with pytest.raises(ValueError, match=r"non-finite entry in row 123$"):
            cc.fit_clusters(dev(u), 7, init=init)
    for shape, k in (((100, 1), 4), ((100, 65), 4), ((1, 32), 1), ((100, 32), 0), ((100, 32), 65), ((5, 32), 6)):
        with pytest.raises(ValueError):
            cc.fit_clusters(torch.zeros(shape, device="cuda"), k)
    for bad in (dict(init="random"), dict(max_iter=0), dict(k=3.0)):
        with pytest.raises(ValueError):
            cc.fit_clusters(dev(t), **{"k": 7, **bad})
    with pytest.raises(TypeError):
        cc.fit_clusters(dev(t.astype(np.float64)), 7)
    lib = _lib.load()  # one row past the cap: the workspace queries only, nothing is allocated
    n = (1 << 24) + 1
    assert lib.sdt_code_clusters_seed_workspace_bytes(n, 32) == 0 and lib.sdt_code_clusters_update_workspace_bytes(n, 32, 8) == 0
    assert lib.sdt_code_clusters_final_workspace_bytes(n, 32, 8) == 0 and lib.sdt_code_clusters_final_workspace_bytes(n - 1, 32, 8) > 0
    with pytest.raises(ValueError, match="2\\^24"):
        cc._check_args(n, 8, "kmeans++", 100)


# -- (e) both demo modes read the file the command line writes ---------------------------------------------------------------------------------
def test_pose2pose_demo_decodes_one_sequence_per_cluster(tmp_path, capsys):
    cc = CC()
    ckpt = _train(tmp_path, "pose2pose")
    out = str(tmp_path / "clusters.npz")
    assert cc.main(["--checkpoint", ckpt, "--out", out, "--k", "3", "--seed", "4"]) == 0
    printed = capsys.readouterr().out
    z = np.load(out)
    assert z["v"].shape == (3, 32) and z["v"].dtype == np.float32 and z["centers"].shape == (3, 32) and z["labels"].shape == (8,)
    assert z["counts"].sum() == 8 and (np.diff(z["counts"]) <= 0).all()
    assert "module.clip_code_mu (8, 32): k=3" in printed and "DEMO.CODE_PATH %s DEMO.MULTIPLE 3" % out in printed
    assert "DEMO.CODE_INDEX %d DEMO.CODE_INDEX_B %d" % (z["code_index"][0], z["code_index"][1]) in printed
    assert all("cluster %d: count %d code_index %d " % (i, z["counts"][i], z["code_index"][i]) in printed for i in range(3))
    demo, cfg, wav = _demo_pipeline(tmp_path, "pose2pose", ["DEMO.CODE_PATH", out, "DEMO.MULTIPLE", 3])
    outs = demo.demo(cfg, "demo", ckpt, wav)
    assert len(outs) == 3
    batch = next(iter(demo.test_dataloader))
    for i, o in enumerate(outs):
        p = o["poses_pred_batch"]
        assert p.shape == (1, cfg.DATASET.NUM_FRAMES, 2, 121) and p.dtype == torch.float64 and torch.isfinite(p).all()
        code = torch.tensor(z["v"][i] * 10, dtype=torch.float32, device="cuda").unsqueeze(0)
        assert torch.equal(o["clip_code_mu"], code)
        with torch.no_grad():  # the model's external-code path, directly
            pred, _, _ = demo.model.ae(None, cfg.DATASET.NUM_FRAMES, external_code=code)
        assert torch.equal(p, demo.test_dataset.get_final_results(pred.detach(), batch["speaker_stat"]))
    assert not torch.equal(outs[0]["poses_pred_batch"], outs[1]["poses_pred_batch"])
    # the file's own numbers: the model on the table the checkpoint holds
    from speechdrivestemplates_amd.code_pca import load_code_table
    model = cc.model_fit(load_code_table(ckpt)[1].numpy(), 3, seed=4)
    for key in FINAL_KEYS:
        assert same(z[key], model[key]), key
    demo.close()


def test_voice2pose_demo_takes_the_medoids(tmp_path):
    cc = CC()
    ckpt = _train(tmp_path, "voice2pose_sdt_bp")
    out = str(tmp_path / "clusters.npz")
    assert cc.main(["--checkpoint", ckpt, "--out", out, "--table", "module.clips_code", "--k", "2", "--init", "farthest"]) == 0
    z = np.load(out)
    a, b = int(z["code_index"][0]), int(z["code_index"][1])
    assert z["code_index"].shape == (2,) and 0 <= a < 8 and 0 <= b < 8 and a != b and z["labels"][a] == 0 and z["labels"][b] == 1
    demo, cfg, wav = _demo_pipeline(tmp_path, "voice2pose_sdt_bp", ["DEMO.CODE_INDEX", a, "DEMO.CODE_INDEX_B", b, "DEMO.MULTIPLE", 2])
    outs = demo.demo(cfg, "demo", ckpt, wav)
    assert len(outs) == 2
    table = demo.model.clips_code.detach()
    assert torch.equal(outs[0]["condition_code"][0], table[a]) and torch.equal(outs[1]["condition_code"][0], table[b])
    model = cc.model_fit(table.cpu().numpy(), 2, init="farthest", first_seed=int(z["seeds"][0]))
    for key in FINAL_KEYS:
        assert same(z[key], model[key]), key
    demo.close()
