"""csrc/bootstrap.hip against the numpy contract of speechdrivestemplates_amd/bootstrap.py: every word of every stage, bit for bit; the
accumulator front end; TEST.BOOTSTRAP in validate()."""
import numpy as np
import pytest
import torch

from speechdrivestemplates_amd import bootstrap as bs
from speechdrivestemplates_amd import clip_metrics as cm
from test_bootstrap_host import BIG_SEED, bits, records
from test_clip_metrics_host import alphas_for, part_table, poses

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 7
SIZES = cm.part_sizes(part_table(K))


def rank_tables(n, N, ranks, seed, **kw):
    """``ranks`` tables of N rows over n live clips (the first and the last row dead; the other dead rows unseen or nonfinite).  Rank r owns
    the live clips i with i % ranks == r; a higher rank also holds another record for every second clip of the rank below."""
    rng = np.random.Generator(np.random.PCG64(seed + 31 * n))
    live = 1 + np.sort(rng.permutation(N - 2)[:n])
    recs, spoiled = records(n, seed=seed, **kw), records(n, seed=seed + 1, **kw)
    bad = np.setdiff1d(np.arange(N), live)[::2]
    tables = np.zeros((ranks, N, cm.COLS), dtype=np.int64)
    for r in range(ranks):
        own = np.arange(n) % ranks == r
        tables[r, live[own]] = recs[own]
        if r > 0:
            below = (np.arange(n) % ranks == r - 1) & (np.arange(n) % 2 == 0)
            tables[r, live[below]] = spoiled[below]
        tables[r, bad] = records(len(bad), seed=seed + 2 + r, **kw)
        tables[r, bad, cm.NONFINITE] = 1
    return tables


def same_stages(got, want):
    assert set(got) == set(want) and got['n'] == want['n']
    for k, w in want.items():
        if k != 'n':
            g = got[k]
            assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
            assert np.array_equal(g.view(np.int64), w.view(np.int64)), k


# (n live, table rows, ranks, T, copies, alphas, R, rank a, seed)
CASES = [(1, 3, 1, 2, 1, 1, 100, 0, 0), (63, 70, 2, 5, 3, 2, 257, 127, BIG_SEED), (64, 66, 1, 2, 1, 3, 100, 49, 0), (65, 100, 3, 5, 3, 4, 257, 6, 0),
         (130, 200, 3, 2, 1, 2, 1000, 25, BIG_SEED), (130, 132, 2, 5, 3, 2, 1000, 499, 0), (64, 200, 1, 5, 3, 2, 100, 0, BIG_SEED)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-N%d-ranks%d-T%d-m%d-A%d-R%d-a%d-seed%d" % c)
def test_every_stage_matches_the_model(case):
    n, N, ranks, T, m, A, R, a, seed = case
    tables = rank_tables(n, N, ranks, seed=n + T, T=T, K=K, m=m, n_alphas=A)
    want = bs.stages_model(list(tables), None, SIZES, A, R, a, seed)
    assert want['n'] == n
    on_dev = torch.from_numpy(tables).to(DEV)
    got = bs.device_stages(on_dev, None, SIZES, A, R, a, seed)
    same_stages(got, want)
    same_stages(bs.device_stages(list(on_dev.unbind(0)), None, SIZES, A, R, a, seed), want)  # a second call, a list of tables: the same bits
    epoch = cm.epoch_model(list(tables), SIZES, A)
    assert np.array_equal(bits(got['values_a'][R]), epoch[:36]) and got['pair_frames_a'][R] == epoch[cm.OUT_PAIR_FRAMES]
    named = bs.named_intervals(got, alphas_for(A), R)
    assert ('diversity' in named) == (m > 1) and all(lo <= hi for _, lo, hi in named.values())


@pytest.mark.parametrize("case", [(65, 100, 2, 2, 3, 2, 100, 2, 0), (130, 200, 3, 5, 1, 4, 257, 127, BIG_SEED)],
                         ids=lambda c: "n%d-N%d-ranks%d-T%d-m%d-A%d-R%d-a%d-seed%d" % c)
def test_paired_form_matches_the_model(case):
    n, N, ranks, T, m, A, R, a, seed = case
    ta = rank_tables(n, N, ranks, seed=n + T, T=T, K=K, m=m, n_alphas=A)
    tb = rank_tables(n, N, 1, seed=n + T, T=T, K=K, m=m, n_alphas=A)
    tb[0, :, 0:4] = bits(tb[0, :, 0:4].copy().view(np.float64) * 0.5)  # the same clips with every l2_sum halved ...
    seen = np.flatnonzero(tb[0, :, cm.SEEN] != 0)
    tb[0, seen[3:8], cm.SEEN] = 0  # ... but live on other clips: five unseen, four more nonfinite
    tb[0, seen[10:14], cm.NONFINITE] = 1
    want = bs.stages_model(list(ta), list(tb), SIZES, A, R, a, seed)
    assert 0 < want['n'] < n
    da, db = torch.from_numpy(ta).to(DEV), torch.from_numpy(tb).to(DEV)
    got = bs.device_stages(da, db, SIZES, A, R, a, seed)
    same_stages(got, want)
    assert (got['signs'].sum(axis=1) == R).all() and (got['signs'][0:4, 1] == R).all()  # A's L2 is above B's in every replicate
    alphas = alphas_for(A)
    assert bs.clip_metric_paired(da, db, SIZES, alphas, R, 0.5, seed) == bs.paired_model(ta, tb, SIZES, alphas, R, 0.5, seed)
    same = bs.clip_metric_paired(da, da, SIZES, alphas, R, 0.9, seed)
    assert same and all(bits(v['diff']) == 0 and bits(v['diff_lo']) == 0 and v['share_a_less'] == v['share_a_greater'] == 0 for v in same.values())


def test_no_live_clip_launches_no_selection(monkeypatch):
    tables = rank_tables(5, 9, 2, seed=1, K=K)
    tables[:, :, cm.NONFINITE] = 1
    calls, orig = [], bs._call
    monkeypatch.setattr(bs, "_call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    on_dev = torch.from_numpy(tables).to(DEV)
    assert bs.clip_metric_intervals(on_dev, SIZES, [0.1, 0.2], 100, 0.9, 0) == {}
    assert bs.clip_metric_paired(on_dev, on_dev, SIZES, [0.1, 0.2], 100, 0.9, 0) == {}
    assert calls == ["sdt_clip_metrics_replicate_dense"] * 2
    same_stages(bs.device_stages(on_dev, None, SIZES, 2, 100, 0, 0), bs.stages_model(list(tables), None, SIZES, 2, 100, 0, 0))


def test_accumulator_front_end_and_the_point_row():
    """the point values are result()'s bits, over the accumulator's own table and over gathered states"""
    T, m, N, alphas = 3, 2, 70, [0.1, 0.2]
    parts = part_table(K)
    accs = [cm.ClipMetricsAccumulator(N, K, alphas, DEV, parts=parts) for _ in range(2)]
    for r, acc in enumerate(accs):
        idx = np.arange(1 + r, N - 1, 3 - r)  # holes, the first and last row dead, and clips that both ranks hold
        pred, gt = poses(m * len(idx), T, K, seed=r)
        if r == 1:
            pred[0, 0, 0, 0] = np.nan  # one nonfinite clip
        acc.add(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(idx), m)
    for acc, gathered in ((accs[0], None), (accs[1], None), (accs[0], torch.stack([a.state() for a in accs]))):
        res, st = acc.result(gathered), {}
        ci = bs.clip_metric_intervals(acc, replicates=100, level=0.9, seed=3, gathered=gathered, stages=st)
        assert st['n'] == res['clips_seen'] - res['clips_nonfinite'] > 0
        assert list(ci) == ['L2'] + [k for k in res if k not in ('clips_nonfinite', 'clips_seen', 'index_errors')]
        for k, (point, lo, hi) in ci.items():
            assert lo <= point <= hi and (k == 'L2' or bits(point) == bits(res[k])), k
        tables = [acc.table()] if gathered is None else [g[:N] for g in gathered]
        assert ci == bs.intervals_model([t.cpu().numpy() for t in tables], SIZES, alphas, 100, 0.9, 3)
    with pytest.raises(ValueError, match="part sizes and alphas"):
        bs.clip_metric_intervals(accs[0].table())
    with pytest.raises(ValueError, match="replicates"):
        bs.clip_metric_intervals(accs[0], replicates=99)


def test_command_line_prints_the_intervals(tmp_path, capsys):
    ta = rank_tables(65, 100, 1, seed=3, K=K, m=2)[0]
    tb = ta.copy()
    tb[:, 0:4] = bits(ta[:, 0:4].copy().view(np.float64) * 0.5)
    cm.save_table(str(tmp_path / "a.npz"), ta, [0.1, 0.2])
    cm.save_table(str(tmp_path / "b.npz"), tb, [0.1, 0.2])
    opts = ["--replicates", "100", "--level", "0.9", "--seed", "4", "--part-sizes"] + [str(s) for s in SIZES]
    assert bs.main([str(tmp_path / "a.npz"), "--out", str(tmp_path / "ci.npz")] + opts) == 0
    want = bs.intervals_model(ta, SIZES, [0.1, 0.2], 100, 0.9, 4)
    assert capsys.readouterr().out.splitlines() == ["%s: %r [%r, %r]" % ((k,) + v) for k, v in want.items()]
    with np.load(str(tmp_path / "ci.npz")) as z:
        assert list(z["keys"]) == list(want) and z["lo"].tolist() == [v[1] for v in want.values()] and int(z["replicates"]) == 100
    assert bs.main(["compare", str(tmp_path / "a.npz"), str(tmp_path / "b.npz")] + opts) == 0
    pair = bs.paired_model(ta, tb, SIZES, [0.1, 0.2], 100, 0.9, 4)
    assert capsys.readouterr().out.splitlines() == [
        "%s: %r %r %r [%r, %r] %r" % (k, v["a"], v["b"], v["diff"], v["diff_lo"], v["diff_hi"], v["share_a_less"]) for k, v in pair.items()]
    cm.save_table(str(tmp_path / "c.npz"), tb, [0.1])
    with pytest.raises(ValueError, match="differ in shape or alphas"):
        bs.main(["compare", str(tmp_path / "a.npz"), str(tmp_path / "c.npz")] + opts)


def test_size_checks_of_the_library():
    import ctypes as C
    from speechdrivestemplates_amd import _lib
    lib, p = _lib.load(), lambda t: C.c_void_p(t.data_ptr())
    w = torch.zeros(1 << 14, dtype=torch.int64, device=DEV)
    ptrs, sizes = (C.c_void_p * 1)(w.data_ptr()), (C.c_int64 * 4)(7, 3, 2, 2)
    assert lib.sdt_clip_metrics_replicate_dense(ptrs, 0, None, 0, 4, p(w), p(w), None, p(w), None, p(w), None) == -1
    assert lib.sdt_clip_metrics_replicate_dense(ptrs, 1, None, 1, 4, p(w), p(w), None, p(w), None, p(w), None) == -1
    assert lib.sdt_clip_metrics_replicate_dense(ptrs, 1, None, 0, 0, p(w), p(w), None, p(w), None, p(w), None) == -1
    assert lib.sdt_bootstrap_sums(p(w), 0, 39, 20, 100, 0, p(w), p(w), None) == -1
    assert lib.sdt_bootstrap_sums(p(w), 4, 65, 20, 100, 0, p(w), p(w), None) == -1
    assert lib.sdt_bootstrap_sums(p(w), 4, 39, 40, 100, 0, p(w), p(w), None) == -1
    assert lib.sdt_bootstrap_sums(p(w), 4, 39, 20, 65536, 0, p(w), p(w), None) == -1
    assert lib.sdt_clip_metrics_replicate_values(p(w), 1, sizes, 5, p(w), p(w), None) == -1
    assert lib.sdt_bootstrap_diff_f64(p(w), p(w), 0, p(w), None) == -1
    assert lib.sdt_bootstrap_intervals_f64(p(w), 100, 36, 50, p(w), None, None) == -1
    assert lib.sdt_bootstrap_intervals_f64(p(w), 100, 0, 2, p(w), None, None) == -1
    torch.cuda.synchronize()
    assert not w.any()


def _set_keys(cfg, clip=False, boot=False, fit=False):
    cfg.defrost()
    cfg.TEST.CLIP_METRICS, cfg.TEST.MULTIPLE = clip, 1
    cfg.TEST.BOOTSTRAP.ENABLE, cfg.TEST.BOOTSTRAP.REPLICATES, cfg.TEST.BOOTSTRAP.LEVEL, cfg.TEST.BOOTSTRAP.SEED = boot, 100, 0.9, 11
    cfg.TEST.FIT_CODE.ENABLE, cfg.TEST.FIT_CODE.STEPS = fit, 3
    cfg.freeze()


def test_validate_with_the_key_off_and_on(monkeypatch, tmp_path):
    from oracle import sdt_oracle as O
    from test_clip_metrics_gpu import NEW_KEYS
    from test_fgd_gpu import _validation_pipeline
    pipe, cfg = _validation_pipeline()
    losses, _ = pipe.forward_backward(O.make_batch(4, 16, step=0, seed=1))
    pipe.optimizer_updates(losses)
    calls, orig = [], bs._call
    monkeypatch.setattr(bs, "_call", lambda name, *a: (calls.append(name), orig(name, *a))[1])

    def run(**keys):
        _set_keys(cfg, **keys)
        torch.manual_seed(5)
        return pipe.validate(pipe.test_dataloader, 1)

    clip_keys = [k for k in NEW_KEYS if not k.startswith("diversity")]
    metric_keys = [k for k in clip_keys if k != "clips_nonfinite"]
    pipe.base_path = str(tmp_path)
    try:
        none = run()
        off = run(clip=True)
        assert list(off) == list(none) + clip_keys and not calls  # the key off: the parent's keys, nothing of the bootstrap launched
        assert not (tmp_path / "results" / "epoch1-VAL-clip_bootstrap.npz").exists()
        on = run(clip=True, boot=True)
        ends = [k + e for k in metric_keys for e in ("_lo", "_hi")]
        assert list(on) == list(off) + ends and calls
        for k in off:
            assert torch.equal(torch.as_tensor(on[k]), torch.as_tensor(off[k])), k
        for k in metric_keys:
            print("  %-20s %.17g in [%.17g, %.17g]" % (k, on[k], on[k + "_lo"], on[k + "_hi"]))
            assert on[k + "_lo"] <= on[k] <= on[k + "_hi"], k
        with np.load(str(tmp_path / "results" / "epoch1-VAL-clip_metrics.npz")) as z:
            table, alphas = z["table"], z["alphas"].tolist()
        sizes = cm.part_sizes(part_table(121))
        ci = bs.clip_metric_intervals(torch.from_numpy(table).to(DEV), sizes, alphas, 100, 0.9, 11)
        assert all((on[k], on[k + "_lo"], on[k + "_hi"]) == ci[k] for k in metric_keys)
        assert ci == bs.intervals_model(table, sizes, alphas, 100, 0.9, 11)
        with np.load(str(tmp_path / "results" / "epoch1-VAL-clip_bootstrap.npz")) as z:
            assert z["values"].shape == (100, 36) and tuple(z["names"]) == bs.VALUE_NAMES and z["point"].shape == (36,)
            assert (int(z["n"]), int(z["replicates"]), float(z["level"]), int(z["seed"])) == (8, 100, 0.9, 11)
            assert z["part_sizes"].tolist() == list(sizes) and z["point"][cm.OUT_PCK_MEAN] == on["PCK"]
            assert np.sort(z["values"][:, cm.OUT_PCK_MEAN])[5] == on["PCK_lo"]
        # with the fit: the _fit keys get their ends, and the paired run the three gains
        fit = run(clip=True, boot=True, fit=True)
        assert [k for k in fit if k.endswith(("_lo", "_hi"))] == ends + [k + "_fit" + e for k in metric_keys for e in ("_lo", "_hi")] + [
            k + "_fit_gain" + e for k in bs.GAIN_KEYS for e in ("_lo", "_hi")]
        for k in metric_keys:
            assert fit[k + "_fit_lo"] <= fit[k + "_fit"] <= fit[k + "_fit_hi"] and fit[k + "_lo"] == on[k + "_lo"], k
        gain = bs.clip_metric_paired(pipe.val_observers()[3].acc, pipe.clip_metrics(), replicates=100, level=0.9, seed=11)
        for k in bs.GAIN_KEYS:
            assert gain[k]["a"] == fit[k + "_fit"] and gain[k]["b"] == fit[k] and gain[k]["diff"] == fit[k + "_fit"] - fit[k], k
            assert (fit[k + "_fit_gain_lo"], fit[k + "_fit_gain_hi"]) == (gain[k]["diff_lo"], gain[k]["diff_hi"]), k
    finally:
        pipe.base_path = None
        _set_keys(cfg)
