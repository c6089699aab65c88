"""The motion histograms on the GPU (csrc/motion_dist.hip, speechdrivestemplates_amd/motion_dist.py, TEST.MOTION_DIST)
against the numpy contract model.

Bars.  Every integer word (the 576 counts, seen, copies, nonfinite, frames) is equal whatever the square root does: bins are decided on
squares.  The float sums run the model's operations in the model's order, so where this device's float64 square root is correctly rounded
(``sqrt_is_exact`` asks the library's probe on 200 000 values and on the test's own arguments) they are bit-identical; otherwise they are
held to (n + 2) 2^-52 relative, n the number of terms (the bar of tests/test_motion_dist_host.py).  The epoch stage: integers and merged
histograms equal ``epoch_model`` of the device's own table; the floats bit for bit where the square root is exact on the epoch stage's own
arguments, otherwise |BC - BC_model| <= 34 2^-52 (32 terms <= 1 each off by at most one ulp, and the order is the same) and H is compared
through BC: H^2 = max(1 - BC, 0) to 4 2^-52.  Every comparison prints how many values were bit-identical before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

from speechdrivestemplates_amd import clip_metrics as cm
from speechdrivestemplates_amd import motion_dist as md
from speechdrivestemplates_amd import tb_events
from test_motion_dist_host import (CASES, EDGES, ULP, check_inf_records, check_nan_records, check_tie_records, inf_case, model_records, nan_case,
                                   part_table, poses, tie_case)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def device_sqrt_equals_numpy(x):
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())
    x = x[np.isfinite(x)]
    return x.size == 0 or np.array_equal(cm.device_sqrt(dev(x)).cpu().numpy(), np.sqrt(x))


@functools.lru_cache(maxsize=None)
def sqrt_is_exact():
    rng = np.random.Generator(np.random.PCG64(11))
    x = np.concatenate([rng.uniform(0, 4, 100000), np.exp(rng.uniform(-30, 30, 100000)), [0.0, 1.0, 2.0, 4.0, 2.0 ** -1040]])
    same = device_sqrt_equals_numpy(x)
    print("  device sqrt(float64) equals numpy's on %d values: %s" % (x.size, same))
    return same


def terms_of(pred, gt):
    """every argument of a square root the rows kernel takes on these inputs"""
    out = []
    with np.errstate(all='ignore'):
        for x in (pred, gt):
            for d in md._differences(x):
                out.append((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]).ravel())
    return np.concatenate(out)


def exact_on(pred, gt):
    return sqrt_is_exact() and device_sqrt_equals_numpy(terms_of(pred, gt))


def held(name, got, want, exact, T, parts):
    """records ``got`` (device) against ``want`` (model): integers equal; floats bit-identical, or within (n + 2) 2^-52 where sqrt is not exact"""
    assert np.array_equal(got[:, md.COUNT0:], want[:, md.COUNT0:]), "%s: integer words differ" % name
    gf, wf = got[:, :md.FLOATS].view(np.float64), want[:, :md.FLOATS].view(np.float64)
    same = int((got[:, :md.FLOATS] == want[:, :md.FLOATS]).sum())
    print("  %-40s %d of %d float sums bit-identical (sqrt exact on these inputs: %s)" % (name, same, gf.size, exact))
    if exact:
        assert same == gf.size, "%s: %d of %d float sums differ in bits" % (name, gf.size - same, gf.size)
        return
    m = want[:, md.COPIES].reshape(-1, 1, 1, 1)
    frames = np.array([max(T - 1 - o, 0) for o in range(3)]).reshape(1, 1, 3, 1)
    n = np.broadcast_to(m * frames * np.array(cm.part_sizes(parts)).reshape(1, 1, 1, 4), (len(got), 2, 3, 4)).reshape(gf.shape)
    ok = (np.abs(gf - wf) <= (n + 2) * ULP * np.abs(wf)) | ((gf != gf) & (wf != wf)) | (gf == wf)
    assert ok.all(), "%s: error %s" % (name, np.abs(gf - wf).max())


def committed(pred, gt, parts, m=1, index=None, num_clips=None, edges=EDGES):
    B = pred.shape[0] // m
    acc = md.MotionDistAccumulator(B if num_clips is None else num_clips, pred.shape[3], edges, DEV, parts=parts)
    acc.add(dev(pred), dev(gt), torch.arange(B, dtype=torch.int64) if index is None else index, m)
    return acc


def epoch_held(name, acc, tables, gathered=None):
    """``result_words`` / ``histograms`` of the device against ``epoch_model`` of ``tables`` -> the device's words"""
    got = acc.result_words(gathered)
    hist = acc.histograms()
    want, want_hist = md.epoch_model(tables, index_errors=int(got[md.OUT_INDEX_ERRORS]))
    assert np.array_equal(got[60:], want[60:]), "%s: integer words %s, model %s" % (name, got[60:], want[60:])
    assert np.array_equal(hist, want_hist), "%s: merged histograms differ" % name
    gf, wf = got[:60].view(np.float64), want[:60].view(np.float64)
    same = int((got[:60] == want[:60]).sum())
    merged = md.merge_tables(tables)
    merged[merged[:, md.NONFINITE] != 0] = 0  # (left out whole)
    floor = np.stack([md.with_all(md.unpack(merged)['counts'][i::2, 1].sum(axis=0)) for i in (0, 1)])
    args = []  # the arguments of the epoch stage's square roots
    for a, b in ((want_hist[0], want_hist[1]), (floor[0], floor[1])):
        na, nb = a.sum(axis=-1, keepdims=True), b.sum(axis=-1, keepdims=True)
        with np.errstate(all='ignore'):
            args.append(((a / na) * (b / nb)).ravel())
    exact = sqrt_is_exact() and device_sqrt_equals_numpy(np.concatenate(args + [np.maximum(1.0 - wf[12:24], 0), np.maximum(1.0 - wf[36:48], 0)]))
    print("  %-40s %d of 60 epoch floats bit-identical (sqrt exact on these arguments: %s)" % (name, same, exact))
    assert np.array_equal(got[md.OUT_RATIO:60], want[md.OUT_RATIO:60]), "%s: the ratios have no square root and must be equal" % name
    if exact:
        assert same == 60, "%s: %d of 60 epoch floats differ in bits" % (name, 60 - same)
    else:
        for h0, b0 in ((md.OUT_H, md.OUT_BC), (md.OUT_H_FLOOR, md.OUT_BC_FLOOR)):
            assert (np.abs(gf[b0:b0 + 12] - wf[b0:b0 + 12]) <= 34 * ULP).all(), name
            assert (np.abs(gf[h0:h0 + 12] ** 2 - np.maximum(1.0 - gf[b0:b0 + 12], 0)) <= 4 * ULP).all(), name
    return got


# (a) ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-m%d" % c)
def test_kernels_match_the_model(case):
    R, T, K, m = case
    pred, gt = poses(R, T, K)
    want = model_records(case)
    acc = committed(pred, gt, part_table(K), m)
    got = acc.table().cpu().numpy()
    held("R=%d T=%d K=%d m=%d" % case, got, want, exact_on(pred, gt), T, part_table(K))
    assert acc.state()[-1].cpu().tolist() == [0] * md.COLS  # the header: no index error, nothing else written
    if m == 1:  # the row records alone are the clip records of one copy
        assert np.array_equal(acc.row_records(dev(pred), dev(gt)).cpu().numpy(), got)
    epoch_held("epoch of R=%d T=%d K=%d m=%d" % case, acc, [got])


# (b) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_edges_out_of_range_nan_and_inf_on_the_device():
    pred, gt, parts = tie_case()
    got = committed(pred, gt, parts).table().cpu().numpy()
    check_tie_records(got)
    assert np.array_equal(got, md.motion_dist_model(pred, gt, parts, EDGES))  # (sqrt of an exact square and of 0: no rounding to differ in)
    pred, gt, parts = nan_case()
    acc = committed(pred, gt, parts)
    got = acc.table().cpu().numpy()
    clean = committed(np.nan_to_num(pred), gt, parts).table().cpu().numpy()
    check_nan_records(got, clean)
    want = md.motion_dist_model(pred, gt, parts, EDGES)
    assert np.array_equal(got[:, md.COUNT0:], want[:, md.COUNT0:])
    assert np.array_equal(np.isnan(got[:, :md.FLOATS].view(np.float64)), np.isnan(want[:, :md.FLOATS].view(np.float64)))
    words = epoch_held("epoch with a NaN clip", acc, [got])
    res = acc.result()
    assert res['motion_clips_nonfinite'] == 1 and res['motion_clips_seen'] == 3 and all(np.isfinite(v) for v in res.values())
    assert words[md.OUT_NONFINITE] == 1
    pred, gt, parts = inf_case()
    got = committed(pred, gt, parts).table().cpu().numpy()
    check_inf_records(got, committed(np.where(np.isinf(pred), 1e100, pred), gt, parts).table().cpu().numpy())
    # copies: a NaN in one copy of clip 1 flags clip 1 alone
    pred, gt = poses(6, 5, 5, seed=4)
    pred[3, 1, 1, 2] = np.nan  # row 3 = copy 1 of clip 1 (B = 2)
    got = committed(pred, gt, parts, 3).table().cpu().numpy()
    clean = committed(np.nan_to_num(pred), gt, parts, 3).table().cpu().numpy()
    assert got[:, md.NONFINITE].tolist() == [0, 1] and np.array_equal(got[0], clean[0])
    assert np.array_equal(got[:, md.COUNT0:], md.motion_dist_model(pred, gt, parts, EDGES, 3)[:, md.COUNT0:])


# (c) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_commit_writes_the_addressed_rows_and_counts_bad_indices():
    N, T, K, SENTINEL = 10, 5, 5, 0x5A5AA5A55A5AA5A5
    parts = part_table(K)
    pred, gt = poses(5, T, K, seed=5)
    acc = md.MotionDistAccumulator(N, K, EDGES, DEV, parts=parts)
    acc.state().fill_(SENTINEL)
    acc.state()[N].zero_()
    acc.add(dev(pred), dev(gt), torch.tensor([7, 2, -1, N, 4], dtype=torch.int64), 1)
    want = md.motion_dist_model(pred, gt, parts, EDGES)
    state = acc.state().cpu().numpy()
    exact = exact_on(pred, gt)
    held("rows 7, 2, 4", state[[7, 2, 4]], want[[0, 1, 4]], exact, T, parts)
    untouched = [r for r in range(N) if r not in (7, 2, 4)]
    assert (state[untouched] == SENTINEL).all()
    assert state[N, 0] == 2 and not state[N, 1:].any()  # the two bad indices are counted, and wrote nothing
    # a multiplied batch hands its index in multiplied: the first B entries are read; a clip written twice takes the second record
    pred2, gt2 = poses(2, T, K, seed=6)
    acc.add(dev(pred2), dev(gt2), torch.tensor([2, 2], dtype=torch.int64), 2)
    again = acc.state().cpu().numpy()
    held("row 2 again", again[[2]], md.motion_dist_model(pred2, gt2, parts, EDGES, 2), exact_on(pred2, gt2), T, parts)
    keep = [r for r in range(N + 1) if r != 2]
    assert again[2, md.COPIES] == 2 and np.array_equal(again[keep], state[keep])
    acc.reset()
    assert not acc.state().any()


# (d) ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 64, 65, 200])
def test_epoch_is_the_same_however_the_records_arrive(N):
    T, K, m = 5, 5, 2
    parts = part_table(K)
    rng = np.random.Generator(np.random.PCG64(N))
    seen = np.array([0]) if N == 1 else np.sort(rng.permutation(N)[:max(1, 3 * N // 4)])  # holes: a quarter of the clips arrive nowhere
    n = len(seen)
    pred, gt = poses(m * n, T, K, seed=N)
    if n > 4:
        pred[3, 2, 0, 1] = np.nan  # one record is nonfinite
    p5, g5 = pred.reshape(m, n, T, 2, K), gt.reshape(m, n, T, 2, K)

    def rows(a, sel):
        return dev(a[:, sel].reshape(m * len(sel), T, 2, K))

    def feed(acc, sel, spoil=False):
        acc.add(rows(p5 * 1.5 if spoil else p5, sel), rows(g5, sel), torch.from_numpy(seen[sel]), m)

    def fresh():
        return md.MotionDistAccumulator(N, K, EDGES, DEV, parts=parts)

    one = fresh()
    feed(one, rng.permutation(n))  # one add of all rows, shuffled
    table = one.table().cpu().numpy()
    words = epoch_held("N=%d, one add" % N, one, [table])
    hist = one.histograms()
    assert words[md.OUT_SEEN] == n and words[md.OUT_NONFINITE] == (1 if n > 4 else 0)
    ragged = fresh()
    for sel in np.array_split(np.arange(n), min(7, n)):  # up to 7 adds of ragged sizes: the same table bits
        feed(ragged, sel)
    assert torch.equal(ragged.state(), one.state()) and np.array_equal(ragged.result_words(), words)
    # three tables as ``gathered``: overlapping clips (the higher rank of an overlap holds another record, which must not be read), and
    # the last clip seen by the last table only
    ranks = [fresh() for _ in range(3)]
    body, last = np.arange(n - 1), np.array([n - 1])
    for r in range(3):
        own = body[body % 3 == r]
        if len(own):
            feed(ranks[r], own)
        other = body[(body % 3 == r - 1) & (body % 2 == 0)] if r > 0 else body[:0]
        if len(other):
            feed(ranks[r], other, spoil=True)
    feed(ranks[2], last)
    gathered = torch.stack([a.state() for a in ranks])
    assert np.array_equal(ranks[2].result_words(gathered), words) and np.array_equal(ranks[2].histograms(), hist)
    assert np.array_equal(ranks[0].result_words(ranks), words)
    epoch_held("N=%d, three tables" % N, ranks[1], [a.table().cpu().numpy() for a in ranks], gathered)
    if n >= 8:
        assert not np.array_equal(ranks[0].result_words(ranks[::-1]), words)  # (rank order matters where records differ)
    one.reset()
    assert one.result()['motion_clips_seen'] == 0
    feed(one, np.arange(n))
    assert np.array_equal(one.result_words(), words)


# (e) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_size_checks():
    with pytest.raises(ValueError, match="K = 129"):
        md.MotionDistAccumulator(4, 129, None, DEV, parts=[0] * 129)
    with pytest.raises(ValueError, match="ascending"):
        md.MotionDistAccumulator(4, 5, EDGES[:, ::-1].tolist(), DEV, parts=part_table(5))
    acc = md.MotionDistAccumulator(4, 5, None, DEV, parts=part_table(5))
    x = torch.zeros((17, 2, 2, 5), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="17 copies"):
        acc.add(x, x, torch.zeros(1, dtype=torch.int64), 17)
    with pytest.raises(ValueError):
        acc.add(x, x, torch.zeros(1, dtype=torch.int64), 2)  # 17 rows are not 2 copies
    with pytest.raises(TypeError):
        acc.add(x.float(), x.float(), torch.zeros(17, dtype=torch.int64), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        acc.add(x.cpu(), x.cpu(), torch.zeros(17, dtype=torch.int64), 1)
    # the library checks the same sizes before any launch
    import ctypes as C
    from speechdrivestemplates_amd import _lib
    lib, p = _lib.load(), lambda t: C.c_void_p(t.data_ptr())
    w = torch.zeros(1 << 16, dtype=torch.int64, device=DEV)
    assert lib.sdt_motion_dist_rows_f64(p(w), p(w), p(w), p(w), 1, 1, 129, p(w), None) == -1
    assert lib.sdt_motion_dist_rows_f64(p(w), p(w), p(w), p(w), 1, 0, 5, p(w), None) == -1
    assert lib.sdt_motion_dist_rows_f64(p(w), p(w), p(w), p(w), 1, 65537, 5, p(w), None) == -1
    assert lib.sdt_motion_dist_commit(p(w), p(w), 1, 17, 1, 5, p(w), 4, None) == -1
    assert lib.sdt_motion_dist_commit(p(w), p(w), 1, 1, 1, 129, p(w), 4, None) == -1
    assert lib.sdt_motion_dist_commit(p(w), p(w), 1, 1, 65537, 5, p(w), 4, None) == -1
    ptrs = (C.c_void_p * 1)(w.data_ptr())
    assert lib.sdt_motion_dist_epoch(ptrs, 65, 4, p(w), p(w), p(w), None) == -1
    assert lib.sdt_motion_dist_epoch(ptrs, 1, 0, p(w), p(w), p(w), None) == -1
    assert lib.sdt_motion_dist_epoch_work_words(65) == 2 * md.CHUNK_WORDS and lib.sdt_motion_dist_epoch_work_words(0) == 0
    torch.cuda.synchronize()
    assert not w.any()


# (f) the pipeline -----------------------------------------------------------------------------------------------------------------------------------
NEW_KEYS = ["hellinger_speed", "hellinger_speed_hands", "hellinger_speed_floor", "hellinger_accel", "hellinger_accel_hands", "hellinger_accel_floor",
            "hellinger_jerk", "hellinger_jerk_hands", "hellinger_jerk_floor", "accel_ratio", "accel_ratio_hands", "jerk_ratio", "jerk_ratio_hands",
            "motion_clips_nonfinite"]


def _set_key(cfg, on, multiple=1, tensorboard=False):
    cfg.defrost()
    cfg.TEST.MOTION_DIST, cfg.TEST.MULTIPLE, cfg.SYS.TENSORBOARD = bool(on), multiple, tensorboard
    cfg.freeze()


def test_validate_with_the_key_off_and_on(monkeypatch, tmp_path):
    from oracle import sdt_oracle as O
    from test_fgd_gpu import _validation_pipeline
    pipe, cfg = _validation_pipeline()
    losses, _ = pipe.forward_backward(O.make_batch(4, 16, step=0, seed=1))
    pipe.optimizer_updates(losses)
    _set_key(cfg, False, 2)
    torch.manual_seed(5)
    off = pipe.validate(pipe.test_dataloader, 1)
    assert {"L2_dist", "lip_sync_error_n", "FGD_mu", "FGD_mu_logvar"} <= set(off)
    assert pipe.motion_dist() is None and not set(off) & set(NEW_KEYS)  # no accumulator exists, no new key
    assert not any(k.startswith(("hellinger", "motion_", "accel_", "jerk_")) for k in off)
    _set_key(cfg, True, 2, tensorboard=True)
    pipe.base_path = str(tmp_path)
    try:
        pipe.setup_tb_writer()
        torch.manual_seed(5)
        on = pipe.validate(pipe.test_dataloader, 1)
        assert list(on) == list(off) + NEW_KEYS
        for k in off:
            assert torch.equal(torch.as_tensor(on[k]), torch.as_tensor(off[k])), k  # the parent's values keep their bits
        acc = pipe.motion_dist()
        table, hist = acc.table().cpu().numpy(), acc.histograms()
        want = md.epoch_values(epoch_held("validate()", acc, [table]))
        for k in NEW_KEYS:
            print("  %-24s %.17g" % (k, float(on[k])))
            assert float(on[k]) == want[k] and np.isfinite(float(on[k])), k
        assert on["motion_clips_nonfinite"] == 0 and 0 < on["hellinger_speed"] <= 1 and on["accel_ratio"] > 0
        with np.load(str(tmp_path / "results" / "epoch1-VAL-motion_metrics.npz")) as z:
            assert np.array_equal(z["table"], table) and np.array_equal(z["edges"], md.default_edges()) and np.array_equal(z["histograms"], hist)
            sizes = np.array(cm.part_sizes(part_table(121)))
            for o in range(3):  # m (T - 1 - o) |part| clips terms behind every histogram
                assert np.array_equal(z["histograms"][:, o].sum(axis=-1), np.broadcast_to(2 * (63 - o) * sizes * 8, (2, 4)))
        pipe.tb_writer.flush()
        histos = {}
        for path in sorted(tmp_path.glob("events.out.tfevents.*")):
            for ev in tb_events.read_events(str(path)):
                for v in ev["values"]:
                    if "histo" in v:
                        histos[v["tag"]] = (ev["step"], v["histo"])
        tags = ["val/motion/%s_%s_%s" % (o, s, p) for s in md.SOURCES for o in md.ORDERS for p in ("all", "body", "face", "hands")]
        assert sorted(histos) == sorted(tags) and len(tags) == 24
        for s, source in enumerate(md.SOURCES):
            for o, order in enumerate(md.ORDERS):
                for p, part in enumerate(("all", "body", "face", "hands")):
                    step, h = histos["val/motion/%s_%s_%s" % (order, source, part)]
                    assert step == 1 and [int(c) for c in h["bucket"]] == hist[s, o, p].tolist() and h["num"] == hist[s, o, p].sum()
                    assert list(h["bucket_limit"][:31]) == md.default_edges()[o].tolist() and h["bucket_limit"][31] == np.finfo(np.float64).max
        # a second epoch starts from a reset table: the same values
        torch.manual_seed(5)
        again = pipe.validate(pipe.test_dataloader, 1)
        assert all(float(again[k]) == float(on[k]) for k in on) and pipe.motion_dist() is acc
    finally:
        tb = getattr(pipe, "tb_writer", None)
        if tb is not None:
            tb.close()
            pipe.tb_writer = None
        pipe.base_path = None
        _set_key(cfg, False, 1)


# (g) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_command_line_prints_the_values_of_the_device_route(tmp_path, capsys):
    files, sets = [], []
    for i in range(2):
        pred, gt = poses(2 + 2 * i, 6, 121, seed=20 + i)
        files.append(str(tmp_path / ("epoch0-TEST-step%d.npz" % i)))
        np.savez(files[-1], poses_pred_batch=pred, poses_gt_batch=gt, mu_pred=np.zeros((2, 4)))
        sets.append((pred, gt))
    acc = md.MotionDistAccumulator(3, 121, None, DEV)
    acc.add(dev(sets[0][0]), dev(sets[0][1]), torch.tensor([0]), 2)
    acc.add(dev(sets[1][0]), dev(sets[1][1]), torch.tensor([1, 2]), 2)
    want = md.epoch_values(acc.result_words(), full=True)
    out = str(tmp_path / "hist.npz")
    assert md.main(files + ["--multiple", "2", "--worst", "2", "--out", out]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    fields = dict(ln.split(": ", 1) for ln in lines if ": " in ln and not ln.startswith("worst"))
    assert list(fields) == list(want)
    for k, v in want.items():
        assert float(fields[k]) == v, k
    worst = [ln for ln in lines if ln.startswith("worst")]
    h = md.clip_hellinger(acc.table().cpu().numpy())
    assert len(worst) == 2 and worst[0].startswith("worst: clip %d " % int(np.argmax(h))) and repr(float(h.max())) in worst[0]
    with np.load(out) as z:
        assert np.array_equal(z["table"], acc.table().cpu().numpy()) and np.array_equal(z["histograms"], acc.histograms())
