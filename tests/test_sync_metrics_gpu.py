"""The speech-gesture synchrony metrics on the GPU (csrc/sync_metrics.hip, speechdrivestemplates_amd/sync_metrics.py, TEST.SYNC_METRICS;
DESIGN.md section 24) against the numpy contract models.

Bars.  Onset and beat tick lists and every integer word are equal.  The envelopes and the align sums run the model's operations in the model's
order, so where this device's float64 square root is correctly rounded on the test's own arguments (the ``sqrt_is_exact`` pattern of
tests/test_clip_metrics_gpu.py) they are bit-identical; otherwise they are held to (n + 2) 2^-52 relative, n the number of terms (320 for an
envelope, the beats for an align sum).  The epoch stage has no square root: its vector equals ``epoch_model`` of the device's own table bit
for bit.  Every comparison prints how many values were bit-identical before it asserts.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from speechdrivestemplates_amd import clip_metrics as cm
from speechdrivestemplates_amd import sync_metrics as sm
from test_sync_metrics_host import (COPIES, SHAPES, ULP, audio_batch, click_train, gestures, nan_cases, part_table, refractory_audio, speech,
                                    stepped)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(B, T, K, L, m) for B, T, K, L in SHAPES for m in COPIES]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def sqrt_is_exact():
    rng = np.random.Generator(np.random.PCG64(11))
    x = np.concatenate([rng.uniform(0, 4, 100000), np.exp(rng.uniform(-30, 30, 100000)), [0.0, 1.0, 2.0, 4.0, 2.0 ** -1040]])
    same = np.array_equal(cm.device_sqrt(dev(x)).cpu().numpy(), np.sqrt(x))
    print("  device sqrt(float64) equals numpy's on %d values: %s" % (x.size, same))
    return same


def exact_on(args):
    """is the device's square root correctly rounded on these arguments (the squares under every root the kernels take)"""
    x = np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in args])
    x = x[np.isfinite(x)]
    return sqrt_is_exact() and (x.size == 0 or np.array_equal(cm.device_sqrt(dev(x)).cpu().numpy(), np.sqrt(x)))


def root_arguments(audio, *poses):
    out = [sm.onsets_model(a)['energy'] for a in audio]
    for x in poses:
        if x is not None and x.shape[1] > 1:
            vx, vy = x[:, 1:, 0] - x[:, :-1, 0], x[:, 1:, 1] - x[:, :-1, 1]
            out.append(vx * vx + vy * vy)
    return out


def held(name, got, want, exact):
    """clip records ``got`` (device) against ``want`` (model): integers equal; align sums bit-identical, or within (beats + 2) 2^-52"""
    assert np.array_equal(got[:, 8:], want[:, 8:]), "%s: integer columns differ" % name
    gf, wf = got[:, :8].copy().view(np.float64), want[:, :8].copy().view(np.float64)
    same = int((got[:, :8] == want[:, :8]).sum())
    print("  %-44s %d of %d align sums bit-identical (sqrt exact on these inputs: %s)" % (name, same, gf.size, exact))
    if exact:
        assert same == gf.size, "%s: %d of %d align sums differ in bits" % (name, gf.size - same, gf.size)
        return
    n = np.concatenate([want[:, sm.INT_PRED:sm.INT_PRED + 4], want[:, sm.INT_GT:sm.INT_GT + 4]], axis=1)
    assert (np.abs(gf - wf) <= (n + 2) * ULP * np.abs(wf)).all(), "%s: error %s" % (name, np.abs(gf - wf).max())


def accumulator(N, K, tol=30, sigma=0.1):
    return sm.SyncAccumulator(N, K, tol, sigma, DEV, parts=part_table(K))


def committed(pred, gt, audio, m, tol=30, sigma=0.1, index=None, num_clips=None):
    B = pred.shape[0] // m
    acc = accumulator(B if num_clips is None else num_clips, pred.shape[3], tol, sigma)
    acc.add(dev(pred), None if gt is None else dev(gt), dev(audio), torch.arange(B, dtype=torch.int64) if index is None else index, m)
    return acc


# (a) device against model -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%dx%d-m%d" % c)
def test_kernels_match_the_model(case):
    B, T, K, L, m = case
    pred, gt, audio, parts = gestures(m * B, T, K, 1), gestures(m * B, T, K, 2), audio_batch(B, L, T), part_table(K)
    exact = exact_on(root_arguments(audio, pred, gt))
    want = sm.sync_model(pred, gt, audio, parts, 30, 0.1, m)
    acc = committed(pred, gt, audio, m)
    held("B=%d T=%d K=%d L=%d m=%d" % case, acc.table().cpu().numpy(), want, exact)
    assert acc.state()[-1].cpu().tolist() == [0] * sm.COLS  # the header: no index error, nothing else written
    if m > 1:
        return
    # the detector's and the beat rule's own outputs
    ticks, env, strength, flag = sm.onsets(dev(audio), details=True)
    for b in range(B):
        om = sm.onsets_model(audio[b])
        assert np.array_equal(ticks[b], om['ticks']), b
        if exact:
            assert np.array_equal(env[b], om['env']) and np.array_equal(strength[b], om['strength'])
        else:
            assert np.all(np.abs(env[b] - om['env']) <= (320 + 2) * ULP * om['env'])
    assert not flag.any()
    got, speed = sm.beats(dev(pred), parts, details=True)
    bm = sm.beats_model(pred, parts)
    for r in range(B):
        for p in range(4):
            assert np.array_equal(got[r][p], sm.beat_ticks(bm['flags'][r, p])), (r, p)
    if exact:
        assert np.array_equal(speed, bm['speed'])
    rows = sm.row_records(dev(pred), dev(audio), 30, 0.1, parts).cpu().numpy()
    assert np.array_equal(rows[:, 4:], sm.row_records_model(pred, [sm.onsets_model(a) for a in audio], parts, 30, 0.1)[:, 4:])


# (b) constructed cases ----------------------------------------------------------------------------------------------------------------------------
def device_onsets(x, **kw):
    return sm.onsets(dev(np.asarray(x, dtype=np.float32)), **kw)


def test_constructed_onsets_on_the_device():
    x, clicks = click_train()
    assert device_onsets(x)[0].tolist() == [3 * (c // 160 - 1) + 3 for c in clicks]
    assert device_onsets(np.zeros(8000))[0].size == 0
    assert device_onsets(refractory_audio(7))[0].tolist() == [63] and device_onsets(refractory_audio(8))[0].tolist() == [63, 87]
    ticks, env, _, flag = device_onsets(np.ones(100), details=True)
    assert ticks[0].size == 0 and env.shape == (1, 0) and not flag.any()  # L = 100: no frame
    ticks, env, _, _ = device_onsets(np.ones(479), details=True)
    assert ticks[0].size == 0 and env.shape == (1, 2)  # L = 479: two frames, no interior one
    if sqrt_is_exact():
        assert env[0].tolist() == [np.sqrt(320.0), np.sqrt(319.0)]  # the last frame reads one zero past the end


def device_beats(speeds):
    return sm.beats(dev(stepped(speeds)[None]), [0])[0][0].tolist()


def test_constructed_beats_on_the_device():
    assert device_beats([1, 1, 4, 4, 4, 1, 1, 1]) == [50]  # a plateau takes its first frame
    assert device_beats([1, 5]) == [] and device_beats([1, 5, 1]) == [30] and device_beats([5, 1, 1]) == []  # T = 3, T = 4
    assert sm.beats(torch.zeros((1, 1, 2, 1), dtype=torch.float64, device=DEV), [0])[0][0].size == 0  # T = 1
    # every beat lands in d = 150 when the clip has no onset
    x = gestures(1, 64, 5)
    rec = committed(x, None, np.zeros((1, 8000), dtype=np.float32), 1).table().cpu().numpy()
    assert np.array_equal(rec[:, 8:], sm.sync_model(x, None, np.zeros((1, 8000), dtype=np.float32), part_table(5), 30, 0.1)[:, 8:])
    n = rec[0, sm.INT_PRED:sm.INT_PRED + 4]
    assert (n > 0).all() and np.array_equal(rec[0, sm.INT_PRED + 8:sm.INT_PRED + 12], 150 * n) and not rec[0, sm.INT_PRED + 4:sm.INT_PRED + 8].any()


def test_tolerance_boundary_and_an_equidistant_beat_on_the_device():
    # one beat at t = 4 (tick 90); clicks at samples 3200 and 6400 give onsets at frames 19 and 39 (ticks 60 and 120): both 30 ticks away
    x = np.repeat(stepped([1, 1, 1, 1, 5, 1, 1, 1]), 2, axis=2)[None]  # K = 2, both keypoints in part 0 (body)
    audio = click_train(8000, (3200, 6400))[0][None]
    assert sm.onsets(dev(audio))[0].tolist() == [60, 120] and sm.beats(dev(x), [0, 0])[0][0].tolist() == [90]
    G = sm.gauss_table(0.1)
    for tol, hits, covered in ((30, 1, 2), (29, 0, 0), (150, 1, 2)):
        row = sm.row_records(dev(x), dev(audio), tol, 0.1, [0, 0]).cpu().numpy()[0]
        for p, has in enumerate((True, True, False, False)):  # parts all and body hold the keypoints
            assert [int(row[4 + 4 * g + p]) for g in range(4)] == ([1, hits, 30, covered] if has else [0, 0, 0, 0]), (tol, p)
            assert row[p:p + 1].view(np.float64)[0] == (G[30] if has else 0.0)
        assert row[sm.ROW_ONSETS] == 2 and row[sm.ROW_NONFINITE] == 0 and row[sm.ROW_FRAMES] == 9
    one = click_train(8000, (6400,))[0][None]  # the onset at tick 120 alone: tol 30 hits, tol 29 misses
    assert sm.row_records(dev(x), dev(one), 30, 0.1, [0, 0]).cpu().numpy()[0, 8] == 1
    assert sm.row_records(dev(x), dev(one), 29, 0.1, [0, 0]).cpu().numpy()[0, 8] == 0


def test_nan_flags_its_clip_only_on_the_device():
    pred, gt, audio, parts = nan_cases()
    clean = committed(pred, gt, audio, 1).table().cpu().numpy()
    bad = pred.copy()
    bad[1, 4, 0, 2] = np.nan
    acc = committed(bad, gt, audio, 1)
    rec = acc.table().cpu().numpy()
    assert rec[:, sm.NONFINITE].tolist() == [0, 1, 0] and np.array_equal(rec[[0, 2]], clean[[0, 2]])
    assert np.array_equal(rec[:, 8:], sm.sync_model(bad, gt, audio, parts, 30, 0.1)[:, 8:])
    res = acc.result()
    assert res['sync_clips_nonfinite'] == 1 and res['sync_clips_seen'] == 3 and all(np.isfinite(v) for v in res.values())
    assert np.array_equal(acc.result_words(), sm.epoch_model([rec]))
    for value in (np.nan, np.inf):
        noisy = audio.copy()
        noisy[2, 1234] = value
        rec = committed(pred, gt, noisy, 1).table().cpu().numpy()
        assert rec[:, sm.NONFINITE].tolist() == [0, 0, 1] and np.array_equal(rec[:2], clean[:2])
        assert np.array_equal(rec[:, 8:], sm.sync_model(pred, gt, noisy, parts, 30, 0.1)[:, 8:])
    p2, g2 = gestures(4, 17, 5, 5), gestures(4, 17, 5, 6)
    p2[3, 2, 1, 1] = np.nan  # row 3 = copy 1 of clip 1 (B = 2)
    assert committed(p2, g2, audio[:2], 2).table()[:, sm.NONFINITE].cpu().tolist() == [0, 1]


# (c) a long row ---------------------------------------------------------------------------------------------------------------------------------
def test_one_long_row():
    T, L, K = 4500, 4800000, 121
    x, audio, parts = gestures(1, T, K, 9), speech(L, 9)[None], part_table(K)
    want = sm.row_records_model(x, [sm.onsets_model(audio[0])], parts, 30, 0.1)
    got = sm.recording_report(dev(x[0]), dev(audio[0]), 30, 0.1, parts).cpu().numpy()[None]
    print("  long row: %d onsets, beats %s, hits %s" % (want[0, sm.ROW_ONSETS], want[0, 4:8].tolist(), want[0, 8:12].tolist()))
    assert want[0, sm.ROW_ONSETS] > 1000 and want[0, 4] > 500 and want[0, 8] > 0
    assert np.array_equal(got[:, 4:], want[:, 4:])
    if exact_on(root_arguments(audio, x)):
        assert np.array_equal(got, want)
    else:
        gf, wf = got[:, :4].copy().view(np.float64), want[:, :4].copy().view(np.float64)
        assert (np.abs(gf - wf) <= (want[:, 4:8] + 2) * ULP * wf).all()
    assert np.array_equal(sm.onsets(dev(audio))[0], sm.onsets_model(audio[0])['ticks'])


# (d) commit and epoch ---------------------------------------------------------------------------------------------------------------------------
def test_commit_writes_the_addressed_rows_and_counts_bad_indices():
    N, T, K, L, SENTINEL = 10, 17, 5, 6401, 0x5A5AA5A55A5AA5A5
    pred, gt, audio, parts = gestures(5, T, K, 7), gestures(5, T, K, 8), audio_batch(5, L, 7), part_table(K)
    acc = accumulator(N, K)
    acc.state().fill_(SENTINEL)
    acc.state()[N].zero_()
    acc.add(dev(pred), dev(gt), dev(audio), torch.tensor([7, 2, -1, N, 4], dtype=torch.int64), 1)
    want = sm.sync_model(pred, gt, audio, parts, 30, 0.1)
    state = acc.state().cpu().numpy()
    exact = exact_on(root_arguments(audio, pred, gt))
    held("commit", state[[7, 2, 4]], want[[0, 1, 4]], exact)
    assert (state[[r for r in range(N) if r not in (7, 2, 4)]] == SENTINEL).all()
    assert state[N, 0] == 2 and not state[N, 1:].any()  # the two bad indices are counted, and wrote nothing
    assert acc.result()['sync_index_errors'] == 2
    # a multiplied batch hands its audio and its index in multiplied: the first B are read
    acc.add(dev(pred[:4]), dev(gt[:4]), dev(np.concatenate([audio[:2], audio[:2]])), torch.tensor([3, 5, 3, 5], dtype=torch.int64), 2)
    again = acc.state().cpu().numpy()
    held("commit of two copies", again[[3, 5]], sm.sync_model(pred[:4], gt[:4], audio[:2], parts, 30, 0.1, 2), exact)
    keep = [r for r in range(N + 1) if r not in (3, 5)]
    assert np.array_equal(again[keep], state[keep])
    acc.reset()
    assert not acc.state().any()


@pytest.mark.parametrize("N", [1, 63, 64, 65])
def test_epoch_is_the_same_however_the_records_arrive(N):
    T, K, L, m = 17, 5, 3200, 2
    rng = np.random.Generator(np.random.PCG64(N))
    seen = np.array([0]) if N == 1 else np.sort(rng.permutation(N)[:max(1, 3 * N // 4)])  # holes: a quarter of the clips arrive nowhere
    n = len(seen)
    pred, gt, audio = gestures(m * n, T, K, N), gestures(m * n, T, K, N + 1), audio_batch(n, L, N)
    p5, g5 = pred.reshape(m, n, T, 2, K), gt.reshape(m, n, T, 2, K)

    def rows(a, sel):
        return dev(a[:, sel].reshape(m * len(sel), T, 2, K))

    def feed(acc, sel, spoil=False):
        acc.add(rows(g5 if spoil else p5, sel), rows(g5, sel), dev(audio[sel]), torch.from_numpy(seen[sel]), m)

    one = accumulator(N, K)
    feed(one, rng.permutation(n))  # one add of all rows, shuffled
    words = one.result_words()
    assert np.array_equal(words, sm.epoch_model([one.table().cpu().numpy()]))
    assert words[sm.OUT_SEEN] == n and words[sm.OUT_NONFINITE] == 0
    vals = one.result()
    assert all(np.isfinite(v) for v in vals.values()) and vals['sync_clips_seen'] == n and vals['beats_per_s'] > 0
    ragged = accumulator(N, K)
    for sel in np.array_split(np.arange(n), min(7, n)):  # up to 7 adds of ragged sizes
        feed(ragged, sel)
    assert torch.equal(ragged.state(), one.state()) and np.array_equal(ragged.result_words(), words)
    # three per-rank tables with overlapping clips: the higher rank of an overlap holds another record, which must not be read
    ranks = [accumulator(N, K) for _ in range(3)]
    for r in range(3):
        own = np.arange(n)[np.arange(n) % 3 == r]
        if len(own):
            feed(ranks[r], own)
        if r > 0:
            other = np.arange(n)[(np.arange(n) % 3 == r - 1) & (np.arange(n) % 2 == 0)]
            if len(other):
                feed(ranks[r], other, spoil=True)
    gathered = torch.stack([a.state() for a in ranks])
    assert np.array_equal(ranks[2].result_words(gathered), words) and np.array_equal(ranks[0].result_words(ranks), words)
    if n >= 6:
        assert not np.array_equal(ranks[0].result_words(ranks[::-1]), words)  # (rank order matters where records differ)
    one.reset()
    assert one.result()['sync_clips_seen'] == 0


# (e) size checks --------------------------------------------------------------------------------------------------------------------------------
def test_size_checks():
    with pytest.raises(ValueError, match="K = 129"):
        sm.SyncAccumulator(4, 129, 30, 0.1, DEV, parts=[0] * 129)
    for tol in (0, 151):
        with pytest.raises(ValueError, match="tolerance"):
            sm.SyncAccumulator(4, 5, tol, 0.1, DEV, parts=part_table(5))
    acc = accumulator(4, 5)
    x = torch.zeros((17, 4, 2, 5), dtype=torch.float64, device=DEV)
    a = torch.zeros((17, 800), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="17 copies"):
        acc.add(x, x, a[:1], torch.zeros(1, dtype=torch.int64), 17)
    with pytest.raises(ValueError):
        acc.add(x, x, a, torch.zeros(17, dtype=torch.int64), 2)  # 17 rows are not 2 copies
    with pytest.raises(ValueError, match="audio"):
        acc.add(x, x, a[:3], torch.zeros(17, dtype=torch.int64), 1)
    with pytest.raises(TypeError):
        acc.add(x.float(), x.float(), a, torch.zeros(17, dtype=torch.int64), 1)
    with pytest.raises(TypeError):
        acc.add(x, x, a.double(), torch.zeros(17, dtype=torch.int64), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        acc.add(x.cpu(), x.cpu(), a, torch.zeros(17, dtype=torch.int64), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sm.SyncAccumulator(4, 5, 30, 0.1, "cpu", parts=part_table(5))
    assert not acc.state().any()
    # the library checks the same sizes before any launch
    import ctypes as C
    from speechdrivestemplates_amd import _lib
    lib, p = _lib.load(), lambda t: C.c_void_p(t.data_ptr())
    w = torch.zeros(1 << 16, dtype=torch.int64, device=DEV)
    rows = lambda T, K, tol: lib.sdt_sync_rows_f64(p(w), p(w), 1, T, K, 1, p(w), 8, p(w), p(w), tol, 1.0, p(w), p(w), None)  # noqa: E731
    assert rows(4, 129, 30) == -1 and rows(4, 0, 30) == -1 and rows(4, 5, 0) == -1 and rows(4, 5, 151) == -1 and rows(0, 5, 30) == -1
    assert lib.sdt_sync_onsets_f64(p(w), 1, -1, 1.5, 0.1, p(w), p(w), 8, p(w), None) == -1
    assert lib.sdt_sync_onsets_f64(p(w), 1, 16000, 1.5, 0.1, p(w), p(w), 1, p(w), None) == -1  # a tick list that is too short
    assert lib.sdt_sync_commit(p(w), p(w), p(w), 1, 17, 4, 800, p(w), 4, None) == -1
    assert lib.sdt_sync_commit(p(w), p(w), p(w), 1, 1, 4, -1, p(w), 4, None) == -1
    assert lib.sdt_sync_workspace_bytes(1, -1, 1, 4) == -1 and lib.sdt_sync_onset_capacity(-1) == -1
    assert lib.sdt_sync_workspace_bytes(2, 800, 3, 5) == max(2 * 5 * 2 * 8, 3 * 4 * 4 * 8 + 64) and lib.sdt_sync_onset_capacity(800) == 1
    torch.cuda.synchronize()
    assert not w.any()


# (f) the pipeline -------------------------------------------------------------------------------------------------------------------------------
NEW_KEYS = [n + h for n in sm.VALUE_PAIRS for h in ("", "_hands")] + ["onsets_per_s", "sync_clips_nonfinite"]


def _set_key(cfg, on, multiple=1):
    cfg.defrost()
    cfg.TEST.SYNC_METRICS, cfg.TEST.MULTIPLE = bool(on), multiple
    cfg.freeze()


def test_validate_with_the_key_off_and_on(monkeypatch, tmp_path):
    """The new values against the model on the poses and audio test_step handed over: the table to the bar of ``held``, and the epoch values
    bit for bit against ``epoch_model`` of the device's own table (the epoch stage has no square root)."""
    from oracle import sdt_oracle as O
    from test_fgd_gpu import _validation_pipeline
    pipe, cfg = _validation_pipeline()
    losses, _ = pipe.forward_backward(O.make_batch(4, 16, step=0, seed=1))
    pipe.optimizer_updates(losses)
    _set_key(cfg, False, 2)
    torch.manual_seed(5)
    off = pipe.validate(pipe.test_dataloader, 1)
    assert {"L2_dist", "lip_sync_error_n", "FGD_mu", "FGD_mu_logvar"} <= set(off)
    assert pipe.sync_metrics() is None and not set(off) & set(NEW_KEYS)  # no accumulator exists, no new key
    calls = []
    orig_add = sm.SyncAccumulator.add
    monkeypatch.setattr(sm.SyncAccumulator, "add",
                        lambda self, p, g, a, idx, m=1: (calls.append((p.cpu().numpy(), g.cpu().numpy(), a.cpu().numpy(), idx.cpu().numpy(), m)),
                                                         orig_add(self, p, g, a, idx, m))[1])
    _set_key(cfg, True, 2)
    pipe.base_path = str(tmp_path)
    try:
        torch.manual_seed(5)
        on = pipe.validate(pipe.test_dataloader, 1)
        assert list(on) == list(off) + NEW_KEYS
        for k in off:
            assert torch.equal(torch.as_tensor(on[k]), torch.as_tensor(off[k])), k  # the parent's values keep their bits
        assert all(np.isfinite(float(on[k])) for k in NEW_KEYS) and on["sync_clips_nonfinite"] == 0
        assert len(calls) == 2 and all(c[0].shape == (8, 64, 2, 121) and c[4] == 2 for c in calls)
        parts = part_table(121)
        table = np.zeros((8, sm.COLS), dtype=np.int64)
        exact = True
        for p, g, a, idx, m in calls:
            assert idx.shape == (8,) and np.array_equal(idx[:4], idx[4:]) and a.shape[0] == 8 and np.array_equal(a[:4], a[4:])
            table[idx[:4]] = sm.sync_model(p, g, a[:4], parts, 30, 0.1, m)
            exact = exact and exact_on(root_arguments(a[:4], p, g))
        acc = pipe.sync_metrics()
        got_table = acc.table().cpu().numpy()
        held("validate(): the table against the model", got_table, table, exact)
        want = sm.epoch_values(sm.epoch_model([got_table]))
        for k in NEW_KEYS:
            print("  %-26s device %.17g model %.17g" % (k, float(on[k]), want[k]))
            assert float(on[k]) == want[k], k
        with np.load(str(tmp_path / "results" / "epoch1-VAL-sync_metrics.npz")) as z:
            assert np.array_equal(z["table"], got_table) and tuple(z["columns"]) == sm.COLUMN_NAMES and int(z["tolerance_ticks"]) == 30
        torch.manual_seed(5)
        again = pipe.validate(pipe.test_dataloader, 1)  # a second epoch starts from a reset table: the same values
        assert all(float(again[k]) == float(on[k]) for k in on) and pipe.sync_metrics() is acc
    finally:
        pipe.base_path = None
        _set_key(cfg, False, 1)


def test_long_demo_with_the_key(tmp_path):
    from test_long_demo_gpu import _batch, _pipeline
    pipe = _pipeline(None, "DEMO.LONG_FORM", True, "DEMO.LONG_BATCH", 2, "DEMO.SMOOTH", [2, 2], "TEST.SYNC_METRICS", True, "TEST.SAVE_VIDEO", False)
    batch = _batch(tmp_path, 150)
    res = pipe.demo_step(batch, 1)
    pipe.close()
    rep = res["sync_report"].numpy()
    assert rep.shape == (2, sm.ROW_COLS) and tuple(res["long_report"].shape) == (40,)
    audio, parts = batch["audio"].numpy(), part_table(121)
    om = [sm.onsets_model(audio[0])]
    for i, key in enumerate(("poses_pred_batch", "poses_stitched")):  # the final (smoothed) poses, then the stitched ones
        x = res[key].cpu().numpy()
        want = sm.row_records_model(x, om, parts, 30, 0.1)
        assert np.array_equal(rep[i:i + 1, 4:], want[:, 4:]), key
        if exact_on(root_arguments(audio, x)):
            assert np.array_equal(rep[i:i + 1], want), key
    assert rep[0, sm.ROW_FRAMES] == 150 and rep[0, sm.ROW_ONSETS] == len(om[0]['ticks'])
    assert "150 frames" in sm.describe_row(rep[0], audio.shape[1] // 160)


# (g) the command line ---------------------------------------------------------------------------------------------------------------------------
def test_command_line_prints_the_values_of_the_device_route(tmp_path):
    pred, gt, audio, _ = (gestures(3, 17, 121, 3), gestures(3, 17, 121, 4), audio_batch(3, 6401, 3), None)
    poses_file, audio_file, out = str(tmp_path / "epoch0-TEST-step1.npz"), str(tmp_path / "audio.npy"), str(tmp_path / "table.npz")
    np.savez(poses_file, poses_pred_batch=pred, poses_gt_batch=gt)
    np.save(audio_file, audio)
    acc = committed(pred, gt, audio, 1, tol=15, sigma=0.2)
    want = acc.result()
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "speechdrivestemplates_amd.sync_metrics", poses_file, audio_file, "--tolerance", "0.05",
                        "--sigma", "0.2", "--out", out], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    fields = dict(ln.split(": ", 1) for ln in r.stdout.strip().splitlines() if ": " in ln)
    assert list(fields) == list(want)
    for k, v in want.items():
        assert float(fields[k]) == v, k
    with np.load(out) as z:
        assert np.array_equal(z["table"], acc.table().cpu().numpy()) and int(z["tolerance_ticks"]) == 15 and float(z["sigma"]) == 0.2
