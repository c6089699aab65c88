"""The speech-gesture synchrony metrics (speechdrivestemplates_amd/sync_metrics.py) without a GPU: the numpy contract
models against plain formulations, constructed cases with known answers, flags and merging, the config check and the command line.

Bars.  Onset and beat lists and every count are integers and must be equal (the generated inputs have no near-ties).  A sum of n non-negative
float64 terms computed in any order differs from any other order by at most (n - 1) 2^-52 relative, and the two formulations of one term
differ by at most 2 ulp: together (n + 2) 2^-52 relative.
"""
import numpy as np
import pytest

from speechdrivestemplates_amd import sync_metrics as sm
from speechdrivestemplates_amd.config import check_sync_metrics, get_cfg_defaults
from speechdrivestemplates_amd.core.datasets.gesture_dataset import PoseTransforms

ULP = 2.0 ** -52
SHAPES = [(1, 4, 1, 480), (1, 5, 121, 800), (2, 64, 121, 68266), (3, 17, 128, 6401), (1, 3, 7, 100)]  # (R, T, K, L)
COPIES = (1, 2, 16)


def part_table(K):
    return PoseTransforms.part_table() if K == 121 else [k % 3 for k in range(K)]


def speech(L, seed=0, period=2900):
    """a noise floor with louder bursts every ``period`` samples or so: onsets a detector can find, and no two equal values"""
    rng = np.random.Generator(np.random.PCG64(77 + seed))
    x = rng.standard_normal(L) * 0.01
    start = int(rng.integers(200, 900))
    while start < L:
        n = int(rng.integers(300, 900))
        x[start:start + n] += rng.standard_normal(len(x[start:start + n])) * rng.uniform(0.2, 0.8)
        start += int(period * rng.uniform(0.6, 1.4))
    return x.astype(np.float32)


def audio_batch(B, L, seed=0):
    return np.stack([speech(L, 10 * seed + b) for b in range(B)])


def gestures(R, T, K, seed=0):
    """a slow drift with strokes of a few frames: speeds with clear peaks"""
    rng = np.random.Generator(np.random.PCG64(1000 * seed + 7 * R + 3 * T + K))
    v = rng.standard_normal((R, T, 2, K)) * 0.5
    for r in range(R):
        t = int(rng.integers(1, 6))
        while t < T:
            v[r, t:t + 2] += rng.standard_normal((1, 2, K)) * rng.uniform(4.0, 12.0)
            t += int(rng.integers(4, 11))
    return 200.0 + np.cumsum(v, axis=1)


def plain_onsets(x):
    """the onset rule with np.sqrt(np.sum(...)) and boolean masks -> (e, accepted frames)"""
    x = np.asarray(x, dtype=np.float64)
    L = len(x)
    Nf = L // 160
    pad = np.concatenate([x, np.zeros(320)])
    e = np.array([np.sqrt(np.sum(pad[160 * n:160 * n + 320] ** 2)) for n in range(Nf)])
    o = np.concatenate([[0.0], np.maximum(np.diff(e), 0.0)]) if Nf else np.zeros(0)
    mean = np.array([np.mean(o[max(n - 15, 0):n + 16]) for n in range(Nf)])
    n = np.arange(1, max(Nf - 1, 1))
    ok = (o[n] > o[n - 1]) & (o[n] >= o[n + 1]) & (o[n] > 1.5 * mean[n]) & (o[n] > e.max() / 64) if Nf > 2 else np.zeros(0, dtype=bool)
    frames, last = [], None
    for c in n[ok] if Nf > 2 else []:
        if last is None or c - last >= 8:
            frames.append(int(c))
            last = c
    return e, o, np.array(frames, dtype=np.int64)


def plain_beats(x, parts):
    """(T, 2, K) -> (speeds (T - 1, 4), per part the beat frames) with np.linalg.norm and boolean masks"""
    parts = np.asarray(parts)
    sp = np.linalg.norm(x[1:] - x[:-1], axis=1)  # (T - 1, K)
    masks = [np.ones(len(parts), dtype=bool)] + [parts == i for i in range(3)]
    s = np.stack([sp[:, mk].sum(axis=1) for mk in masks], axis=1)
    out = []
    for p in range(4):
        c = s[:, p]
        t = np.arange(1, len(c) - 1)
        out.append(t[(c[t] > c[t - 1]) & (c[t] >= c[t + 1]) & (c[t] > c.mean())] if len(c) >= 3 else np.zeros(0, dtype=np.int64))
    return s, out


def plain_match(beats, onsets, tol, sigma):
    d = np.array([min([abs(b - a) for a in onsets] + [150]) for b in beats], dtype=np.int64)
    covered = sum(1 for a in onsets if any(abs(b - a) <= tol for b in beats))
    return len(beats), int((d <= tol).sum()), int(d.sum()), covered, float(np.sum(np.exp(-(d / 300.0) ** 2 / (2 * sigma * sigma))))


# ---- models against plain formulations -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [100, 479, 480, 800, 6401, 68266])
def test_onsets_model_against_plain_formulas(L):
    x = speech(L, seed=L)
    om = sm.onsets_model(x)
    e, o, frames = plain_onsets(x)
    assert om['env'].shape == e.shape == (L // 160,)
    assert np.all(np.abs(om['env'] - e) <= (320 + 2) * ULP * e)
    assert np.array_equal(om['frames'], frames) and np.array_equal(om['ticks'], 3 * frames + 3)
    assert not om['nonfinite']
    if L >= 6401:
        assert len(frames) >= 2 and np.all(np.diff(frames) >= 8)
        try:  # where the rule coincides (no plateaus): the candidates are peaks of the onset strength
            from scipy.signal import find_peaks
        except ImportError:
            return
        assert set(om['candidates']) <= set(find_peaks(om['strength'])[0])


@pytest.mark.parametrize("shape", [(1, 4, 1), (1, 5, 121), (2, 64, 121), (3, 17, 128), (1, 3, 7)], ids=lambda s: "x".join(map(str, s)))
def test_beats_model_against_plain_formulas(shape):
    R, T, K = shape
    x, parts = gestures(R, T, K), part_table(K)
    bm = sm.beats_model(x, parts)
    sizes = [K] + [int((np.asarray(parts) == i).sum()) for i in range(3)]
    for r in range(R):
        s, frames = plain_beats(x[r], parts)
        for p in range(4):
            assert np.all(np.abs(bm['speed'][r, :, p] - s[:, p]) <= (sizes[p] + 2) * ULP * s[:, p])
            assert np.array_equal(np.flatnonzero(bm['flags'][r, p]), frames[p]), (r, p)
            assert np.array_equal(sm.beat_ticks(bm['flags'][r, p]), 20 * frames[p] + 10)
    assert not bm['nonfinite'].any()
    if T == 64:
        assert bm['flags'][:, 0].sum() >= 4
        try:
            from scipy.signal import find_peaks
        except ImportError:
            return
        assert set(np.flatnonzero(bm['flags'][0, 0])) <= set(find_peaks(bm['speed'][0, :, 0])[0])


@pytest.mark.parametrize("tol,sigma", [(30, 0.1), (1, 0.05), (150, 0.3)])
def test_match_model_against_plain_formulas(tol, sigma):
    rng = np.random.Generator(np.random.PCG64(tol))
    beats = 20 * np.sort(rng.permutation(60)[:25]) + 10
    onsets = np.sort(3 * rng.permutation(400)[:12] + 3)
    for b, a in ((beats, onsets), (beats, onsets[:0]), (beats[:0], onsets), (beats[:1], onsets[:1])):
        n, hits, dsum, covered, align = sm.match_model(b, a, tol, sigma)
        want = plain_match(b, a, tol, sigma)
        assert (n, hits, dsum, covered) == want[:4]
        assert abs(align - want[4]) <= (n + 2) * ULP * want[4]


@pytest.mark.parametrize("m", COPIES)
def test_sync_model_sums_the_copies_in_order(m):
    B, T, K, L = 2, 17, 5, 6401
    pred, gt, audio, parts = gestures(m * B, T, K, 1), gestures(m * B, T, K, 2), audio_batch(B, L), part_table(K)
    rec = sm.sync_model(pred, gt, audio, parts, 30, 0.1, m)
    assert rec.shape == (B, sm.COLS) and rec[:, sm.SEEN].tolist() == [1] * B and rec[:, sm.COPIES].tolist() == [m] * B
    assert rec[:, sm.FRAMES].tolist() == [T] * B and rec[:, sm.HOPS].tolist() == [L // 160] * B and not rec[:, 46:].any()
    for b in range(B):
        onsets = sm.onsets_model(audio[b])['ticks']
        assert rec[b, sm.ONSETS] == m * len(onsets)
        for w, x in ((0, pred), (1, gt)):
            for p in range(4):
                rows = [plain_match(20 * plain_beats(x[j * B + b], parts)[1][p] + 10, onsets, 30, 0.1) for j in range(m)]
                got = [int(rec[b, (sm.INT_PRED, sm.INT_GT)[w] + 4 * g + p]) for g in range(4)]
                assert got == [sum(r[g] for r in rows) for g in range(4)]
                align = rec[b, 4 * w + p:4 * w + p + 1].view(np.float64)[0]
                want = sum(r[4] for r in rows)
                assert abs(align - want) <= (got[0] + 2) * ULP * want
    one = sm.sync_model(pred, None, audio, parts, 30, 0.1, m)
    assert np.array_equal(one[:, sm.INT_PRED:sm.INT_GT], rec[:, sm.INT_PRED:sm.INT_GT]) and not one[:, sm.INT_GT:sm.ONSETS].any()


# ---- constructed cases ---------------------------------------------------------------------------------------------------------------------------
def click_train(L=16000, clicks=(2000, 6000, 10000, 14000)):
    x = np.zeros(L, dtype=np.float32)
    for c in clicks:
        x[c] = 1.0
    return x, clicks


def test_a_click_train_gives_onsets_at_the_predicted_ticks():
    x, clicks = click_train()
    om = sm.onsets_model(x)
    # a click at sample c first enters frame n = c // 160 - 1 (samples [160 n, 160 n + 320)): the envelope rises there
    assert om['frames'].tolist() == [c // 160 - 1 for c in clicks]
    assert om['ticks'].tolist() == [3 * (c // 160 - 1) + 3 for c in clicks]
    assert om['env'][clicks[0] // 160] == 1.0 and om['env'][clicks[0] // 160 + 1] == 0.0


def test_silence_has_no_onsets_and_every_beat_lands_at_the_cap():
    om = sm.onsets_model(np.zeros(8000, dtype=np.float32))
    assert om['ticks'].size == 0 and not om['nonfinite']
    x, parts = gestures(1, 64, 5), part_table(5)
    rec = sm.sync_model(x, None, np.zeros((1, 8000), dtype=np.float32), parts, 30, 0.1)
    G = sm.gauss_table(0.1)
    for p in range(4):
        n = int(rec[0, sm.INT_PRED + p])
        assert n > 0 and rec[0, sm.INT_PRED + 4 + p] == 0 and rec[0, sm.INT_PRED + 8 + p] == 150 * n and rec[0, sm.INT_PRED + 12 + p] == 0
        assert abs(rec[0, p:p + 1].view(np.float64)[0] - n * G[150]) <= (n + 2) * ULP * n * G[150]
    assert rec[0, sm.ONSETS] == 0


def stepped(speeds, K=1):
    """(T, 2, K) poses whose summed speed between frames t and t + 1 is speeds[t] * K exactly (small integers)"""
    x = np.zeros((len(speeds) + 1, 2, K))
    x[1:, 0] = np.cumsum(np.asarray(speeds, dtype=np.float64))[:, None]
    return x


def test_a_speed_plateau_takes_its_first_frame():
    flags = sm.beats_model(stepped([1, 1, 4, 4, 4, 1, 1, 1])[None], [0])['flags'][0, 0]
    assert np.flatnonzero(flags).tolist() == [2]
    assert sm.beat_ticks(flags).tolist() == [50]


def test_short_rows():
    assert not sm.beats_model(stepped([1, 5])[None], [0])['flags'].any()  # T = 3: no interior speed
    flags = sm.beats_model(stepped([1, 5, 1])[None], [0])['flags'][0, 0]  # T = 4: t = 1 is the one candidate
    assert np.flatnonzero(flags).tolist() == [1]
    assert not sm.beats_model(stepped([5, 1, 1])[None], [0])['flags'].any()
    assert not sm.beats_model(np.zeros((1, 1, 2, 1)), [0])['flags'].any() and sm.speeds_model(np.zeros((1, 1, 2, 1)), [0]).shape == (1, 0, 4)


def refractory_audio(gap):
    """two bursts whose envelopes rise ``gap`` frames apart, the second louder"""
    x = np.zeros(160 * 80, dtype=np.float32)
    x[160 * 21] = 1.0
    x[160 * (21 + gap)] = 2.0
    return x


def test_refractory_gap_of_seven_drops_one_and_eight_keeps_both():
    seven, eight = sm.onsets_model(refractory_audio(7)), sm.onsets_model(refractory_audio(8))
    assert seven['candidates'].tolist() == [20, 27] and seven['frames'].tolist() == [20]
    assert eight['candidates'].tolist() == [20, 28] and eight['frames'].tolist() == [20, 28]


def test_short_audio():
    assert sm.onsets_model(np.ones(100, dtype=np.float32))['env'].size == 0
    om = sm.onsets_model(speech(479))
    assert om['env'].size == 2 and om['ticks'].size == 0  # two frames: no interior frame
    e = sm.envelope_model(np.ones(479, dtype=np.float32))
    assert e.tolist() == [np.sqrt(320.0), np.sqrt(319.0)]  # the last frame reads one zero past the end


def test_tolerance_boundary_and_equidistant_beats():
    G = sm.gauss_table(0.1)
    assert sm.match_model([110], [110 + 30], 30, G)[:4] == (1, 1, 30, 1)
    assert sm.match_model([110], [110 + 31], 30, G)[:4] == (1, 0, 31, 0)
    assert sm.match_model([110], [110 - 30], 30, G)[:4] == (1, 1, 30, 1)
    n, hits, dsum, covered, align = sm.match_model([110], [90, 130], 30, G)  # equidistant: one beat, both onsets covered
    assert (n, hits, dsum, covered) == (1, 1, 20, 2) and align == G[20]
    assert sm.match_model([110, 130], [120], 5, G)[:4] == (2, 0, 20, 0)
    assert sm.match_model([10], [900], 30, G)[:4] == (1, 0, 150, 0) and sm.match_model([10], [900], 30, G)[4] == G[150]
    assert G[0] == 1.0 and G.shape == (151,) and np.all(np.diff(G) < 0)
    with pytest.raises(ValueError):
        sm.match_model([10], [20], 0, G)
    with pytest.raises(ValueError):
        sm.match_model([10], [20], 151, G)
    with pytest.raises(ValueError):
        sm.gauss_table(0.0)


# ---- flags and merging ---------------------------------------------------------------------------------------------------------------------------
def nan_cases():
    B, T, K, L = 3, 17, 5, 6401
    pred, gt, audio = gestures(B, T, K, 3), gestures(B, T, K, 4), audio_batch(B, L, 3)
    return pred, gt, audio, part_table(K)


def test_nan_flags_its_clip_only():
    pred, gt, audio, parts = nan_cases()
    clean = sm.sync_model(pred, gt, audio, parts, 30, 0.1)
    assert not clean[:, sm.NONFINITE].any()
    bad = pred.copy()
    bad[1, 4, 0, 2] = np.nan
    rec = sm.sync_model(bad, gt, audio, parts, 30, 0.1)
    assert rec[:, sm.NONFINITE].tolist() == [0, 1, 0] and np.array_equal(rec[[0, 2]], clean[[0, 2]])
    noisy = audio.copy()
    noisy[2, 1234] = np.nan
    rec = sm.sync_model(pred, gt, noisy, parts, 30, 0.1)
    assert rec[:, sm.NONFINITE].tolist() == [0, 0, 1] and np.array_equal(rec[:2], clean[:2])
    noisy[2, 1234] = np.inf
    assert sm.sync_model(pred, gt, noisy, parts, 30, 0.1)[:, sm.NONFINITE].tolist() == [0, 0, 1]
    # a copy's NaN flags the clip of that copy
    p2, g2 = gestures(4, 17, 5, 5), gestures(4, 17, 5, 6)
    p2[3, 2, 1, 1] = np.nan  # row 3 = copy 1 of clip 1 (B = 2)
    assert sm.sync_model(p2, g2, audio[:2], parts, 30, 0.1, 2)[:, sm.NONFINITE].tolist() == [0, 1]


def test_epoch_model_leaves_flagged_clips_out_and_the_lowest_rank_wins():
    pred, gt, audio, parts = nan_cases()
    clean = sm.sync_model(pred, gt, audio, parts, 30, 0.1)
    flagged = clean.copy()
    flagged[1, sm.NONFINITE] = 1
    words = sm.epoch_model([flagged])
    assert np.array_equal(words[:20], sm.epoch_model([clean[[0, 2]]])[:20])
    assert words[sm.OUT_SEEN] == 3 and words[sm.OUT_NONFINITE] == 1
    v = sm.epoch_values(words)
    assert v['sync_clips_nonfinite'] == 1 and v['sync_clips_seen'] == 3
    beats = clean[[0, 2], sm.INT_PRED].sum()
    assert v['sync_precision'] == clean[[0, 2], sm.INT_PRED + 4].sum() / beats
    assert v['sync_offset_ms'] == (np.float64(clean[[0, 2], sm.INT_PRED + 8].sum()) * (1000.0 / 300.0)) / beats
    assert v['beats_per_s'] == beats * 15.0 / (2 * 17) and v['onsets_per_s'] == clean[[0, 2], sm.ONSETS].sum() * 100.0 / (2 * 40)
    assert v['sync_recall_hands'] == clean[[0, 2], sm.INT_PRED + 12 + 3].sum() / clean[[0, 2], sm.ONSETS].sum()
    assert v['sync_precision_gt_hands'] == clean[[0, 2], sm.INT_GT + 4 + 3].sum() / clean[[0, 2], sm.INT_GT + 3].sum()
    # ranks: clip 1 arrives at both, with different records; an unseen clip arrives nowhere
    other = sm.sync_model(gt, pred, audio, parts, 30, 0.1)
    r0, r1 = np.zeros((4, sm.COLS), dtype=np.int64), np.zeros((4, sm.COLS), dtype=np.int64)
    r0[[0, 1]], r1[[1, 2]] = clean[[0, 1]], other[[1, 2]]
    merged = sm.merge_tables([r0, r1])
    assert np.array_equal(merged[1], clean[1]) and np.array_equal(merged[2], other[2]) and not merged[3].any()
    assert np.array_equal(sm.epoch_model([r0, r1]), sm.epoch_model([merged]))
    assert not np.array_equal(sm.epoch_model([r1, r0]), sm.epoch_model([merged]))
    empty = sm.epoch_values(sm.epoch_model([np.zeros((5, sm.COLS), dtype=np.int64)], index_errors=2))
    assert empty['sync_precision'] == 0.0 and empty['onsets_per_s'] == 0.0 and empty['sync_index_errors'] == 2


# ---- the host interface --------------------------------------------------------------------------------------------------------------------------
def _cfg(*opts):
    cfg = get_cfg_defaults()
    cfg.merge_from_list(["PIPELINE_TYPE", "Voice2Pose"] + list(opts))
    return cfg


def test_config_defaults_and_every_rejected_value():
    cfg = get_cfg_defaults()
    assert cfg.TEST.SYNC_METRICS is False and cfg.TEST.SYNC_TOLERANCE == 0.1 and cfg.TEST.SYNC_SIGMA == 0.1
    assert check_sync_metrics(_cfg()) is None
    assert check_sync_metrics(_cfg("TEST.SYNC_METRICS", True)) == {'tol_ticks': 30, 'sigma': 0.1}
    for opts, key in ((("TEST.SYNC_METRICS", 1), "SYNC_METRICS"), (("TEST.SYNC_TOLERANCE", "x"), "SYNC_TOLERANCE"),
                      (("TEST.SYNC_TOLERANCE", 0.001), "SYNC_TOLERANCE"), (("TEST.SYNC_TOLERANCE", 0.51), "SYNC_TOLERANCE"),
                      (("TEST.SYNC_TOLERANCE", True), "SYNC_TOLERANCE"), (("TEST.SYNC_SIGMA", 0), "SYNC_SIGMA"),
                      (("TEST.SYNC_SIGMA", -1.0), "SYNC_SIGMA"), (("TEST.SYNC_SIGMA", float('nan')), "SYNC_SIGMA"),
                      (("TEST.SYNC_SIGMA", None), "SYNC_SIGMA")):
        with pytest.raises(ValueError, match=key):
            check_sync_metrics(_cfg(*opts))
    on = ("TEST.SYNC_METRICS", True)
    for opts, key in (((on + ("DATASET.AUDIO_SR", 22050)), "AUDIO_SR"), ((on + ("DATASET.FPS", 25)), "FPS"),
                      ((on + ("TEST.MULTIPLE", 17)), "MULTIPLE"), ((on + ("TEST.MULTIPLE", 0)), "MULTIPLE"),
                      ((on + ("PIPELINE_TYPE", "Pose2Pose")), "Voice2Pose")):
        with pytest.raises(ValueError, match=key):
            check_sync_metrics(_cfg(*opts))
    # with the key off the time base is not looked at
    assert check_sync_metrics(_cfg("DATASET.FPS", 25, "PIPELINE_TYPE", "Pose2Pose")) is None


def test_tolerance_to_ticks_rounding():
    assert sm.tolerance_ticks(0.1) == 30 and sm.tolerance_ticks(0.5) == 150 and sm.tolerance_ticks(1 / 300) == 1
    assert sm.tolerance_ticks(0.005) == 2 and sm.tolerance_ticks(0.0049) == 1 and sm.tolerance_ticks(0.0017) == 1  # floor(300 tol + 0.5)
    for bad in (0.0016, 0.502, -0.1, float('nan'), True, "0.1"):
        with pytest.raises(ValueError):
            sm.tolerance_ticks(bad)
    assert check_sync_metrics(_cfg("TEST.SYNC_METRICS", True, "TEST.SYNC_TOLERANCE", 0.005))['tol_ticks'] == 2


def test_command_line_arguments_and_npz_keys(tmp_path):
    a = sm.parse_args(["p.npz", "a.wav"])
    assert (a.poses, a.audio, a.tolerance, a.sigma, a.out, a.tolerance_ticks) == ("p.npz", "a.wav", 0.1, 0.1, None, 30)
    a = sm.parse_args(["p.npz", "a.npy", "--tolerance", "0.05", "--sigma", "0.2", "--out", "t.npz"])
    assert (a.tolerance_ticks, a.sigma, a.out) == (15, 0.2, "t.npz")
    for bad in (["p.npz"], ["p.npz", "a.npy", "--tolerance", "0.6"], ["p.npz", "a.npy", "--sigma", "0"]):
        with pytest.raises(SystemExit):
            sm.parse_args(bad)
    pred, gt, audio, parts = nan_cases()
    path = str(tmp_path / "t.npz")
    sm.save_table(path, sm.sync_model(pred, gt, audio, parts, 30, 0.1), 30, 0.1)
    with np.load(path) as z:
        assert sorted(z.files) == ["columns", "sigma", "table", "tolerance_ticks"]
        assert z["table"].shape == (3, sm.COLS) and tuple(z["columns"]) == sm.COLUMN_NAMES and int(z["tolerance_ticks"]) == 30
    assert sm.COLUMN_NAMES[sm.INT_PRED + 4 + 3] == "hits_pred_hands" and sm.COLUMN_NAMES[sm.INT_GT + 12] == "covered_gt_all"
    # audio files: .npy of one clip or of several, and 16-bit PCM wav
    np.save(str(tmp_path / "a.npy"), audio[0])
    assert sm.load_audio(str(tmp_path / "a.npy")).shape == (1, 6401)
    import wave
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes((np.clip(audio[0], -1, 1) * 32767).astype("<i2").tobytes())
    x = sm.load_audio(str(tmp_path / "a.wav"))
    assert x.shape == (1, 6401) and x.dtype == np.float32 and np.abs(x[0] - np.clip(audio[0], -1, 1)).max() < 1e-4
    with wave.open(str(tmp_path / "b.wav"), "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(8000)
        w.writeframes(b"\0\0" * 10)
    with pytest.raises(ValueError, match="16000"):
        sm.load_audio(str(tmp_path / "b.wav"))


def test_the_device_route_refuses_cpu_tensors():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sm.SyncAccumulator(4, 5, 30, 0.1, "cpu", parts=part_table(5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sm.onsets(torch.zeros(1000))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sm.beats(torch.zeros((1, 4, 2, 5), dtype=torch.float64))
    with pytest.raises(ValueError, match="K = 129"):
        sm.SyncAccumulator(4, 129, 30, 0.1, "cuda", parts=[0] * 129)
    with pytest.raises(ValueError, match="tolerance"):
        sm.SyncAccumulator(4, 5, 151, 0.1, "cuda", parts=part_table(5))
