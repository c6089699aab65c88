"""The whole-recording demo (speechdrivestemplates_amd/long_demo.py) without a GPU: the window layout, the numpy contract
models of the blend, the smoother and the report against plain formulas, the config check and the command line's arguments.

Bars.  The unit roundoff of float64 is 2^-53.  A blended value is at most three products, two sums and one division of positive numbers, so
two formulations of it differ by at most 4 * 2^-52 relative; identical windows give (sum w g) / (sum w) = g within 2 * 2^-52 relative.  A sum
of n non-negative terms differs between two orders by at most (n - 1) 2^-52 relative and the two formulations of a term (separately rounded
operations here, np.linalg.norm there) by 2 ulp: together (n + 2) 2^-52.  Counts are integers and must be equal.
"""
import numpy as np
import pytest

from speechdrivestemplates_amd import long_demo as ld
from speechdrivestemplates_amd.config import check_long_demo, get_cfg_defaults
from speechdrivestemplates_amd.core.datasets.gesture_dataset import PoseTransforms, parse_audio_length

ULP = 2.0 ** -52
SR, FPS = 16000, 15
LW = parse_audio_length(68267, SR, FPS)[0]
LAYOUTS = [(F, 8, O) for O in (0, 1, 3, 4) for F in range(8, 33)] + [(F, 64, O) for O in (0, 16, 32) for F in (64, 65, 111, 112, 113, 160, 4500)]
# (F, W, O, K) of the device tests (tests/test_long_demo_gpu.py uses the same list)
SHAPES = [(8, 8, 0, 1), (9, 8, 4, 1), (17, 8, 3, 5), (65, 64, 16, 121), (113, 64, 32, 121), (160, 64, 0, 64), (300, 64, 16, 128)]


def part_table(K):
    return PoseTransforms.part_table() if K == 121 else [k % 3 for k in range(K)]


def window_poses(F, W, O, K, seed=0):
    """window poses as a network would give them: one smooth positive trajectory over the recording (pixels), each window a few pixels off it"""
    rng = np.random.Generator(np.random.PCG64(1000 * seed + 7 * F + 3 * W + 11 * O + K))
    starts, _ = ld.window_layout(F, W, O)
    t = np.arange(F)[:, None, None]
    base = 300.0 + 100.0 * np.sin(0.05 * t + rng.uniform(0, 6.0, (1, 2, K))) + rng.uniform(0.0, 200.0, (1, 2, K))
    return np.stack([base[s:s + W] + 3.0 * rng.standard_normal((W, 2, K)) for s in starts])


def test_layout_properties():
    assert LW == 68266
    for F, W, O in LAYOUTS:
        starts, offsets = ld.window_layout(F, W, O, SR, FPS)
        H = W - O
        assert len(starts) == 1 + -(-(F - W) // H)
        assert starts[0] == 0 and starts[-1] + W == F, (F, W, O)  # the last window ends at F
        assert all(b > a for a, b in zip(starts, starts[1:])), (F, W, O)
        assert starts[:-1] == [i * H for i in range(len(starts) - 1)]
        cover = np.zeros(F, dtype=np.int64)
        for s in starts:
            cover[s:s + W] += 1
        assert cover.min() >= 1 and cover.max() <= 3, (F, W, O, cover.min(), cover.max())
        for t in (0, W - 1, F // 2, F - W, F - 1):
            idx = ld.covering(t, starts, W)
            assert idx == sorted(idx) and len(idx) == cover[t]
        assert offsets == [(s * SR) // FPS for s in starts]
        if W == 64:  # (Lw is the length of 64 frames)
            assert all(a + LW <= int(F * SR / FPS) + 1 for a in offsets), (F, W, O)


@pytest.mark.parametrize("bad", [dict(F=7, W=8, O=0), dict(F=8, W=8, O=5), dict(F=8, W=8, O=-1), dict(F=8, W=1, O=0), dict(F=8.0, W=8, O=0)])
def test_layout_rejects(bad):
    with pytest.raises(ValueError):
        ld.window_layout(bad["F"], bad["W"], bad["O"])


def plain_stitch(windows, O, F):
    N, W, _, K = windows.shape
    starts, _ = ld.window_layout(F, W, O)
    w = np.zeros((N, F))
    x = np.zeros((N, F, 2, K))
    for i, s in enumerate(starts):
        u = np.minimum(np.arange(s, s + W) - s + 1, s + W - np.arange(s, s + W))
        w[i, s:s + W] = np.minimum(u, max(O, 1))
        x[i, s:s + W] = windows[i]
    return np.sum(w[:, :, None, None] * x, axis=0) / np.sum(w, axis=0)[:, None, None], (w > 0).sum(axis=0)


@pytest.mark.parametrize("shape", SHAPES + [(32, 8, 4, 3), (4500, 64, 16, 2)], ids=lambda s: "x".join(map(str, s)))
def test_stitch_model_against_plain_formula(shape):
    F, W, O, K = shape
    win = window_poses(F, W, O, K)
    got = ld.stitch_model(win, O, F)
    want, cover = plain_stitch(win, O, F)
    assert got.shape == (F, 2, K)
    err = np.abs(got - want) / np.abs(want)
    assert err.max() <= 4 * ULP, err.max()
    starts, _ = ld.window_layout(F, W, O)
    for t in np.nonzero(cover == 1)[0]:  # a frame one window covers is that window's value, bit for bit
        i = ld.covering(int(t), starts, W)[0]
        assert np.array_equal(got[t].view(np.int64), win[i, t - starts[i]].view(np.int64))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stitch_model_identical_windows(shape):
    F, W, O, K = shape
    rng = np.random.Generator(np.random.PCG64(5))
    g = rng.uniform(1.0, 500.0, (F, 2, K))
    starts, _ = ld.window_layout(F, W, O)
    got = ld.stitch_model(np.stack([g[s:s + W] for s in starts]), O, F)
    assert (np.abs(got - g) <= 2 * ULP * np.abs(g)).all()


def test_stitch_model_without_overlap_is_concatenation():
    win = window_poses(16, 8, 0, 7)
    assert win.shape[0] == 2
    assert np.array_equal(ld.stitch_model(win, 0, 16).view(np.int64), np.concatenate([win[0], win[1]]).view(np.int64))
    assert np.array_equal(ld.stitch_model(win, 0).view(np.int64), np.concatenate([win[0], win[1]]).view(np.int64))  # (F defaults to N W)


def test_stitch_model_rejects_a_wrong_window_count():
    with pytest.raises(ValueError, match="windows"):
        ld.stitch_model(np.zeros((2, 8, 2, 1)), 0, 8)
    with pytest.raises(ValueError):
        ld.stitch_model(np.zeros((1, 8, 2, 129)), 0, 8)


@pytest.mark.parametrize("m,d", [(1, 0), (2, 2), (4, 3), (8, 3), (8, 5)])
def test_smooth_model_reproduces_polynomials(m, d):
    F = 40
    t = np.arange(F, dtype=np.float64)
    x = np.zeros((F, 2, 3))
    for k in range(3):
        deg = min(d, k + 1) if d else 0
        x[:, 0, k] = sum((0.3 + 0.1 * q) * (t / 10.0) ** q for q in range(deg + 1))
        x[:, 1, k] = 2.0 + (t / 7.0) ** deg
    y = ld.smooth_model(x, (m, d))
    inner = slice(m, F - m)
    assert np.allclose(y[inner], x[inner], rtol=1e-12, atol=0)
    assert y is not x and y.shape == x.shape


def test_smooth_model_degree_zero_is_the_moving_average_and_scipy_agrees():
    rng = np.random.Generator(np.random.PCG64(3))
    x = rng.uniform(0.0, 400.0, (50, 2, 4))
    for m in (1, 3, 8):
        c = ld.savgol_table(m, 0)
        assert np.allclose(c, 1.0 / (2 * m + 1), rtol=1e-14)
        pad = np.concatenate([np.repeat(x[:1], m, 0), x, np.repeat(x[-1:], m, 0)])
        avg = np.mean(np.stack([pad[j:j + 50] for j in range(2 * m + 1)]), axis=0)
        assert np.allclose(ld.smooth_model(x, (m, 0)), avg, rtol=1e-12, atol=0)
    assert ld.smooth_model(x, None) is x
    signal = pytest.importorskip("scipy.signal")
    for m, d in ((1, 0), (2, 2), (8, 3), (5, 4)):
        want = signal.savgol_filter(x, 2 * m + 1, d, axis=0, mode="nearest")
        assert np.allclose(ld.smooth_model(x, (m, d)), want, rtol=1e-12, atol=0), (m, d)


@pytest.mark.parametrize("m,d", [(0, 0), (9, 2), (2, 5), (2, -1), (2.0, 1), (True, 0)])
def test_savgol_table_rejects(m, d):
    with pytest.raises(ValueError):
        ld.savgol_table(m, d)


def plain_report(win, stitched, smoothed, O, parts):
    N, W, _, K = win.shape
    F = stitched.shape[0]
    starts, _ = ld.window_layout(F, W, O)
    parts = np.asarray(parts)
    masks = [np.ones(K, dtype=bool)] + [parts == i for i in range(3)]
    sums, counts = np.zeros((5, 4)), np.zeros((3, 4), dtype=np.int64)
    for g, x in ((0, stitched), (2, smoothed)):
        if x is None:
            continue
        speed = np.linalg.norm(x[1:] - x[:-1], axis=1)
        jerk = np.linalg.norm(x[3:] - 3.0 * x[2:-1] + 3.0 * x[1:-2] - x[:-3], axis=1) if F > 3 else np.zeros((0, K))
        for p, mk in enumerate(masks):
            sums[g, p], sums[g + 1, p] = np.sum(speed[:, mk]), np.sum(jerk[:, mk])
    seam, n_pairs = np.zeros(K), 0
    for t in range(F):
        idx = [i for i, s in enumerate(starts) if s <= t < s + W]
        for a in range(len(idx)):
            for b in range(a + 1, len(idx)):
                seam = seam + np.linalg.norm(win[idx[a], t - starts[idx[a]]] - win[idx[b], t - starts[idx[b]]], axis=0)
                n_pairs += 1
    for p, mk in enumerate(masks):
        sums[4, p] = np.sum(seam[mk])
        counts[:, p] = (F - 1) * mk.sum(), max(F - 3, 0) * mk.sum(), n_pairs * mk.sum()
    return sums.reshape(20), counts, n_pairs


@pytest.mark.parametrize("shape", SHAPES + [(8, 8, 4, 3)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("smooth", [None, (2, 2)], ids=["plain", "smoothed"])
def test_report_model_against_plain_formulas(shape, smooth):
    F, W, O, K = shape
    win = window_poses(F, W, O, K)
    parts = part_table(K)
    stitched = ld.stitch_model(win, O, F)
    smoothed = None if smooth is None else ld.smooth_model(stitched, smooth)
    words, tot = ld.report_model(win, stitched, smoothed, O, parts, return_sums=True)
    sums, counts, n_pairs = plain_report(win, stitched, smoothed, O, parts)
    assert np.array_equal(words[ld.N_SPEED:ld.N_SPEED + 4], counts[0]) and np.array_equal(words[ld.N_JERK:ld.N_JERK + 4], counts[1])
    assert np.array_equal(words[ld.N_SEAM:ld.N_SEAM + 4], counts[2])
    assert (words[ld.NONFINITE], words[ld.FRAMES], words[ld.WINDOWS], words[ld.SMOOTHED], words[ld.PAIR_FRAMES]) == (
        0, F, win.shape[0], int(smooth is not None), n_pairs)
    assert not words[37:].any()
    n = np.array([counts[2 if g == 4 else g & 1][p] for g in range(5) for p in range(4)])
    assert (np.abs(tot - sums) <= (n + 2) * ULP * np.abs(sums)).all(), np.abs(tot - sums) / np.maximum(np.abs(sums), 1e-300)
    means = words[:20].view(np.float64)
    want = np.where(n > 0, sums / np.maximum(n, 1), 0.0)
    assert (np.abs(means - want) <= (n + 3) * ULP * np.abs(want)).all()  # (one more rounding: the division)
    if smooth is None:
        assert not words[8:16].any()
    v = ld.report_values(words)
    assert v["frames"] == F and ("speed_smoothed" in v) == (smooth is not None) and set(v["seam"]) == {"all", "body", "face", "hands"}
    assert isinstance(ld.describe(words), str)


def test_report_model_seam_is_zero_for_identical_windows_and_a_nan_sets_the_flag():
    F, W, O, K = 113, 64, 32, 121
    rng = np.random.Generator(np.random.PCG64(9))
    g = rng.uniform(1.0, 500.0, (F, 2, K))
    starts, _ = ld.window_layout(F, W, O)
    win = np.stack([g[s:s + W] for s in starts])
    stitched = ld.stitch_model(win, O, F)
    words = ld.report_model(win, stitched, None, O)
    assert words[ld.PAIR_FRAMES] > 0 and words[ld.NONFINITE] == 0
    assert np.array_equal(words[16:20], np.zeros(4, dtype=np.int64))  # exactly +0.0
    win[1, 5, 0, 100] = np.nan
    stitched = ld.stitch_model(win, O, F)
    assert np.isnan(stitched[starts[1] + 5, 0, 100]) and np.isnan(stitched).sum() == 1
    words = ld.report_model(win, stitched, None, O)
    assert words[ld.NONFINITE] == 1
    f = words[:20].view(np.float64)
    assert np.isnan(f[0]) and np.isnan(f[3]) and np.isfinite(f[1]) and np.isfinite(f[2])  # keypoint 100 is a hand keypoint


def _cfg(*opts):
    cfg = get_cfg_defaults()
    cfg.merge_from_list(["PIPELINE_TYPE", "Voice2Pose"] + list(opts))
    return cfg


def test_config_defaults_and_accepted_values():
    cfg = get_cfg_defaults()
    assert (cfg.DEMO.LONG_FORM, cfg.DEMO.WINDOW_OVERLAP, cfg.DEMO.LONG_BATCH, cfg.DEMO.SMOOTH, cfg.DEMO.SEGMENT_FRAMES) == (False, 16, 32, None, 900)
    assert check_long_demo(cfg) is None
    assert check_long_demo(_cfg("DEMO.LONG_FORM", True)) == {"overlap": 16, "batch": 32, "smooth": None, "segment": 900}
    got = check_long_demo(_cfg("DEMO.LONG_FORM", True, "DEMO.WINDOW_OVERLAP", 32, "DEMO.LONG_BATCH", 256, "DEMO.SMOOTH", [8, 16],
                               "DEMO.SEGMENT_FRAMES", 64))
    assert got == {"overlap": 32, "batch": 256, "smooth": (8, 16), "segment": 64}
    assert check_long_demo(_cfg("DEMO.LONG_FORM", True, "DEMO.WINDOW_OVERLAP", 0, "DEMO.LONG_BATCH", 1, "DEMO.SMOOTH", [1, 0]))["smooth"] == (1, 0)


@pytest.mark.parametrize("key,value", [
    ("DEMO.LONG_FORM", 1), ("DEMO.LONG_FORM", "yes"),
    ("DEMO.WINDOW_OVERLAP", -1), ("DEMO.WINDOW_OVERLAP", 33), ("DEMO.WINDOW_OVERLAP", 16.0), ("DEMO.WINDOW_OVERLAP", True),
    ("DEMO.WINDOW_OVERLAP", None),
    ("DEMO.LONG_BATCH", 0), ("DEMO.LONG_BATCH", 257), ("DEMO.LONG_BATCH", 2.5), ("DEMO.LONG_BATCH", None),
    ("DEMO.SMOOTH", 3), ("DEMO.SMOOTH", [2]), ("DEMO.SMOOTH", [0, 0]), ("DEMO.SMOOTH", [9, 2]), ("DEMO.SMOOTH", [2, 5]), ("DEMO.SMOOTH", [2, -1]),
    ("DEMO.SMOOTH", [2.0, 1]), ("DEMO.SMOOTH", [2, 1, 0]),
    ("DEMO.SEGMENT_FRAMES", 63), ("DEMO.SEGMENT_FRAMES", 0), ("DEMO.SEGMENT_FRAMES", 900.0), ("DEMO.SEGMENT_FRAMES", None),
    ("DATASET.NUM_FRAMES", 1),
])
def test_config_rejects(key, value):
    opts = [key, value] if key == "DEMO.LONG_FORM" else ["DEMO.LONG_FORM", True, key, value]
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        check_long_demo(_cfg(*opts))


def test_config_rejects_other_pipelines_and_the_ground_truth_code():
    cfg = get_cfg_defaults()
    cfg.merge_from_list(["PIPELINE_TYPE", "Pose2Pose", "DEMO.LONG_FORM", True])
    with pytest.raises(ValueError, match=r"DEMO\.LONG_FORM"):
        check_long_demo(cfg)
    with pytest.raises(ValueError, match="TEST_WITH_GT_CODE"):
        check_long_demo(_cfg("DEMO.LONG_FORM", True, "VOICE2POSE.GENERATOR.CLIP_CODE.TEST_WITH_GT_CODE", True))
    # the keys of a run that does not use them are type-checked only: a short NUM_FRAMES with the default overlap is no error
    assert check_long_demo(_cfg("DATASET.NUM_FRAMES", 16)) is None
    with pytest.raises(ValueError, match=r"DEMO\.LONG_BATCH"):
        check_long_demo(_cfg("DEMO.LONG_BATCH", 0))


def test_segments_cover_the_frames():
    assert ld.segments(150, 100) == [(0, 75), (75, 150)]
    assert ld.segments(900, 900) == [(0, 900)] and ld.segments(64, 900) == [(0, 64)]
    for F, lim in ((4500, 900), (4501, 900), (129, 64), (1000, 333)):
        segs = ld.segments(F, lim)
        assert segs[0][0] == 0 and segs[-1][1] == F and all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
        assert all(0 < b - a <= lim for a, b in segs) and len(segs) == -(-F // lim)


def test_command_line_arguments():
    a = ld.parse_args(["w.npy", "out.npz"])
    assert (a.windows, a.out, a.overlap, a.frames, a.smooth) == ("w.npy", "out.npz", 16, None, None)
    a = ld.parse_args(["w.npy", "out.npz", "--overlap", "8", "--frames", "150", "--smooth", "2", "3"])
    assert (a.overlap, a.frames, a.smooth) == (8, 150, [2, 3])
    for bad in (["w.npy"], ["w.npy", "o.npz", "--overlap", "-1"], ["w.npy", "o.npz", "--smooth", "9", "1"], ["w.npy", "o.npz", "--smooth", "2"],
                ["w.npy", "o.npz", "--smooth", "2", "5"]):
        with pytest.raises(SystemExit):
            ld.parse_args(bad)
    assert ld.OUT_KEYS == ("poses_stitched", "poses_pred_batch", "window_starts", "long_report")


def test_device_functions_refuse_cpu_tensors():
    import torch
    x = torch.zeros(1, 8, 2, 1, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ld.stitch(x, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ld.smooth(x[0], (1, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ld.report(x, x[0], None, 0, [0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ld.gather_windows(torch.zeros(10), [0], 4)
