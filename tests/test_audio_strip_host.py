"""The audio strip's host side (speechdrivestemplates_amd/audio_strip.py): the column layouts, the per-frame window
tables, the numpy contract models on hand-made inputs, and SYS.AUDIO_STRIP's validation.  No GPU."""
import numpy as np
import pytest

from speechdrivestemplates_amd import audio_strip as st
from speechdrivestemplates_amd.config import check_audio_strip, get_cfg_defaults
from speechdrivestemplates_amd.render import LONG_W, long_image_layout


# ---- layouts -------------------------------------------------------------------------------------------------------------------------------------
def test_uniform_bounds_short_ragged_and_the_documented_clip():
    bounds, spc, Nc, scrolls = st.uniform_bounds(100, 1280, 68800)  # L < W: one sample per column, fewer columns than pixels
    assert (spc, Nc, scrolls) == (1, 100, False) and Nc < 1280 and bounds.tolist() == list(range(101))
    bounds, spc, Nc, scrolls = st.uniform_bounds(1000, 64, 68800)  # ceil(1000 / 64) = 16, 1000 = 62 * 16 + 8: a ragged last column
    assert (spc, Nc) == (16, 63) and bounds[-1] == 63 * 16 > 1000 > bounds[-2] and bounds.dtype == np.int64
    assert np.array_equal(np.diff(bounds), np.full(Nc, spc))
    bounds, spc, Nc, scrolls = st.uniform_bounds(68267, 1280, st.span_samples(4.3))  # a 64-frame clip
    assert st.span_samples(4.3) == 68800 and (spc, Nc, scrolls) == (54, 1265, False)


def test_uniform_bounds_stands_at_the_span_and_scrolls_one_sample_later():
    span = 68800
    _, spc, Nc, scrolls = st.uniform_bounds(span, 1280, span)
    assert not scrolls and spc == 54 and Nc == -(-span // 54) <= 1280
    _, spc1, Nc1, scrolls1 = st.uniform_bounds(span + 1, 1280, span)
    assert scrolls1 and spc1 == 54 and Nc1 == -(-(span + 1) // 54)
    for bad in ((0, 10, 10), (10, 0, 10), (10, 10, 0)):
        with pytest.raises(ValueError):
            st.uniform_bounds(*bad)


@pytest.mark.parametrize("T", [1, 8, 9, 64, 65, 360])
def test_long_image_bounds_sit_under_the_window_centres(T):
    width, windows = long_image_layout(T)
    bounds = st.long_image_bounds(T, 16000)
    assert bounds.dtype == np.int64 and bounds.shape == (width + 1,)
    assert (np.diff(bounds) >= 0).all()
    for j, (i, x0) in enumerate(windows):
        assert i == 8 * j and bounds[x0 + LONG_W // 2] == (8 * j * 16000) // 15
    # left of the first centre and right of the last one the neighbouring slope goes on (one window: 8533 samples over 503 columns)
    cx = [x0 + LONG_W // 2 for _, x0 in windows] + ([LONG_W // 2 + 503] if len(windows) == 1 else [])
    s = [(8 * j * 16000) // 15 for j in range(len(cx))]
    assert bounds[0] == s[0] + ((0 - cx[0]) * (s[1] - s[0])) // (cx[1] - cx[0]) < 0
    assert bounds[width] == s[-2] + ((width - cx[-2]) * (s[-1] - s[-2])) // (cx[-1] - cx[-2])


def test_long_image_bounds_refuse_nonsense():
    for bad in ((0, 100), (9, 0)):
        with pytest.raises(ValueError):
            st.long_image_bounds(*bad)


def test_frame_tables_of_a_scrolling_and_a_standing_piece():
    W, n = 1280, 900
    L = n * 16000 // 15
    _, spc, Nc, scrolls = st.uniform_bounds(L, W, 68800)
    assert scrolls and spc == 54
    c0, ph = st.frame_tables(n, W, spc, Nc, scrolls)
    assert c0.dtype == np.int32 and ph.dtype == np.int32 and c0.shape == ph.shape == (n,)
    assert c0[0] == -(W // 2) < 0 and c0[-1] + W > Nc
    assert ((ph - c0) == W // 2).all()  # the playhead stays in the middle
    assert [int(p) for p in ph[:3]] == [0, 1066 // 54, 2133 // 54]
    _, spc, Nc, scrolls = st.uniform_bounds(68267, W, 68800)
    c0, ph = st.frame_tables(64, W, spc, Nc, scrolls)
    assert not scrolls and not c0.any() and ((ph >= 0) & (ph < W)).all() and ph[63] == (63 * 16000 // 15) // 54
    # more frames than audio: a playhead that would leave the picture is left out, never drawn outside [0, W)
    c0, ph = st.frame_tables(40, 8, 1000, 8, False)
    shown = ph[ph >= 0]
    assert (ph[8:] == -1).all() and ((shown - c0[ph >= 0] >= 0) & (shown - c0[ph >= 0] < 8)).all()


# ---- the models on hand-made inputs --------------------------------------------------------------------------------------------------------------
S = 160
SW, Y_MARK, Y_MEL, SM = st.lanes(S)


def test_lane_partition():
    assert (SW, Y_MARK, Y_MEL, SM) == (60, 60, 84, 76)
    assert st.lanes(64) == (24, 24, 48, 16) and st.lanes(80) == (30, 30, 54, 26)
    for bad in (63, 1025, 64.0, True):
        with pytest.raises(ValueError):
            st.lanes(bad)


def _flat_mel(n_mels=4, F=4, value=1.0):
    return np.full((n_mels, F), value, dtype=np.float32)


def test_a_full_scale_impulse_fills_from_the_top_row_to_the_zero_row():
    x = np.zeros(64, dtype=np.float32)
    x[20] = 1.0
    bounds = np.arange(0, 65, 8)  # 8 columns of 8 samples; the impulse is in column 2
    env = st.envelope_model(x, bounds)
    assert env['peak'] == 1.0 and env['nonfinite'] == 0 and (env['flags'] == st.OK).all()
    assert env['env'][2].tolist() == [0.0, 1.0] and not env['env'][[0, 1, 3]].any()
    band = st.raster_model(env, bounds, _flat_mel(), S)
    zero_row = int(np.floor((SW - 1) / 2 + 0.5))  # floor((1 - 0) * 59 / 2 + 0.5) = 30
    assert zero_row == 30
    col = band[:SW, 2]
    assert (col[:zero_row + 1] == st.WAVE).all() and (col[zero_row + 1:] == st.BACKGROUND).all()
    other = band[:SW, 1]  # a silent column: one row at the centre
    assert (other[zero_row] == st.WAVE).all() and (np.delete(other, zero_row, 0) == st.BACKGROUND).all()


def test_all_zero_audio_is_a_one_row_bar_through_the_peak_floor():
    x = np.zeros(32, dtype=np.float32)
    bounds = np.arange(0, 33, 8)
    env = st.envelope_model(x, bounds)
    assert env['peak'] == 0.0  # g = 1 / 2^-15, a = 0 * g = 0: no division by zero, no NaN
    band = st.raster_model(env, bounds, _flat_mel(), S)
    rows = np.flatnonzero((band[:SW, 0] == st.WAVE).all(axis=1))
    assert rows.tolist() == [30] and (band[:SW] == band[:SW, :1]).all()
    tiny = np.full(32, 2.0 ** -20, dtype=np.float32)  # below the floor: a = 2^-5, row floor(29.5 - 0.92 + 0.5) = 29
    band = st.raster_model(st.envelope_model(tiny, bounds), bounds, _flat_mel(), S)
    assert np.flatnonzero((band[:SW, 0] == st.WAVE).all(axis=1)).tolist() == [29]


def test_a_power_on_a_threshold_takes_the_index_of_that_threshold():
    k = st.factor_table(80.0)
    assert k.dtype == np.float32 and k.shape == (255,) and k[-1] == 1.0 and (np.diff(k) > 0).all()
    ref = np.float32(3.7)
    thresholds = ref * k
    assert thresholds.dtype == np.float32
    cmap = st.colormap()
    x = np.ones(16, dtype=np.float32)
    bounds = np.array([0, 16])
    for i in (1, 77, 200, 255):  # index i counts the thresholds 1 .. i, so p = fl32(ref * k[i]) gives i and the next float below gives i - 1
        p = thresholds[i - 1]
        for value, want in ((p, i), (np.nextafter(p, np.float32(0.0)), i - 1)):
            mel = np.array([[value], [ref]], dtype=np.float32)  # bin 0 holds the probe, bin 1 the reference power
            band = st.raster_model(st.envelope_model(x, bounds), bounds, mel, S)
            assert (band[S - 1, 0] == cmap[want]).all(), (i, want)  # the bottom row of the mel lane is bin 0
            assert (band[Y_MEL, 0] == cmap[255]).all()  # the top row is the last bin: the reference itself
    assert cmap[0].tolist() == [0, 0, 0] and cmap[255].tolist() == [255, 255, 255] and cmap[100].tolist() == [0, 45, 255]


def test_an_onset_and_a_beat_in_one_column_land_in_different_lanes():
    x = np.ones(1600, dtype=np.float32)
    bounds = np.arange(0, 1601, 100)  # 16 columns of 100 samples
    env = st.envelope_model(x, bounds)
    # tick 9 is at sample 9 * 16000 // 300 = 480, tick 8 at 426: both in column 4
    assert st.tick_sample(9) == 480 and st.tick_sample(8) == 426
    band = st.raster_model(env, bounds, _flat_mel(), S, marks=[[9], [8], None])
    lane = lambda q: band[Y_MARK + q * st.MARK_ROWS:Y_MARK + (q + 1) * st.MARK_ROWS]  # noqa: E731
    for q in (0, 1):
        assert (lane(q)[:, 4:4 + st.TICK_WIDTH] == st.MARKS[q]).all()
        assert (np.delete(lane(q), [4, 5], axis=1) == st.BACKGROUND).all()
    assert (lane(2) == st.BACKGROUND).all()  # an absent list: an empty lane
    # ticks before 0 and past the band are ignored; one in the last column is clipped to it
    band = st.raster_model(env, bounds, _flat_mel(), S, marks=[[-3, 30, 10 ** 6], None, [29, 29]])
    assert (band[Y_MARK:Y_MARK + st.MARK_ROWS] == st.BACKGROUND).all()  # (tick 30 is sample 1600 = bounds[16]: past the band)
    gt_lane = band[Y_MARK + 2 * st.MARK_ROWS:Y_MARK + 3 * st.MARK_ROWS]
    assert (gt_lane[:, 15] == st.MARKS[2]).all() and (gt_lane[:, :15] == st.BACKGROUND).all()  # tick 29: sample 1546, column 15
    with pytest.raises(ValueError):
        st.raster_model(env, bounds, _flat_mel(), S, marks=[None] * 4)


def test_nonfinite_samples_are_selected_away_and_flag_their_column():
    x = np.array([0.5, np.nan, -0.25, np.inf, 1.0, -np.inf, 0.0, -0.0], dtype=np.float32)
    bounds = np.array([-4, 0, 3, 4, 4, 8, 20, 30])  # before 0, finite + NaN, inf alone, empty, -inf + signed zeros, ragged past L, past L
    env = st.envelope_model(x, bounds)
    assert env['flags'].tolist() == [st.EMPTY, st.NONFINITE, st.NONFINITE, st.EMPTY, st.NONFINITE, st.EMPTY, st.EMPTY]
    assert env['peak'] == 1.0 and env['nonfinite'] == 3
    assert env['env'][1].tolist() == [-0.25, 0.5] and env['env'][2].tolist() == [0.0, 0.0]
    lo, hi = env['env'][4]
    assert (lo, hi) == (0.0, 1.0) and np.signbit(lo)  # -0 orders below +0: the minimum of {1, 0, -0} is -0
    band = st.raster_model(env, bounds, _flat_mel(), S)
    assert (band[:SW, 1] == st.WARNING).all() and (band[:, 0] == st.BACKGROUND).all() and (band[:, 3] == st.BACKGROUND).all()
    mel = np.array([[np.nan, 1.0], [np.inf, 0.5]], dtype=np.float32)  # non-finite powers: the warning colour, and no part of the reference
    assert st.mel_ref(mel) == 1.0
    band = st.raster_model(st.envelope_model(np.ones(320, dtype=np.float32), np.array([0, 160, 320])), np.array([0, 160, 320]), mel, S)
    assert (band[Y_MEL:, 0] == st.WARNING).all() and (band[S - 1, 1] == 255).all()


def test_compose_model_windows_and_playhead():
    rng = np.random.Generator(np.random.PCG64(3))
    frames = rng.integers(0, 256, (3, 5, 10, 3), dtype=np.uint8)
    band = rng.integers(0, 256, (64, 6, 3), dtype=np.uint8)
    out = st.compose_model(frames, band, [0, -3, 4], [0, 5, -1])
    assert out.shape == (3, 69, 10, 3) and np.array_equal(out[:, :5], frames)
    assert (out[0, 5:, :2] == st.PLAYHEAD).all() and np.array_equal(out[0, 5:, 2:6], band[:, 2:6]) and (out[0, 5:, 6:] == st.BACKGROUND).all()
    assert (out[1, 5:, :3] == st.BACKGROUND).all() and np.array_equal(out[1, 5:, 3:8], band[:, :5]) and (out[1, 5:, 8:] == st.PLAYHEAD).all()
    assert np.array_equal(out[2, 5:, :2], band[:, 4:]) and (out[2, 5:, 2:] == st.BACKGROUND).all()


# ---- configuration -------------------------------------------------------------------------------------------------------------------------------
def _cfg(*opts):
    cfg = get_cfg_defaults()
    cfg.merge_from_list(["PIPELINE_TYPE", "Voice2Pose"] + list(opts))
    return cfg


def test_config_defaults_and_every_refusal_names_its_key():
    cfg = _cfg()
    assert dict(cfg.SYS.AUDIO_STRIP) == {"ENABLE": False, "HEIGHT": 160, "SPAN_S": 4.3, "MARKS": True, "DB_RANGE": 80.0}
    assert check_audio_strip(cfg) is None
    on = ["SYS.AUDIO_STRIP.ENABLE", True, "SYS.RENDER_VIDEO", True]
    assert check_audio_strip(_cfg(*on)) == {"height": 160, "span_s": 4.3, "marks": True, "db_range": 80.0}
    for key, values in (("HEIGHT", (48, 528, 72, 160.0, True)), ("SPAN_S", (0.5, 61, "x", float("nan"))), ("DB_RANGE", (19.9, 121, None)),
                        ("ENABLE", (1, "yes")), ("MARKS", (0, None))):
        for v in values:  # checked with the key off too
            with pytest.raises(ValueError, match="SYS.AUDIO_STRIP." + key):
                check_audio_strip(_cfg("SYS.AUDIO_STRIP." + key, v))
    for opts, word in ((["SYS.AUDIO_STRIP.ENABLE", True], "SYS.RENDER_VIDEO"), (on + ["PIPELINE_TYPE", "Pose2Pose"], "Voice2Pose"),
                       (on + ["DATASET.AUDIO_SR", 22050], "DATASET.AUDIO_SR"), (on + ["DATASET.FPS", 25], "DATASET.FPS"),
                       (on + ["SYS.DEVICE_JPEG", True, "SYS.CANVAS_SIZE", (65400, 1280)], "HEIGHT")):
        with pytest.raises(ValueError, match="SYS.AUDIO_STRIP.*" + word):
            check_audio_strip(_cfg(*opts))
    assert check_audio_strip(_cfg(*(on + ["SYS.CANVAS_SIZE", (65400, 1280)])))["height"] == 160  # (PIL writes those frames)


def test_the_device_route_refuses_cpu_tensors():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.strip_for_clip(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(8), torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.strip_for_long_image(torch.zeros(720, 960, 3, dtype=torch.uint8), torch.zeros(8), torch.zeros(2, 2), 1)
