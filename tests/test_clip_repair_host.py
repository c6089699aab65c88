"""The repair stage's numpy contract models (speechdrivestemplates_amd/clip_builder.py) against an independent
per-track python loop with np.interp (tests/golden/synth_repair_videos.py), hand-written despike cases, and the argument checks of
build_clips.  No GPU."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import synth_repair_videos as R  # noqa: E402

from speechdrivestemplates_amd import clip_builder as cb  # noqa: E402

CASES = [(v, g, d, dt) for v, g, d in R.PARAMS for dt in ('float32', 'float64')]


@pytest.mark.parametrize("video,max_gap,despike,dtype", CASES)
def test_models_equal_the_loop_reference(video, max_gap, despike, dtype):
    """Decisions and counts are equal.  Values: the model forms xa + (xb - xa) * ((f - a) / (b - a)), np.interp a slope form of the same
    line; either makes at most four float64 roundings of quantities no larger than 2 * max(|xa|, |xb|), so they agree within 8 ulp of
    that.  In float32 the two float64 values round to neighbours at worst: 1 ulp of the result."""
    a, present = R.video_frames(video, dtype)
    want = R.reference(video, dtype, max_gap, despike)
    got = cb.model_repair(a, present, max_gap, despike)
    assert np.array_equal(cb.model_valid(a, present), R.loop_valid(a, present))
    for k in ('valid', 'spike', 'filled', 'present_r', 'repaired_per_frame'):
        assert np.array_equal(got[k], want[k]), k
    assert got['src_r'].dtype == a.dtype and got['repaired_per_frame'].dtype == np.int32
    keep = ~got['filled']
    for c in range(3):
        assert np.array_equal(got['src_r'][:, c, :][keep], a[:, c, :][keep], equal_nan=True)  # nothing else changes
    assert (got['src_r'][:, 2, :][got['filled']] == 0).all()
    for (f, k), (lo, hi) in want['anchors'].items():
        for c in (0, 1):
            g, w = got['src_r'][f, c, k], want['src_r'][f, c, k]
            if dtype == 'float64':
                bound = 8 * np.spacing(2.0 * max(abs(float(a[lo, c, k])), abs(float(a[hi, c, k]))))
            else:
                bound = float(np.spacing(np.float32(max(abs(g), abs(w)))))
            assert abs(float(g) - float(w)) <= bound, (f, k, c, g, w)
    keep_r, _ = cb.model_frame_flags(got['src_r'], got['present_r'])
    assert np.array_equal(keep_r, R.loop_keep(want['src_r'], want['present_r']))
    starts = cb.model_clip_starts(keep_r, R.VIDEOS[video]['start'], R.FRAMES)
    assert starts == R.loop_starts(keep_r, R.VIDEOS[video]['start'])
    per_clip = cb.model_repaired_per_clip(got['repaired_per_frame'], starts, R.FRAMES)
    assert per_clip.dtype == np.int32 and list(per_clip) == [int(want['repaired_per_frame'][s:s + R.FRAMES].sum()) for s in starts]


def _track(xs, ys=None, dtype='float64'):
    """one video whose keypoint 50 follows xs / ys; every other keypoint sits still at (400, 400)"""
    n = len(xs)
    a = np.full((n, 3, 137), 400.0, dtype)
    a[:, 2] = 0.5
    a[:, 0, 50] = xs
    a[:, 1, 50] = ys if ys is not None else 300.0
    return a, np.ones(n, bool)


def test_despike_by_hand():
    # x: 10 11 12 90 14 15 16, h = 1 at f = 3: window (12, 90, 14), med 14, |v - med| (2, 76, 0), mad 2: 76 > 3 * 2.9652 + 1
    a, p = _track([10, 11, 12, 90, 14, 15, 16])
    v = cb.model_valid(a, p)
    assert list(np.flatnonzero(cb.model_despike(a, v, 1, 3.0, 1.0)[:, 50])) == [3]
    # f = 2: window (11, 12, 90), med 12, deviations (1, 0, 78), mad 1: 0 is no spike; f = 4: (90, 14, 15), med 15, mad 1: 1 > 4.4478 + 1 fails
    assert not cb.model_despike(a, v, 1, 3.0, 1.0)[[2, 4], 50].any()
    # kappa so large that 76 stays below the bar: 76 > 26 * 2.9652 = 77.0952 fails
    assert not cb.model_despike(a, v, 1, 26.0, 0.0).any()
    # a jump in y only
    a, p = _track([10] * 7, [5, 5, 5, 40, 5, 5, 5])
    sp = cb.model_despike(a, cb.model_valid(a, p), 2, 3.0, 0.0)
    assert list(np.flatnonzero(sp[:, 50])) == [3] and sp.sum() == 1  # the still keypoints: mad 0, deviation 0, 0 > 0 fails
    # even m: f = 0 with h = 3 sees (10, 11, 12, 90): med 0.5 * (11 + 12) = 11.5, deviations (1.5, 0.5, 0.5, 78.5), mad 0.5 * (0.5 + 1.5) = 1
    a, p = _track([10, 11, 12, 90, 14, 15, 16])
    v = cb.model_valid(a, p)
    assert cb.model_despike(a, v, 3, 1.0, 0.0)[0, 50] and not cb.model_despike(a, v, 3, 1.0, 0.02)[0, 50]  # 1.5 > 1.4826, 1.5 > 1.5026 fails
    # m == 2 is not tested: frame 0 with h = 1 sees two points
    a, p = _track([500, 10, 10, 10, 10])
    v = cb.model_valid(a, p)
    assert not cb.model_despike(a, v, 1, 3.0, 0.0)[0, 50] and cb.model_despike(a, v, 2, 3.0, 0.0)[0, 50]
    # a jump next to a gap: frames 1 and 2 invalid, f = 3 with h = 2 sees (90, 10, 10): m = 3
    a, p = _track([10, 0, 0, 90, 10, 10, 10], [300, 0, 0, 300, 300, 300, 300])
    v = cb.model_valid(a, p)
    assert not v[1:3, 50].any() and cb.model_despike(a, v, 2, 3.0, 0.0)[3, 50]
    # mad == 0 and no floor: any deviation is a spike; a floor saves it
    a, p = _track([10, 10, 10.25, 10, 10])
    v = cb.model_valid(a, p)
    assert cb.model_despike(a, v, 2, 3.0, 0.0)[2, 50] and not cb.model_despike(a, v, 2, 3.0, 0.25)[2, 50]
    # two adjacent spikes are decided from the original map, both against (10, 10, 50, 50, 10) -> (10, 10, 10, 50, 50): med 10
    a, p = _track([10, 10, 10, 50, 50, 10, 10, 10])
    v = cb.model_valid(a, p)
    assert list(np.flatnonzero(cb.model_despike(a, v, 2, 3.0, 0.0)[:, 50])) == [3, 4]
    r = cb.model_repair(a, p, 2, (2, 3.0, 0.0))
    assert list(r['src_r'][:, 0, 50]) == [10] * 8 and list(r['src_r'][:, 2, 50]) == [0.5, 0.5, 0.5, 0, 0, 0.5, 0.5, 0.5]
    assert list(r['repaired_per_frame']) == [0, 0, 0, 1, 1, 0, 0, 0] and r['present_r'].all()
    # a spike that cannot be filled keeps its value and its confidence
    a, p = _track([10, 10, 10, 10, 70])
    r = cb.model_repair(a, p, 4, (2, 3.0, 0.0))
    assert r['spike'][4, 50] and not r['filled'].any() and np.array_equal(r['src_r'], a)
    a, p = _track([10, 10, 10, 50, 50, 10, 10, 10])  # two adjacent spikes and a max_gap of one: marked, not filled
    r = cb.model_repair(a, p, 1, (2, 3.0, 0.0))
    assert r['spike'].sum() == 2 and not r['filled'].any() and np.array_equal(r['src_r'], a)


def test_fill_by_hand():
    a, p = _track([10, 0, 0, 0, 18], [20, 0, 0, 0, 4], 'float32')
    r = cb.model_repair(a, p, 3)
    assert list(r['src_r'][:, 0, 50]) == [10, 12, 14, 16, 18] and list(r['src_r'][:, 1, 50]) == [20, 16, 12, 8, 4]
    assert list(r['src_r'][:, 2, 50]) == [0.5, 0, 0, 0, 0.5] and r['src_r'].dtype == np.float32
    assert not cb.model_repair(a, p, 2)['filled'].any()
    # x <= 3 with y > 3 is an anchor; a missing frame comes back when all 121 kept keypoints are filled
    a, p = _track([2, 7, 12], [50, 50, 50])
    p[1] = False
    a[1] = 0
    r = cb.model_repair(a, p, 1)
    assert r['present_r'].all() and r['filled'][1].all() and r['src_r'][1, 0, 50] == 7 and r['repaired_per_frame'][1] == 121
    assert list(cb.model_repaired_per_clip(r['repaired_per_frame'], [0, 1], 2)) == [121, 121]


@pytest.mark.parametrize("dtype", ['float32', 'float64'])
def test_nothing_invalid_returns_the_input_bit_for_bit(dtype):
    g = np.random.Generator(np.random.PCG64(31))
    a = g.uniform(10.0, 900.0, (40, 3, 137)).astype(dtype)
    r = cb.model_repair(a, np.ones(40, bool), 64)
    assert r['src_r'].tobytes() == a.tobytes() and r['src_r'] is not a
    assert not r['filled'].any() and not r['spike'].any() and r['valid'].all() and r['present_r'].all() and not r['repaired_per_frame'].any()


def test_build_clips_refuses_bad_repair_arguments(tmp_path):
    root = str(tmp_path)  # (the arguments are checked before any file is looked for)
    with pytest.raises(ValueError, match="despike needs repair_max_gap"):
        cb.build_clips(root, 'nobody', despike=(2, 3.0, 0.0))
    with pytest.raises(ValueError, match="despike needs repair_max_gap"):
        cb.build_clips(root, 'nobody', repair_max_gap=0, despike=(2, 3.0, 0.0))
    with pytest.raises(ValueError, match="repair_max_gap must be"):
        cb.build_clips(root, 'nobody', repair_max_gap=65)
    with pytest.raises(ValueError, match="repair_max_gap must be"):
        cb.build_clips(root, 'nobody', repair_max_gap=-1)
    with pytest.raises(ValueError, match="despike h must be"):
        cb.build_clips(root, 'nobody', repair_max_gap=4, despike=(4, 3.0, 0.0))
    with pytest.raises(ValueError, match="kappa must be positive"):
        cb.build_clips(root, 'nobody', repair_max_gap=4, despike=(2, 0.0, 0.0))
    for g in (0, 65):
        with pytest.raises(ValueError, match="repair_max_gap must be"):
            cb.model_repair(np.zeros((2, 3, 137)), np.ones(2, bool), g)
    with pytest.raises(FileNotFoundError):  # repair_max_gap = 0 is "off": the call goes on to look for the speaker
        cb.build_clips(root, 'nobody', repair_max_gap=0)
