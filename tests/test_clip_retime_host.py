"""The retime stage's numpy contract models (speechdrivestemplates_amd/clip_builder.py) against a rational brute
force and an independent per-point python loop (tests/golden/synth_retime_videos.py), np.interp, a sinusoid above the new Nyquist rate,
hand-built support cases, the argument checks and the sizes the C ABI refuses.  No GPU."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import synth_retime_videos as V  # noqa: E402

from speechdrivestemplates_amd import clip_builder as cb  # noqa: E402

RECORDS = ('valid_t', 'taps_used')
U = 2.0 ** -53  # the unit roundoff of float64


@pytest.mark.parametrize("p,q", V.RATES)
def test_plan_equals_the_rational_brute_force(p, q):
    for n in (1, 2, 7, 64, 257, 1000):
        plan, want = cb.model_retime_plan(n, p, q), V.loop_plan(n, p, q)
        assert plan['n_out'] == want['n_out'] and plan['phases'] == want['phases'] == cb.model_retime_taps(p, q, 'linear').shape[0]
        assert plan['a'].dtype == np.int64 and plan['phase'].dtype == np.int64 and plan['nearest_src'].dtype == np.int32
        assert list(plan['a']) == want['a'] and list(plan['phase']) == want['phase'] and list(plan['nearest_src']) == want['nearest_src']
        assert plan['a'][-1] <= n - 1 and (plan['a'][-1] + 1) * 15 * q > (plan['n_out'] - 1) * p  # the last frame is inside the video
        assert plan['n_out'] * p > (n - 1) * 15 * q  # and one more would not be
    if (p, q) in ((30, 1), (60, 1)):  # the last output frame exactly on the last source frame
        plan = cb.model_retime_plan(257, p, q)
        assert plan['a'][-1] == 256 and plan['r'][-1] == 0 and plan['nearest_src'][-1] == 256


def test_tap_tables():
    assert np.array_equal(cb.model_retime_taps(30, 1, 'smooth'), [[0.5, 1.0, 0.5, 0.0]])  # [1/4, 1/2, 1/4] once normalised
    for mode in V.MODES:
        assert np.array_equal(cb.model_retime_taps(15, 1, mode), [[1.0, 0.0]])
    assert np.array_equal(cb.model_retime_taps(25, 1, 'nearest'), [[1, 0], [1, 0], [0, 1]])  # phases 0, 1, 2: t = 0, 1/3, 2/3
    lin = cb.model_retime_taps(25, 1, 'linear')
    assert np.array_equal(lin[:, 1], [0.0, 5.0 / 15.0, 10.0 / 15.0]) and np.array_equal(lin[:, 0], 1.0 - lin[:, 1])
    assert cb.model_retime_taps(60, 1, 'smooth').shape == (1, 8) and cb.model_retime_taps(30000, 1001, 'smooth').shape == (1001, 4)
    assert cb.model_retime_taps(240, 1, 'smooth').shape == (1, 32) and cb.model_retime_taps(12, 1, 'smooth').shape == (5, 2)
    for p, q in V.RATES:
        for mode in V.MODES:
            h = cb.model_retime_taps(p, q, mode)
            for phi in (0, h.shape[0] // 2, h.shape[0] - 1):
                want = [w for _, w in V.loop_taps(p, q, mode, V.Fraction(phi, h.shape[0]))]
                assert list(h[phi]) == want, (p, q, mode, phi)
            assert (h >= 0).all() and (h.sum(axis=1) > 0).all()


CASES = [(v, p, q) for v in V.TRACKS for p, q in V.RATES if V.VIDEOS[v]['n'] < 1000 or (p, q) in ((25, 1), (30000, 1001))]


@pytest.mark.parametrize("video,p,q", CASES)
def test_model_equals_the_loop_reference_bit_for_bit(video, p, q):
    """the loop forms the same float64 operations in the same order, so nothing but equality is asked for"""
    for dtype in ('float32', 'float64'):
        a, present = V.video_frames(video, dtype)
        for mode in V.MODES:
            got = cb.model_retime(a, present, p, q, mode)
            want = V.loop_retime(a, present, p, q, mode, kps=V.loop_keypoints(video))
            k = want['kps']
            assert got['src_t'].dtype == a.dtype and got['src_t'].shape == (len(want['nearest_src']), 3, 137)
            assert got['src_t'][:, :, k].tobytes() == want['src_t'][:, :, k].tobytes(), (dtype, mode)
            for key in RECORDS:
                assert np.array_equal(got[key][:, k], want[key][:, k]), (dtype, mode, key)
            assert got['taps_used'].dtype == np.uint8 and got['nearest_src'].dtype == np.int32 and got['counts'].dtype == np.int64
            assert np.array_equal(got['present_t'], want['present_t']) and np.array_equal(got['nearest_src'], want['nearest_src'])
            assert (got['src_t'].transpose(0, 2, 1)[~got['valid_t']] == 0).all()  # an invalid point is OpenPose's (0, 0, 0)
            assert np.isfinite(got['src_t'][:, :2]).all()  # a non-finite coordinate never reaches the output
            valid_src = np.array([[V.loop_valid_point(a, present, f, kk) for kk in range(137)] for f in range(a.shape[0])])
            nonfinite = int((~np.isfinite(a[:, :2])).any(axis=1).sum())
            assert list(got['counts']) == [int((~valid_src).sum()), nonfinite, int((~got['valid_t']).sum())]
            s = cb.model_retime_summary(got, a.shape[0], p, q, mode)
            assert s == {'source_frames': a.shape[0], 'frames': got['src_t'].shape[0], 'points_invalid_in': int((~valid_src).sum()),
                         'points_invalid_out': int((~got['valid_t']).sum()), 'nonfinite_in': nonfinite, 'mode': mode, 'P': p, 'Q': q,
                         'phases': (V.Fraction(p, q) / 15).denominator}


@pytest.mark.parametrize("dtype", ['float32', 'float64'])
def test_integer_ratio_and_15_fps_properties(dtype):
    for video in ('t7', 't64', 't257'):
        a, present = V.video_frames(video, dtype)
        valid = cb.model_valid(a, present)
        for rho in (2, 4):
            for mode in ('nearest', 'linear'):
                r = cb.model_retime(a, present, 15 * rho, 1, mode)
                pick = a[::rho]
                assert r['src_t'].shape == pick.shape and np.array_equal(r['valid_t'], valid[::rho])
                m = np.repeat(valid[::rho][:, None, :], 3, axis=1)
                assert r['src_t'][m].tobytes() == pick[m].tobytes() and (r['src_t'][~m] == 0).all()
                assert np.array_equal(r['nearest_src'], np.arange(0, a.shape[0], rho))
        z = V.clean(a, present)
        for mode in V.MODES:
            for fps in ((15, 1), '15/1', 15, '30/2'):
                p, q = cb.parse_fps(fps)
                r = cb.model_retime(z, present, p, q, mode)
                assert (p, q) == (15, 1) and r['src_t'].tobytes() == z.tobytes() and r['src_t'] is not z
                assert np.array_equal(r['valid_t'], valid) and np.array_equal(r['present_t'], present)


@pytest.mark.parametrize("p,q", [r for r in V.RATES if r != (15, 1)])
def test_linear_agrees_with_np_interp(p, q):
    """On a fully valid track the model's value is ((1 - t) y0 + t y1) / ((1 - t) + t) with t = fl(r / D): t and 1 - t carry one rounding
    each (<= u, u = 2^-53), the two products and their sum three more of size <= u M each (M = max |y| around the frame), the
    denominator is 1 within 2 u and the quotient adds u M: within 8 u M + 2 u S of the exact line, S = the largest step |y[f+1] - y[f]|
    around the frame.  np.interp(j / 15, f Q / P, y) forms slope = (y1 - y0) / (x1 - x0) and slope * (x - x0) + y0 from times that carry
    one rounding each, u * time; in source frames that is u * pos for x and x0 and so 2 u pos in x - x0, 2 u (pos + 1) + u in x1 - x0:
    t is off by at most (4 pos + 8) u, which the slope turns into (4 pos + 8) u S; the quotient, the product and the sum add
    2 u S + 2 u M.  When the rounded time falls on the other side of a source frame np.interp uses the neighbouring interval, whose
    step S covers as well.  Together: u * (S * (4 pos + 12) + 10 M), pos = a_j + 1.  In float32 both float64 values are rounded once
    more and land on the same or on neighbouring float32 numbers: one float32 ulp of the larger."""
    n = 257
    g = np.random.Generator(np.random.PCG64(5))
    y64 = 500.0 + 60.0 * np.sin(np.arange(n)[:, None] * g.uniform(0.02, 0.3, 137)[None]) + g.normal(0.0, 2.0, (n, 137))
    for dtype in ('float64', 'float32'):
        a = np.full((n, 3, 137), 400.0, dtype)
        a[:, 0, :] = y64
        y = a[:, 0, :].astype(np.float64)
        r = cb.model_retime(a, np.ones(n, bool), p, q, 'linear')
        plan = cb.model_retime_plan(n, p, q)
        assert r['valid_t'].all()
        x = np.arange(plan['n_out'], dtype=np.float64) / 15.0
        xp = (np.arange(n, dtype=np.float64) * q) / p
        step = np.abs(np.diff(y, axis=0))
        for k in range(0, 137, 17):
            want = np.interp(x, xp, y[:, k])
            got = r['src_t'][:, 0, k]
            for j in range(plan['n_out']):
                f = int(plan['a'][j])
                lo, hi = max(f - 1, 0), min(f + 2, n)
                big = np.abs(y[lo:hi, k]).max()
                s = step[lo:hi - 1, k].max() if hi - 1 > lo else 0.0
                if dtype == 'float64':
                    bound = U * (s * (4 * (f + 1) + 12) + 10 * big)
                    assert abs(got[j] - want[j]) <= bound, (k, j, got[j], want[j], bound)
                else:
                    w32 = np.float32(want[j])
                    assert abs(float(got[j]) - float(w32)) <= float(np.spacing(np.float32(max(abs(got[j]), abs(w32))))), (k, j, got[j], w32)


def test_aliasing_at_30_fps():
    """a 10 Hz sinusoid sampled at 30 fps: every second frame is a 5 Hz sinusoid of the same amplitude (the alias); [1/4, 1/2, 1/4] scales
    it by 0.5 + 0.5 cos(2 pi 10 / 30) = 0.25"""
    n, amp, mid = 241, 40.0, 500.0
    a = np.full((n, 3, 137), 400.0)
    a[:, 0, 50] = mid + amp * np.sin(2.0 * np.pi * 10.0 * np.arange(n) / 30.0 + 0.3)
    present = np.ones(n, bool)
    j = np.arange((n - 1) // 2 + 1)
    basis = np.stack([np.sin(2.0 * np.pi * 5.0 * j / 15.0), np.cos(2.0 * np.pi * 5.0 * j / 15.0)], axis=1)

    def amplitude(v):  # of the 5 Hz component at 15 fps, by least squares over the interior frames
        coef, res, _, _ = np.linalg.lstsq(basis[1:-1], v[1:-1] - mid, rcond=None)
        assert res.size == 0 or res[0] <= (1e-12 * amp) ** 2 * len(v)  # nothing but that component
        return float(np.hypot(*coef))
    near = cb.model_retime(a, present, 30, 1, 'nearest')['src_t'][:, 0, 50]
    smooth = cb.model_retime(a, present, 30, 1, 'smooth')['src_t'][:, 0, 50]
    assert np.array_equal(near, a[::2, 0, 50])
    assert abs(amplitude(near) - amp) <= 1e-12 * amp
    assert 0.5 + 0.5 * np.cos(2.0 * np.pi * 10.0 / 30.0) == pytest.approx(0.25, abs=1e-15)
    assert abs(amplitude(smooth) - 0.25 * amp) <= 1e-12 * (0.25 * amp)


def _track(xs, present=None):
    """one video whose keypoint 50 has x = xs (0 = OpenPose's dropout, with y and confidence 0); the others sit still at (400, 400)"""
    n = len(xs)
    a = np.full((n, 3, 137), 400.0)
    a[:, 2] = 0.5
    a[:, 0, 50] = xs
    a[:, 1, 50] = np.where(np.asarray(xs) == 0, 0.0, 300.0)
    a[:, 2, 50] = np.where(np.asarray(xs) == 0, 0.0, 0.5)
    return a, np.ones(n, bool) if present is None else np.asarray(present, bool)


def test_support_rule_by_hand():
    # smooth at 30 -> 15 fps: weights (1/2, 1, 1/2) on frames 2j-1, 2j, 2j+1, full = 2, default bar 0.75 * 2 = 1.5
    a, p = _track([10, 12, 14, 0, 18, 20, 22, 24, 0, 28, 30])
    r = cb.model_retime(a, p, 30, 1, 'smooth')
    x, v, used = r['src_t'][:, 0, 50], r['valid_t'][:, 50], r['taps_used'][:, 50]
    assert list(v) == [True, True, True, True, False, True] and list(used) == [2, 2, 2, 3, 2, 2]
    assert x[1] == (0.5 * 12 + 14) / 1.5  # frame 3, a flank of output 1, is lost: den = 1.5 >= 1.5, the point stays
    assert x[2] == (18 + 0.5 * 20) / 1.5 and x[3] == (0.5 * 20 + 22 + 0.5 * 24) / 2.0
    assert x[4] == 0 and (r['src_t'][4, :, 50] == 0).all()  # frame 8, the centre of output 4, is lost: den = 1 < 1.5
    assert x[0] == (10 + 0.5 * 12) / 1.5 and x[5] == (0.5 * 28 + 30) / 1.5  # the two ends of the video: frame -1 and frame 11 do not exist
    assert r['src_t'][1, 1, 50] == 300.0 and r['src_t'][1, 2, 50] == 0.5 and r['present_t'].all()
    strict = cb.model_retime(a, p, 30, 1, 'smooth', min_support=1.0)
    assert list(strict['valid_t'][:, 50]) == [False, False, False, True, False, False] and strict['valid_t'][0, 49] == 0 and strict['valid_t'][3].all()
    loose = cb.model_retime(a, p, 30, 1, 'smooth', min_support=0.5)
    assert loose['valid_t'][:, 50].all() and loose['src_t'][4, 0, 50] == (0.5 * 24 + 0.5 * 28) / 1.0
    # linear at 24 -> 15 fps: t = 0, .6, .2, .8, .4 on source frames 0, 1, 3, 4, 6: next to a dropout a point survives only within a
    # quarter frame of its valid neighbour
    a, p = _track([10, 0, 14, 16, 0, 32, 22, 24, 26])  # (16 and 32: h * x / h is exact for a power of two)
    r = cb.model_retime(a, p, 24, 1, 'linear')
    assert list(cb.model_retime_plan(9, 24, 1)['a']) == [0, 1, 3, 4, 6, 8]
    # output 1: frames (1, 2) at t = .6, frame 1 lost: den = .6 < .75; output 2: frames (3, 4) at t = .2, frame 4 lost: den = .8
    # output 3: frames (4, 5) at t = .8, frame 4 lost: den = .8; output 4: frames (6, 7), both there
    assert list(r['valid_t'][:, 50]) == [True, False, True, True, True, True]
    assert r['src_t'][2, 0, 50] == 16.0 and r['src_t'][3, 0, 50] == 32.0 and list(r['taps_used'][:, 50]) == [1, 1, 1, 1, 2, 1]
    # a missing file is a dropout of every keypoint, and present_t follows the non-zero taps
    a, p = _track([10, 12, 14, 16, 18], [1, 1, 0, 1, 1])
    a[2] = 0
    r = cb.model_retime(a, p, 30, 1, 'linear')
    assert list(r['present_t']) == [True, False, True] and not r['valid_t'][1].any() and (r['src_t'][1] == 0).all()
    assert list(cb.model_retime(a, p, 30, 1, 'smooth')['present_t']) == [True, True, True]
    # a NaN is invalid, counted, and does not reach the output
    a, p = _track([10, 12, 14, 16, 18])
    a[2, 0, 50] = np.nan
    r = cb.model_retime(a, p, 30, 1, 'smooth')
    assert list(r['counts']) == [1, 1, 1] and np.isfinite(r['src_t']).all() and not r['valid_t'][1, 50]


def test_arguments_are_checked_and_named(tmp_path):
    assert cb.parse_fps('30000/1001') == (30000, 1001) and cb.parse_fps(25) == (25, 1) and cb.parse_fps((60, 2)) == (30, 1)
    assert cb.parse_fps(' 2997/100 ') == (2997, 100) and cb.parse_fps(np.int64(30)) == (30, 1)
    for bad in (29.97, np.float32(30.0), 30.0):
        with pytest.raises(ValueError, match=r"fps must be an exact fraction.*'30000/1001'"):
            cb.parse_fps(bad)
    for bad in ('30000/1001/2', 'ntsc', '-30', '30/0', (30,), (30.0, 1), None, 0, (0, 1), 241, '14/15', (1 << 20) + 1, '1048577/65537', '16385/16384'):
        with pytest.raises(ValueError, match="fps"):
            cb.parse_fps(bad)
    with pytest.raises(ValueError, match="source_fps must be an exact fraction"):
        cb.parse_fps(29.97, 'source_fps')
    a = np.zeros((4, 3, 137))
    with pytest.raises(ValueError, match="mode must be one of"):
        cb.model_retime(a, np.ones(4, bool), 30, 1, 'cubic')
    for s in (0.0, -0.5, 1.5, float('nan'), None):
        with pytest.raises(ValueError, match="min_support must lie in"):
            cb.model_retime(a, np.ones(4, bool), 30, 1, 'linear', s)
    with pytest.raises(ValueError, match="n_src"):
        cb.model_retime_plan(0, 30, 1)
    root = str(tmp_path)  # (the arguments are checked before any file is looked for)
    with pytest.raises(ValueError, match="source_fps must be an exact fraction"):
        cb.build_clips(root, 'nobody', source_fps=29.97)
    with pytest.raises(ValueError, match="source_fps"):
        cb.build_clips(root, 'nobody', source_fps='241')
    with pytest.raises(ValueError, match="retime must be one of"):
        cb.build_clips(root, 'nobody', source_fps=30, retime='cubic')
    with pytest.raises(ValueError, match="retime_min_support must lie in"):
        cb.build_clips(root, 'nobody', source_fps=30, retime_min_support=0.0)
    with pytest.raises(FileNotFoundError):  # valid arguments: the call goes on to look for the speaker
        cb.build_clips(root, 'nobody', source_fps='30000/1001', retime='smooth', retime_min_support=1.0)
    with pytest.raises(FileNotFoundError):
        cb.build_clips(root, 'nobody')


def test_frame_image_paths_name_the_nearest_source_frames():
    near = cb.model_retime_plan(9, 24, 1)['nearest_src']
    assert list(near) == [0, 2, 3, 5, 6, 8]
    got = cb.frame_image_paths('R', 'S', 'v', 1, 3, near)
    assert [p.split('_')[-1] for p in got] == ['000002.jpg', '000003.jpg', '000005.jpg']
    assert list(cb.frame_image_paths('R', 'S', 'v', 1, 3)) == list(cb.frame_image_paths('R', 'S', 'v', 1, 3, None))


def test_c_abi_refuses_unsupported_sizes_before_any_launch():
    """outside 1 <= P <= 2^20, 1 <= Q <= 2^16, 1 <= P / Q <= 240, phases <= 16384, an even L in [2, 32], 1 <= n_src, n_out <= 2^30 and
    min_support in (0, 1] the workspace query is negative and the entry point returns SDT_ERR_UNSUPPORTED"""
    import ctypes as C

    from speechdrivestemplates_amd import _lib
    lib = _lib.load()
    ws = lib.sdt_clip_retime_workspace_bytes
    # 1000 frames at 30 fps: 500 output frames in blocks of 16, 137000 source points in blocks of 256, two counts each
    assert ws(1000, 30, 1, 1, 2) == (32 + 2 * 536) * 4 and ws(1000, 30000, 1001, 1001, 4) > 0 and ws(1, 240, 1, 1, 32) > 0
    assert ws(1 << 30, 15, 1, 1, 2) > 0 and ws(1000, 1 << 20, 1 << 16, 15, 2) > 0
    bad = [(0, 30, 1, 1, 2), ((1 << 30) + 1, 30, 1, 1, 2), (1000, 0, 1, 1, 2), (1000, (1 << 20) + 1, 65536, 1, 2), (1000, 30, 0, 1, 2),
           (1000, 1 << 20, (1 << 16) + 1, 1, 2), (1000, 14, 15, 225, 2), (1000, 241, 1, 15, 2), (1000, 30, 1, 2, 2), (1000, 30, 1, 1, 0),
           (1000, 30, 1, 1, 3), (1000, 30, 1, 1, 34), (1000, 16385, 16384, 16384 * 15, 2), (1 << 30, 12, 1, 5, 2)]
    for args in bad:
        assert ws(*args) < 0, args
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)

    def call(n_src=1000, fp=30, fq=1, phases=1, taps=2, support=0.75, n_out=500, ws_bytes=1 << 20):
        return lib.sdt_clip_retime(8, p, p, n_src, fp, fq, p, phases, taps, support, n_out, None, p, p, p, p, p, p, ws_bytes, None)
    for args in bad:
        assert call(*args) == -3, args
    for s in (0.0, -1.0, 1.0000001, float('nan')):
        assert call(support=s) == -3, s
        assert b"min_support" in lib.sdt_last_error()
    assert call() == -1  # supported sizes, a null src_t: an argument error, still before any launch
    assert b"sdt_clip_retime" in lib.sdt_last_error()
    with pytest.raises(ValueError, match="unsupported size"):
        cb._check_size(call(n_src=0))
