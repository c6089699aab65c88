"""The audio activity gate's numpy contract models (speechdrivestemplates_amd/clip_builder.py) against plain-loop
restatements (tests/golden/synth_speech_gate.py) and hand-written cases, the parameter checks and the command line.  No GPU."""
import argparse
import inspect
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import synth_speech_gate as S  # noqa: E402

from speechdrivestemplates_amd import clip_builder as cb  # noqa: E402

FULL = {'min_permille': 500, 'margin_db': 12.0, 'floor_pct': 10, 'abs_dbfs': -60.0, 'hang_hops': 20, 'min_run_hops': 5}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------------ energies
@pytest.mark.parametrize("n", [0, 159, 160, 161, 319, 320, 160 * 5 + 7])
def test_hop_energy_equals_the_lane_by_lane_loop(n):
    x = S.track(n)
    e = cb.model_hop_energy(x)
    assert e.dtype == np.float64 and e.shape == (n // 160,)
    assert np.array_equal(bits(e), bits(S.loop_hop_energy(x)))


def test_hop_energy_order_matters_and_is_the_stated_one():
    """the lane order is part of the contract: on these samples a plain left-to-right sum gives other bits"""
    x = S.track(160 * 5 + 7)
    e = cb.model_hop_energy(x)
    x64 = x.astype(np.float64)
    d = x64 - (31.0 / 32.0) * np.concatenate([[0.0], x64[:-1]])
    serial = np.array([sum(float(v) * float(v) for v in d[160 * h:160 * (h + 1)]) for h in range(5)])
    assert np.allclose(e, serial, rtol=1e-13) and not np.array_equal(bits(e), bits(serial))
    assert d[0] == x64[0] and np.signbit(d[0])  # x[-1] = 0: -0.0 - 0.0 stays -0.0


def test_hop_energy_of_zeros_and_subnormals():
    x = S.track(320)
    e = cb.model_hop_energy(x)
    leak = 31.0 / 32.0 * float(x[159])
    assert e[0] > 1.0 and e[1] == leak * leak  # hop 1 holds its neighbour's last sample through x[n-1], and
    quiet = cb.model_hop_energy(x[160:])                                # 80 squares of about 1e-83 that vanish beside it
    assert 0 < quiet[0] < 1e-80  # alone, the hop of signed zeros and float32 subnormals is kept in float64, not flushed
    assert np.array_equal(bits(cb.model_hop_energy(np.zeros(160, np.float32) * np.float32(-1))), bits(np.zeros(1)))  # +0.0


def test_non_finite_samples_stay_inside_their_hop():
    x = S.track(160 * 4)
    clean = cb.model_hop_energy(x)
    x[160 + 50], x[160 + 90] = np.nan, np.inf
    e = cb.model_hop_energy(x)
    assert not np.isfinite(e[1]) and np.array_equal(bits(e[[0, 2, 3]]), bits(clean[[0, 2, 3]]))
    with pytest.raises(ValueError, match='non-finite'):
        cb.model_speech_gate(x, [80], 80, 64, FULL)


# --------------------------------------------------------------------------------------------------------------- floor and threshold
@pytest.mark.parametrize("h", [1, 2, 101])
@pytest.mark.parametrize("pct", [0, 10, 50])
def test_floor_rank(h, pct):
    for kind in ('random', 'ties', 'equal'):
        e = S.energies(h, kind)
        f = cb.model_floor(e, pct)
        assert bits(f) == bits(S.loop_floor(e, pct)) and f == np.sort(e)[(pct * (h - 1)) // 100]
    e = S.energies(h, 'random')
    assert cb.model_floor(e, 0) == e.min()
    if h == 101:
        assert cb.model_floor(e, 50) == np.sort(e)[50] and cb.model_floor(e, 10) == np.sort(e)[10]
    if h == 2:
        assert cb.model_floor(e, 50) == e.min()  # (50 * 1) // 100 = 0


def test_floor_without_hops():
    assert cb.model_floor(np.zeros(0), 10) is None
    g = cb.model_speech_gate(np.zeros(159, np.float32), [80, 85], 80, 64, FULL)
    assert len(g['energy']) == 0 and not g['kept'].any() and g['summary']['hops'] == 0 and g['summary']['kept'] == 0
    assert g['summary']['floor_db'] is None and g['summary']['thr_db'] is None


def test_threshold_either_side():
    e = np.array([1e-9, 2e-3, 5e-3, 0.1, 0.1 * (1 + 2 ** -52)])
    margin, abs_floor = cb.gate_constants(cb.speech_gate_params(FULL))
    assert margin == 10 ** 1.2 and abs_floor == 160 * 10 ** -6.0
    raw, thr = cb.model_mask(e, 1e-9, margin, abs_floor)  # the absolute floor wins
    assert thr == abs_floor and raw.tolist() == [False, True, True, True, True]
    raw, thr = cb.model_mask(e, 2e-3, margin, abs_floor)  # floor * margin wins: one rounded product
    assert thr == 2e-3 * margin > abs_floor and raw.tolist() == [False, False, False, True, True]
    raw, thr = cb.model_mask(e, 0.1 / margin, 10 ** 1.2, 0.0)
    assert raw.tolist() == (e > thr).tolist() and not raw[:3].any()  # strictly greater, at the last bit
    raw, thr = cb.model_mask(np.array([0.1, np.nextafter(0.1, 1)]), 0.1, 1.0, 0.0)
    assert thr == 0.1 and raw.tolist() == [False, True]


# ------------------------------------------------------------------------------------------------------------------------ smoothing
def rl(text):
    return np.array([c == '1' for c in text.replace(' ', '')], bool)


def test_smoothing_by_hand():
    m = rl('0 111 00 11 000 1 0')
    assert cb.model_smooth(m, 3, 0).tolist() == rl('0 111 00 00 000 0 0').tolist()  # runs of min_run - 1 and less go, min_run stays
    assert cb.model_smooth(m, 2, 0).tolist() == rl('0 111 00 11 000 0 0').tolist()
    assert cb.model_smooth(m, 0, 2).tolist() == rl('0 111 11 11 000 1 0').tolist()  # a gap of hang is filled, hang + 1 is not
    assert cb.model_smooth(m, 0, 3).tolist() == rl('0 111 11 11 111 1 0').tolist()  # and the gaps at the two ends never are
    assert cb.model_smooth(m, 0, 0).tolist() == m.tolist() and cb.model_smooth(m, 1, 0).tolist() == m.tolist()
    assert cb.model_smooth(m, 2, 3).tolist() == rl('0 111 11 11 000 0 0').tolist()  # open, then close: the lone hop is gone before
    closed_first = cb.model_smooth(cb.model_smooth(m, 0, 3), 2, 0)                  # the closing could have bridged to it
    assert closed_first.tolist() == rl('0 111 11 11 111 1 0').tolist() != cb.model_smooth(m, 2, 3).tolist()
    ends = rl('11 000 1111 00 1')
    assert cb.model_smooth(ends, 3, 5).tolist() == rl('00 000 1111 00 0').tolist()  # short runs at both ends go; end gaps stay open
    assert cb.model_smooth(ends, 0, 5).tolist() == rl('11 111 1111 11 1').tolist()
    for h in (0, 1):
        for v in (False, True):
            m1 = np.full(h, v, bool)
            assert cb.model_smooth(m1, 0, 1024).tolist() == m1.tolist() and cb.model_smooth(m1, 2, 0).tolist() == [False] * h


@pytest.mark.parametrize("min_run,hang", [(0, 0), (1, 1), (2, 2), (5, 20), (3, 7), (7, 3), (0, 4), (4, 0), (1024, 1024)])
def test_smoothing_equals_the_serial_walk(min_run, hang):
    pats = [S.smoothing_pattern(max(min_run, 2), max(hang, 2)), S.smoothing_pattern(5, 20), ~S.smoothing_pattern(3, 4)]
    g = np.random.Generator(np.random.PCG64(min_run * 2000 + hang))
    pats += [g.random(n) < p for n in (1, 2, 64, 65, 300) for p in (0.2, 0.5, 0.9)]
    for m in pats:
        got = cb.model_smooth(m, min_run, hang)
        assert got.dtype == bool and got.tolist() == S.loop_smooth(m, min_run, hang).tolist(), (min_run, hang, len(m))


def test_the_pattern_holds_every_case():
    for mr, hg in ((2, 2), (5, 20), (3, 7)):
        m = S.smoothing_pattern(mr, hg)
        r = S.runs(m)
        on = {n for v, _, n in r if v}
        off = {n for v, f, n in r if not v and f > 0 and f + n < len(m)}
        assert {mr - 1, mr, mr + 1} <= on and {hg, hg + 1} <= off and m[-1] and not m[0]
        assert cb.model_smooth(m, mr, hg).tolist() != cb.model_smooth(cb.model_smooth(m, 0, hg), mr, 0).tolist()  # the order matters


# -------------------------------------------------------------------------------------------------------------------------- windows
def test_window_counts_and_the_keep_rule():
    g = np.random.Generator(np.random.PCG64(5))
    active = g.random(40) < 0.5
    n = 40 * 160 + 77
    offs = [(0, 1600), (1, 1600), (159, 1599), (160, 1600), (161, 1761), (3000, 3100), (3040, 3200), (6000, 9000), (6400, 7000), (6477, 9000),
            (n, n + 500), (0, n), (320, 320), (500, 400)]
    got = cb.model_window_counts(active, n, offs)
    assert got.dtype == np.int32 and np.array_equal(got, S.loop_window_counts(active, n, offs))
    assert got[1].tolist() == [active[1:10].sum(), 9]     # starts mid-hop: the cut hop is not inside
    assert got[2].tolist() == [active[1:9].sum(), 8]      # and ends mid-hop
    assert got[5].tolist() == [0, 0] and got[6].tolist() == [active[19], 1]  # a span inside one hop; exactly one hop
    assert got[7].tolist() == [active[38:40].sum(), 2]    # ends past N: clipped to N, the ignored tail is no hop
    assert got[9].tolist() == [0, 0] and got[10].tolist() == [0, 0] and got[12].tolist() == [0, 0] and got[13].tolist() == [0, 0]
    assert got[11].tolist() == [active.sum(), 40]
    counts = np.array([[1, 2], [213, 426], [212, 426], [214, 427], [213, 427], [0, 0], [0, 5], [5, 5], [1, 1000], [0, 1000], [999, 1000]], np.int32)
    assert cb.model_windows_kept(counts, 500).tolist() == [True, True, False, True, False, False, False, True, False, False, True]
    assert cb.model_windows_kept(counts, 1).tolist() == [True, True, True, True, True, False, False, True, True, False, True]
    assert cb.model_windows_kept(counts, 1000).tolist() == [False] * 7 + [True] + [False] * 3
    big = np.array([[2 ** 24, 2 ** 24], [2 ** 24 - 1, 2 ** 24]], np.int32)  # 1000 c does not fit int32: the rule is evaluated in int64
    assert cb.model_windows_kept(big, 1000).tolist() == [True, False]


def test_model_speech_gate_on_the_synthetic_speaker():
    """the end-to-end track really holds what the GPU test relies on"""
    seen = set()
    for video in S.VIDEOS:
        import synth_keypoint_videos as K
        rate, pcm = S.video_audio(video)
        x = cb.model_pcm_to_mono(pcm)[cb.source_cut(K.START, rate):]
        a, present = K.video_frames(video, 'float32')
        keep, _ = cb.model_frame_flags(a, present)
        starts = cb.model_clip_starts(keep, K.START, K.FRAMES)
        g = cb.model_speech_gate(x, starts, K.START, K.FRAMES, S.GATE)
        plan = S.hop_plan(video, len(g['energy']))
        assert g['active_raw'].tolist() == plan.tolist() == g['active'].tolist()
        c, nh = g['counts_all'][:, 0].astype(np.int64), g['counts_all'][:, 1].astype(np.int64)
        seen |= {'boundary'} if ((1000 * c == 500 * nh) & (nh > 0)).any() else set()
        seen |= {'just below'} if ((1000 * c < 500 * nh) & (1000 * (c + 1) >= 500 * nh)).any() else set()
        seen |= {'clipped'} if any(a1 > len(x) > a0 for a0, a1 in g['offsets']) else set()
        seen |= {'mostly silent'} if ((4 * c < nh) & (nh > 0)).any() else set()
        seen |= {'loud'} if (c == nh).any() else set()
        assert 0 < g['kept'].sum() < len(starts) and g['summary']['clips'] == 'clips %d -> %d' % (len(starts), g['kept'].sum())
        assert np.array_equal(g['starts'], np.sort(g['starts'])) and g['counts'].shape == (g['kept'].sum(), 2)
    assert seen == {'boundary', 'just below', 'clipped', 'mostly silent', 'loud'}


def test_summary_notes_a_track_that_is_all_or_nothing():
    s = cb.speech_gate_summary(1000, 40, 40, 1e-6, 1e-4, 10, 0)
    assert 'floor may lie inside the speech' in s['note'] and s['floor_db'] == pytest.approx(-60.0) and s['thr_db'] == pytest.approx(-40.0)
    assert 'next to nothing' in cb.speech_gate_summary(1000, 990, 990, 1e-6, 1e-4, 10, 10)['note']
    assert cb.speech_gate_summary(1000, 500, 500, 0.0, 1e-4, 10, 5)['note'] is None
    assert cb.speech_gate_summary(1000, 500, 500, 0.0, 1e-4, 10, 5)['floor_db'] == float('-inf')


# ----------------------------------------------------------------------------------------------------------------------- parameters
def test_parameters_accepted():
    assert cb.speech_gate_params(FULL) == FULL
    assert cb.speech_gate_params({'min_permille': 1}) == dict(cb.GATE_DEFAULTS, min_permille=1)
    edge = {'min_permille': 1000, 'margin_db': 60, 'floor_pct': 50, 'abs_dbfs': -120, 'hang_hops': 1024, 'min_run_hops': 0}
    p = cb.speech_gate_params(edge)
    assert p == edge and isinstance(p['margin_db'], float) and isinstance(p['hang_hops'], int)
    assert cb.speech_gate_params(dict(FULL, margin_db=0, abs_dbfs=0.0, floor_pct=np.int64(0), hang_hops=20.0))['hang_hops'] == 20


@pytest.mark.parametrize("key,value", [
    ('min_permille', 0), ('min_permille', 1001), ('min_permille', 500.5), ('min_permille', True), ('min_permille', '500'), ('min_permille', None),
    ('margin_db', -0.1), ('margin_db', 60.1), ('margin_db', float('nan')), ('margin_db', float('inf')), ('margin_db', '12'),
    ('floor_pct', -1), ('floor_pct', 51), ('floor_pct', 10.5), ('floor_pct', float('nan')),
    ('abs_dbfs', -120.1), ('abs_dbfs', 0.1), ('abs_dbfs', float('-inf')), ('abs_dbfs', float('nan')),
    ('hang_hops', -1), ('hang_hops', 1025), ('hang_hops', 2.5), ('min_run_hops', -1), ('min_run_hops', 1025), ('min_run_hops', False)])
def test_parameters_rejected(key, value):
    with pytest.raises(ValueError, match=key):
        cb.speech_gate_params(dict(FULL, **{key: value}))


def test_parameter_sets_rejected():
    with pytest.raises(ValueError, match='min_permille'):
        cb.speech_gate_params({'margin_db': 12.0})
    with pytest.raises(ValueError, match='hang_ms'):
        cb.speech_gate_params(dict(FULL, hang_ms=200))
    for bad in (500, [500], 'on', True):
        with pytest.raises(ValueError, match='speech_gate'):
            cb.speech_gate_params(bad)


def test_ms_arguments():
    assert cb.gate_ms_to_hops(0, '--gate-min-ms') == 0 and cb.gate_ms_to_hops(200, '--gate-hang-ms') == 20
    for bad in (5, 15, 199, -10, 10.5, float('nan'), True):
        with pytest.raises(ValueError, match='--gate-hang-ms'):
            cb.gate_ms_to_hops(bad, '--gate-hang-ms')
    with pytest.raises(ValueError, match='--gate-min-ms'):
        cb.gate_ms_to_hops(55, '--gate-min-ms')


# --------------------------------------------------------------------------------------------------------------------- command line
def parser():
    ap = argparse.ArgumentParser()
    cb.add_repair_options(ap)
    cb.add_retime_options(ap)
    cb.add_speech_gate_options(ap)
    return ap


def test_command_line():
    ap = parser()
    assert cb.speech_gate_option(ap.parse_args([])) is None
    assert cb.speech_gate_option(ap.parse_args(['--gate-margin-db', '6'])) is None  # the gate is off without --speech-gate
    assert cb.speech_gate_option(ap.parse_args(['--speech-gate', '500'])) == FULL
    a = ap.parse_args(['--speech-gate', '250', '--gate-margin-db', '9.5', '--gate-floor-pct', '20', '--gate-abs-dbfs', '-50', '--gate-hang-ms', '300',
                       '--gate-min-ms', '0'])
    assert cb.speech_gate_option(a) == {'min_permille': 250, 'margin_db': 9.5, 'floor_pct': 20, 'abs_dbfs': -50.0, 'hang_hops': 30, 'min_run_hops': 0}
    with pytest.raises(ValueError, match='--gate-hang-ms'):
        cb.speech_gate_option(ap.parse_args(['--speech-gate', '500', '--gate-hang-ms', '205']))
    with pytest.raises(ValueError, match='--gate-min-ms'):
        cb.speech_gate_option(ap.parse_args(['--speech-gate', '500', '--gate-min-ms', '7']))
    with pytest.raises(ValueError, match='min_permille'):
        cb.speech_gate_option(ap.parse_args(['--speech-gate', '0']))
    with pytest.raises(ValueError, match='hang_hops'):
        cb.speech_gate_option(ap.parse_args(['--speech-gate', '500', '--gate-hang-ms', '10250']))


def test_main_reports_a_bad_option_as_a_usage_error(capsys):
    for argv, word in ((['--root', 'r', '--speaker', 's', '--speech-gate', '500', '--gate-min-ms', '7'], '--gate-min-ms'),
                       (['--speech-gate', '500'], '--root')):
        with pytest.raises(SystemExit) as e:
            cb.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_the_option_is_off_by_default_and_changes_no_format():
    sig = inspect.signature(cb.build_clips)
    assert sig.parameters['speech_gate'].default is None and list(sig.parameters)[-1] == 'speech_gate'
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == {
        'start_frame': 80, 'num_frames': 64, 'shoulder_chunks': 1, 'scale_confidence': None, 'write': True, 'device': 'cuda', 'repair_max_gap': 0,
        'despike': None, 'source_fps': None, 'retime': 'linear', 'retime_min_support': 0.75, 'speech_gate': None}
    assert cb.COLUMNS == ['dataset', 'start', 'end', 'interval_id', 'pose_fn', 'audio_fn', 'video_fn', 'speaker']
    with pytest.raises(ValueError, match='min_permille'):  # checked before anything is read or launched
        cb.build_clips('/nonexistent', 's', speech_gate={'min_permille': 0})
