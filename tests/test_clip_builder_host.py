"""The clip builder's numpy contract models (speechdrivestemplates_amd/clip_builder.py) against the reference's
own 2_2 / 2_3 / 3_1 / 3_2 recorded in tests/golden/clip_builder_reference.npz, bit for bit, and the resampler model against
scipy.signal.resample_poly within a derived bound.  No GPU."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import synth_keypoint_videos as S  # noqa: E402

from speechdrivestemplates_amd import clip_builder as cb  # noqa: E402

FIXTURE = os.path.join(GOLDEN, "clip_builder_reference.npz")
_Z = []
CASES = [(sp, v) for sp in ('kp_f64', 'kp_f32') for v in S.SPEAKERS[sp][1]]


def fx():
    if not _Z:
        _Z.append(np.load(FIXTURE))
    return _Z[0]


def model_video(sp, video):
    a, present = S.video_frames(video, S.SPEAKERS[sp][0])
    keep, dist = cb.model_frame_flags(a, present)
    return a, present, keep, dist


@pytest.mark.parametrize("sp,video", CASES)
def test_flags_and_starts_equal_the_reference(sp, video):
    _, _, keep, _ = model_video(sp, video)
    assert np.array_equal(keep, fx()["%s/%s/keep" % (sp, video)])
    starts = cb.model_clip_starts(keep, S.START, S.FRAMES)
    assert np.array_equal(np.array(starts, np.int64), fx()["%s/%s/starts" % (sp, video)])


@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("video", ['vidA', 'vidB'])
def test_float64_scalars_equal_the_reference_bits(video, chunks):
    _, _, keep, dist = model_video('kp_f64', video)
    means, dropped = cb.model_shoulder_means(dist[keep], chunks)
    z = fx()
    assert str(z["kp_f64/%s/means%d_dtype" % (video, chunks)]) == 'float64'
    assert np.array_equal(means, z["kp_f64/%s/means%d" % (video, chunks)])
    assert cb.model_scalar(means) == float(z["kp_f64/%s/scalar%d" % (video, chunks)])
    assert dropped == int(keep.sum()) % chunks
    if video == 'vidA':
        assert (dropped != 0) == (chunks == 3)


@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("video", ['vidA', 'vidB'])
def test_float32_scalars_are_the_float64_contract(video, chunks):
    """With float32 files the reference's recurrence follows numpy's promotion of the day (float32 under NEP 50, float64 before);
    the contract is float64 throughout.  The two differ by at most the float32 roundings of the reference's run: the distance
    (4 operations) and 3 per step of the recurrence, each 2^-24 relative to a value bounded by the largest distance."""
    _, _, keep, dist = model_video('kp_f32', video)
    means, _ = cb.model_shoulder_means(dist[keep], chunks)
    ref = fx()["kp_f32/%s/means%d" % (video, chunks)]
    stride = int(keep.sum()) // chunks
    bound = (4 + 3 * stride) * 2.0 ** -24 * dist.max()
    assert np.abs(means - ref).max() <= bound


@pytest.mark.parametrize("sp,video", CASES)
def test_audio_offsets_equal_the_reference_and_pandas(sp, video):
    import pandas as pd
    z = fx()
    cand = z["%s/%s/cand" % (sp, video)]
    assert list(cand) == list(range(S.START, S.VIDEOS[video]['n'] - S.FRAMES, S.STEP))
    times = [cb.frame_idx_to_time(int(f)) for f in cand] + [cb.frame_idx_to_time(int(f) + S.FRAMES) for f in cand]
    assert times == list(z["%s/%s/times" % (sp, video)])
    offs = [cb.audio_offsets(int(f), S.START, S.FRAMES) for f in cand]
    assert [a for a, _ in offs] == list(z["%s/%s/a0" % (sp, video)]) and [b for _, b in offs] == list(z["%s/%s/a1" % (sp, video)])
    t0 = pd.to_timedelta(cb.frame_idx_to_time(S.START))
    for f, (a0, a1) in zip(cand, offs):
        assert cb.time_to_us(cb.frame_idx_to_time(int(f))) * 1000 == pd.to_timedelta(cb.frame_idx_to_time(int(f))).value
        assert a0 == int((pd.to_timedelta(cb.frame_idx_to_time(int(f))) - t0).total_seconds() * cb.SR)
        assert a1 == int((pd.to_timedelta(cb.frame_idx_to_time(int(f) + S.FRAMES)) - t0).total_seconds() * cb.SR)


@pytest.mark.parametrize("sp", ['kp_f64', 'kp_f32'])
def test_split_rows_and_order_equal_the_reference(sp):
    z = fx()
    tables = []
    for video in S.SPEAKERS[sp][1]:
        _, _, keep, _ = model_video(sp, video)
        tables.append(cb.video_table(sp, video, cb.model_clip_starts(keep, S.START, S.FRAMES), S.FRAMES))
    val = cb.split_table(tables, 'val')
    assert list(val.columns) == list(z[sp + "/split_columns"]) == cb.COLUMNS
    assert list(val['dataset']) == list(z[sp + "/split_dataset"])
    assert list(val['interval_id']) == list(z[sp + "/split_video"]) and list(val['start']) == list(z[sp + "/split_start"])
    dev = cb.split_table(tables, 'dev')
    assert [d.replace('dev', 'val') for d in dev['dataset']] == list(val['dataset']) and list(dev['pose_fn']) == list(val['pose_fn'])
    assert not os.path.isabs(dev['pose_fn'].iloc[0])


def test_split_labels_at_sizes_with_a_validation_part():
    for n in (0, 1, 13, 14, 37, 66, 100, 1000):
        lab = cb.split_labels(n)
        k = int(n * 0.8)
        assert lab[:k] == ['train'] * k and lab[k:k + 13] == ['idle'] * min(13, n - k) and lab[k + 13:] == ['dev'] * max(0, n - k - 13)
        assert len(lab) == n


def test_scale_follows_the_reference_default_and_the_override():
    a, _, _, _ = model_video('kp_f32', 'vidB')
    s = 1.2900880565299202
    assert cb.scales_confidence(1) and not cb.scales_confidence(3) and cb.scales_confidence(3, True) and not cb.scales_confidence(1, False)
    full, xy = cb.model_scale(a, s, True), cb.model_scale(a, s, False)
    assert full.dtype == xy.dtype == np.float32
    assert np.array_equal(full, a * np.float32(s)) and np.array_equal(xy[:, :2], full[:, :2]) and np.array_equal(xy[:, 2], a[:, 2])
    a64 = a.astype(np.float64)
    assert np.array_equal(cb.model_scale(a64, s, True), a64 * s)


@pytest.mark.parametrize("sr_in,n", [(48000, 30011), (44100, 20003), (8000, 9001)])
def test_resampler_model_against_resample_poly(sr_in, n):
    """Both sum the same products taps[k] * x[i] in float64, in different orders; each sum of m terms is within (m - 1) * 2^-53 *
    sum|h| * max|x| of the exact value, far below half a float32 unit in the last place of sum|h| * max|x|.  After the one
    rounding to float32 they therefore differ by at most one such unit."""
    from scipy.signal import resample_poly
    g = np.random.Generator(np.random.PCG64(sr_in))
    x = g.uniform(-1.0, 1.0, n)
    up, down, taps, _ = cb.design_taps(sr_in)
    want = resample_poly(x, up, down).astype(np.float32)
    got = cb.model_resample(x, sr_in)
    assert got.dtype == np.float32 and got.shape == want.shape
    ulp = float(np.spacing(np.float32(np.abs(taps).sum() * np.abs(x).max())))
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= ulp


def test_16k_input_is_returned_unchanged():
    x = np.random.Generator(np.random.PCG64(5)).uniform(-1, 1, 4001).astype(np.float32)
    assert np.array_equal(cb.model_resample(x, 16000), x)


def test_pcm_model_is_the_demo_item_conversion():
    g = np.random.Generator(np.random.PCG64(6))
    st = g.integers(-32768, 32768, (1001, 2)).astype(np.int16)
    assert np.array_equal(cb.model_pcm_to_mono(st), (st.astype(np.float32) / 32768.0).mean(axis=1))
    u8 = g.integers(0, 256, 999).astype(np.uint8)
    assert np.array_equal(cb.model_pcm_to_mono(u8), (u8.astype(np.float32) - 128.0) / 128.0)
    assert cb.source_cut(80, 48000) == int(5.333333 * 48000) == 255999 and cb.source_cut(80, 44100) == int(5.333333 * 44100)  # 80 / 15 s, to the microsecond


def test_plan_lists_names_only(tmp_path):
    root = str(tmp_path)
    S.write_speaker(root, 'kp_f32')
    plan = cb.plan_clips(root, 'kp_f32')
    assert [v['video'] for v in plan] == ['vidA', 'vidB']
    assert plan[0]['n_frames'] == 251 and len(plan[0]['frames']) == 250 and 120 not in plan[0]['frames']
    assert plan[1]['wav'].endswith(os.path.join('kp_f32', 'audio_full', 'vidB.wav'))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cb.build_clips(root, 'kp_f32', device='cpu')
