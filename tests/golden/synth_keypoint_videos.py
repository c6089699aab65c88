"""Seeded synthetic per-frame keypoints and wav tracks for the clip builder (speechdrivestemplates_amd/clip_builder.py): the tests
and make_clip_builder_reference.py regenerate them from the seeds below.  ``check()`` asserts that every edge case the tests rely
on really occurs in the generated data."""
import os

import numpy as np
from scipy.io import wavfile

KEPT = [0] + list(range(2, 8)) + [15, 16] + list(range(25, 137))
UNUSED = [1] + list(range(8, 15)) + list(range(17, 25))
START, FRAMES, STEP = 80, 64, 5

# video -> frames, seed, outlier frames (zeros at a kept keypoint), missing files, audio (rate, dtype, channels, seconds)
VIDEOS = {
    'vidA': dict(n=251, seed=11, outliers=[0, 250], missing=[120], x_eq_3=100, x_low_y_high=101, unused_zero=102,
                 audio=(48000, 'int16', 2, 16.7)),
    'vidB': dict(n=260, seed=12, outliers=[], missing=[], audio=(44100, 'uint8', 1, 12.0)),   # audio shorter than the video (17.3 s)
    'vidC': dict(n=100, seed=13, outliers=[], missing=[], audio=(8000, 'float32', 1, 6.7)),   # shorter than START + FRAMES
    'vidD': dict(n=256, seed=14, outliers=list(range(0, 256, 60)), missing=[], audio=(16000, 'int16', 1, 17.0)),
}
SPEAKERS = {'kp_f64': ('float64', ['vidA', 'vidB']), 'kp_f32': ('float32', ['vidA', 'vidB']),
            'kp_empty_f64': ('float64', ['vidC', 'vidD']), 'kp_empty_f32': ('float32', ['vidC', 'vidD'])}


def video_frames(name, dtype):
    """-> (frames (n, 3, 137) in dtype, present (n,) bool)"""
    v = VIDEOS[name]
    g = np.random.Generator(np.random.PCG64(v['seed']))
    base = g.uniform(200.0, 900.0, (2, 137))
    base[0, 2], base[0, 5] = 400.0, 640.0  # the shoulders
    xy = base[None] + g.normal(0.0, 6.0, (v['n'], 2, 137))
    a = np.concatenate([xy, g.uniform(0.1, 1.0, (v['n'], 1, 137))], axis=1)
    for f in v['outliers']:
        a[f, :2, 30] = 0.0
    if 'x_eq_3' in v:
        a[v['x_eq_3'], 0, 4], a[v['x_eq_3'], 1, 4] = 3.0, 2.0          # x == 3 exactly, y <= 3: dropped
        a[v['x_low_y_high'], 0, 4], a[v['x_low_y_high'], 1, 4] = 2.0, 50.0  # x <= 3, y > 3: kept
        a[v['unused_zero'], :2, :][:, UNUSED] = 0.0                     # zeros at the keypoints 2_2 ignores: kept
    present = np.ones(v['n'], bool)
    present[v['missing']] = False
    return a.astype(dtype), present


def video_audio(name):
    """-> (rate, samples as wavfile.write takes them)"""
    rate, dtype, ch, sec = VIDEOS[name]['audio']
    g = np.random.Generator(np.random.PCG64(1000 + VIDEOS[name]['seed']))
    n = int(rate * sec)
    x = g.uniform(-0.9, 0.9, (n, ch) if ch > 1 else (n,))
    if dtype == 'int16':
        return rate, np.round(x * 32767).astype(np.int16)
    if dtype == 'uint8':
        return rate, np.round(x * 127 + 128).astype(np.uint8)
    return rate, x.astype(np.float32)


def write_speaker(root, speaker):
    dtype, videos = SPEAKERS[speaker]
    base = os.path.join(root, speaker)
    os.makedirs(os.path.join(base, 'audio_full'), exist_ok=True)
    for name in videos:
        d = os.path.join(base, 'tmp', 'raw_pose_2d', name)
        os.makedirs(d, exist_ok=True)
        a, present = video_frames(name, dtype)
        for f in np.flatnonzero(present):
            np.save(os.path.join(d, '%s_%06d.npy' % (name, f)), a[f])
        rate, x = video_audio(name)
        wavfile.write(os.path.join(base, 'audio_full', name + '.wav'), rate, x)
    return base


def outlier(frame):
    p = frame[:2][:, KEPT]
    return bool(((p[0] <= 3) & (p[1] <= 3)).any())


def check():
    for dtype in ('float32', 'float64'):
        a, present = video_frames('vidA', dtype)
        v = VIDEOS['vidA']
        keep = np.array([present[f] and not outlier(a[f]) for f in range(v['n'])])
        assert v['n'] % 64 != 0 and not keep[0] and not keep[-1]
        assert a[v['x_eq_3'], 0, 4] == 3.0 and a[v['x_eq_3'], 1, 4] <= 3 and not keep[v['x_eq_3']]
        assert a[v['x_low_y_high'], 0, 4] <= 3 and a[v['x_low_y_high'], 1, 4] > 3 and keep[v['x_low_y_high']]
        assert (a[v['unused_zero'], :2][:, UNUSED] == 0).all() and keep[v['unused_zero']]
        assert not present[120] and present[119] and present[121] and START < 120 < v['n'] - FRAMES
        assert sorted(np.flatnonzero(~keep)) == [0, 100, 120, 250] and keep.sum() % 3 != 0
        starts = [s for s in range(START, v['n'] - FRAMES, STEP) if keep[s:s + FRAMES].all()]
        assert 0 < len(starts) < len(range(START, v['n'] - FRAMES, STEP))
        b, pb = video_frames('vidB', dtype)
        assert pb.all() and not any(outlier(f) for f in b) and VIDEOS['vidB']['audio'][3] < VIDEOS['vidB']['n'] / 15.0
        assert VIDEOS['vidC']['n'] < START + FRAMES
        d, pd_ = video_frames('vidD', dtype)
        kd = np.array([not outlier(f) for f in d])
        assert kd.any() and not any(kd[s:s + FRAMES].all() for s in range(START, VIDEOS['vidD']['n'] - FRAMES, STEP))
    for name, v in VIDEOS.items():
        assert v['n'] <= 260 and v['audio'][3] <= 18.0


check()
