"""Seeded synthetic keypoint tracks recorded at rates other than 15 fps, for the retime stage of the clip builder
(speechdrivestemplates_amd/clip_builder.py), and an independent per-point reference: ``fractions.Fraction`` for the
time map, plain python floats for the sums.  ``check()`` asserts that every case the tests rely on really occurs in the generated data."""
import math
import os
from fractions import Fraction

import numpy as np
from scipy.io import wavfile

KEPT = [0] + list(range(2, 8)) + [15, 16] + list(range(25, 137))
FRAMES, STEP = 16, 5
MODES = ('nearest', 'linear', 'smooth')
RATES = [(15, 1), (12, 1), (25, 1), (30, 1), (60, 1), (24000, 1001), (30000, 1001), (2997, 100)]

# video -> source frames, seed and edits, applied in order:
#   ('zero', k, f0, f1)  OpenPose's (0, 0, 0) at keypoint k in frames [f0, f1)     ('missing', f)  no file (the array holds zeros)
#   ('set', f, k, x, y)  exact coordinates                                          ('nan', f, k)   x = NaN
#   ('dead', k)          a track that is never valid
VIDEOS = {
    't1': dict(n=1, seed=41, edits=[('zero', 30, 0, 1)]),
    't2': dict(n=2, seed=42, edits=[('zero', 30, 1, 2), ('nan', 0, 45)]),
    't7': dict(n=7, seed=43, edits=[('missing', 0), ('zero', 31, 3, 4), ('dead', 11)]),
    't64': dict(n=64, seed=44, edits=[('missing', 63), ('missing', 20), ('zero', 30, 10, 11), ('zero', 31, 40, 43), ('nan', 33, 42),
                                      ('set', 50, 40, 2.0, 50.0), ('set', 52, 41, 3.0, 3.0), ('dead', 11)]),
    't257': dict(n=257, seed=45, edits=[('missing', 0), ('missing', 128), ('missing', 129), ('missing', 256), ('zero', 30, 100, 101),
                                        ('zero', 32, 101, 102), ('zero', 31, 200, 206), ('nan', 77, 42), ('nan', 78, 43),
                                        ('set', 150, 40, 2.0, 50.0), ('set', 151, 40, 1.0, 60.0), ('set', 160, 41, 3.0, 3.0), ('dead', 11)]),
    't1000': dict(n=1000, seed=46, edits=[('missing', 0), ('missing', 500), ('missing', 999), ('dead', 11), ('nan', 640, 42),
                                          ('set', 700, 40, 2.5, 40.0)] + [('zero', 100 + (f % 7), f, f + 1 + (f % 3)) for f in range(20, 990, 37)]),
    # the two videos of the 30 fps speaker: one-frame dropouts of a finger joint on even source frames (retiming by 2 keeps them, a repair
    # with max_gap 1 fills them), a NaN on an odd frame, a missing file
    'sa': dict(n=330, seed=47, edits=[('zero', 110, f, f + 1) for f in range(40, 320, 40)] + [('nan', 151, 42), ('missing', 201), ('missing', 260)]),
    'sb': dict(n=270, seed=48, edits=[('zero', 100, 120, 121), ('zero', 101, 121, 122), ('set', 90, 40, 2.0, 50.0)]),
}
TRACKS = ['t1', 't2', 't7', 't64', 't257', 't1000']
# speaker -> (dtype, videos, start frame in 15 fps frames, source rate)
SPEAKERS = {'rt_f32': ('float32', ['sa', 'sb'], 8, (30, 1)), 'rt_f64': ('float64', ['sa', 'sb'], 8, (30, 1))}
RATE = 16000


def video_frames(name, dtype):
    """-> (frames (n, 3, 137) in dtype, zero where the file is missing; present (n,) bool): smooth motion plus jitter"""
    v = VIDEOS[name]
    n = v['n']
    g = np.random.Generator(np.random.PCG64(v['seed']))
    base = g.uniform(200.0, 900.0, (2, 137))
    base[0, 2], base[0, 5] = 400.0, 640.0  # the shoulders
    f = np.arange(n, dtype=np.float64)[:, None, None]
    motion = g.uniform(5.0, 40.0, (2, 137))[None] * np.sin(2.0 * np.pi * f * g.uniform(0.005, 0.05, (2, 137))[None] + g.uniform(0.0, 6.0, (2, 137))[None])
    a = np.concatenate([base[None] + motion + g.normal(0.0, 1.5, (n, 2, 137)), g.uniform(0.1, 1.0, (n, 1, 137))], axis=1)
    present = np.ones(n, bool)
    for e in v['edits']:
        if e[0] == 'zero':
            a[e[2]:e[3], :, e[1]] = 0.0
        elif e[0] == 'missing':
            present[e[1]] = False
        elif e[0] == 'set':
            a[e[1], 0, e[2]], a[e[1], 1, e[2]] = e[3], e[4]
        elif e[0] == 'nan':
            a[e[1], 0, e[2]] = np.nan
        elif e[0] == 'dead':
            a[:, :, e[1]] = 0.0
        else:
            raise KeyError(e[0])
    a[~present] = 0.0
    return a.astype(dtype), present


def video_audio(name, fps):
    g = np.random.Generator(np.random.PCG64(3000 + VIDEOS[name]['seed']))
    return RATE, np.round(g.uniform(-0.9, 0.9, int(RATE * VIDEOS[name]['n'] * fps[1] / fps[0]) + 1) * 32767).astype(np.int16)


def write_speaker(root, speaker, every=1, name=None, frame_files=False):
    """the speaker's keypoint files and wavs under root/<name or speaker>; ``every`` = 2 writes source frame 2 j as frame j (the same
    wavs next to keypoints that are 15 fps already); ``frame_files`` adds an empty frames/<video>/<video>_<index>.jpg per source frame"""
    dtype, videos, _, fps = SPEAKERS[speaker]
    base = os.path.join(root, name or speaker)
    os.makedirs(os.path.join(base, 'audio_full'), exist_ok=True)
    for video in videos:
        d = os.path.join(base, 'tmp', 'raw_pose_2d', video)
        os.makedirs(d, exist_ok=True)
        a, present = video_frames(video, dtype)
        a, present = a[::every], present[::every]
        for f in np.flatnonzero(present):
            np.save(os.path.join(d, '%s_%06d.npy' % (video, f)), a[f])
        if frame_files:
            os.makedirs(os.path.join(base, 'frames', video), exist_ok=True)
            for f in range(len(a)):
                open(os.path.join(base, 'frames', video, '%s_%06d.jpg' % (video, f)), 'wb').close()
        rate, x = video_audio(video, fps)
        wavfile.write(os.path.join(base, 'audio_full', video + '.wav'), rate, x)
    return base


# ------------------------------------------------------------------------------------------- an independent per-point reference

def loop_plan(n_src, p, q):
    """the time map by rational brute force: output frame j is at j / 15 s = j / 15 * (P / Q) source frames
    -> dict(n_out, phases, a, phase, nearest_src) as python lists"""
    rate = Fraction(p, q)
    n_out = 0
    while Fraction(n_out, 15) * rate <= n_src - 1:  # the last output frame at or before the last source frame
        n_out += 1
    phases = (rate / 15).denominator  # the fractional parts are the multiples of 1 / phases
    a, phase, near = [], [], []
    for j in range(n_out):
        pos = Fraction(j, 15) * rate
        lo = pos.numerator // pos.denominator
        frac = pos - lo
        assert (frac * phases).denominator == 1
        a.append(lo)
        phase.append(int(frac * phases))
        near.append(min(lo if frac < Fraction(1, 2) else lo + 1, n_src - 1))
    return {'n_out': n_out, 'phases': phases, 'a': a, 'phase': phase, 'nearest_src': near}


def loop_taps(p, q, mode, frac):
    """[(source frame offset from a_j, weight)] of an output frame whose position has the fractional part ``frac`` (a Fraction)"""
    t = float(frac)
    if mode == 'nearest':
        return [(0, 1.0), (1, 0.0)] if frac < Fraction(1, 2) else [(0, 0.0), (1, 1.0)]
    if mode == 'linear':
        return [(0, 1.0 - t), (1, t)]
    ratio = Fraction(p, 15 * q)
    width = max(1.0, float(ratio))
    half = max(1, math.ceil(ratio))
    out = []
    for off in range(1 - half, half + 1):
        d = float(off) - t
        out.append((off, 0.5 * (1.0 + math.cos(math.pi * d / width)) if abs(d) < width else 0.0))
    return out


def loop_valid_point(a, present, f, k):
    if f < 0 or f >= a.shape[0] or not present[f]:
        return False
    x, y = a[f, 0, k], a[f, 1, k]
    return bool(np.isfinite(x)) and bool(np.isfinite(y)) and not (x <= 3 and y <= 3)


def loop_retime(a, present, p, q, mode, min_support=0.75, kps=None):
    """-> dict(src_t, present_t, valid_t, taps_used, nearest_src, kps); only the keypoints ``kps`` (default: all) are computed"""
    n_src = a.shape[0]
    plan = loop_plan(n_src, p, q)
    n_out = plan['n_out']
    kps = list(range(137)) if kps is None else sorted(set(kps))
    out = np.zeros((n_out, 3, 137), a.dtype)
    valid_t = np.zeros((n_out, 137), bool)
    used = np.zeros((n_out, 137), np.uint8)
    present_t = np.zeros(n_out, bool)
    for j in range(n_out):
        taps = [(plan['a'][j] + off, w) for off, w in loop_taps(p, q, mode, Fraction(plan['phase'][j], plan['phases'])) if w != 0.0]
        full = 0.0
        for _, w in taps:
            full = full + w
        present_t[j] = any(0 <= f < n_src and present[f] for f, _ in taps)
        for k in kps:
            live = [(f, w) for f, w in taps if loop_valid_point(a, present, f, k)]
            den = 0.0
            for _, w in live:
                den = den + w
            used[j, k] = len(live)
            if not (den > 0.0 and den >= min_support * full):
                continue
            valid_t[j, k] = True
            for c in range(3):
                num = None
                for f, w in live:
                    term = w * float(a[f, c, k])
                    num = term if num is None else num + term
                out[j, c, k] = num / den
    return {'src_t': out, 'present_t': present_t, 'valid_t': valid_t, 'taps_used': used, 'nearest_src': np.array(plan['nearest_src'], np.int32),
            'kps': kps}


SPECIAL = sorted({e[1] for v in VIDEOS.values() for e in v['edits'] if e[0] in ('zero', 'dead')}
                 | {e[2] for v in VIDEOS.values() for e in v['edits'] if e[0] in ('set', 'nan')})


def loop_keypoints(name):
    """the keypoints the loop reference computes: all of them on the short videos, the edited ones and every eighth on the long ones"""
    return None if VIDEOS[name]['n'] <= 64 else sorted(set(SPECIAL) | set(range(0, 137, 8)))


def clean(a, present):
    """the track with every invalid point set to OpenPose's (0, 0, 0)"""
    out = a.copy()
    for f in range(a.shape[0]):
        for k in range(137):
            if not loop_valid_point(a, present, f, k):
                out[f, :, k] = 0
    return out


def loop_keep(a, present):
    return np.array([bool(present[f]) and not bool(((a[f, 0, KEPT] <= 3) & (a[f, 1, KEPT] <= 3)).any()) for f in range(a.shape[0])])


def loop_starts(keep, start, frames=FRAMES):
    return [s for s in range(start, len(keep) - frames, STEP) if keep[s:s + frames].all()]


def check():
    assert sorted(VIDEOS[v]['n'] for v in TRACKS) == [1, 2, 7, 64, 257, 1000]
    assert {Fraction(p, q) for p, q in RATES} == {Fraction(15), Fraction(12), Fraction(25), Fraction(30), Fraction(60), Fraction(24000, 1001),
                                                 Fraction(30000, 1001), Fraction(2997, 100)}
    a, present = video_frames('t257', 'float32')
    assert not present[0] and not present[256] and not present[128] and present[1]
    assert (a[100, :, 30] == 0).all() and np.isnan(a[77, 0, 42]) and present[77]
    assert a[150, 0, 40] <= 3 and a[150, 1, 40] > 3 and loop_valid_point(a, present, 150, 40)
    assert a[160, 0, 41] == 3 and a[160, 1, 41] == 3 and not loop_valid_point(a, present, 160, 41)
    assert not any(loop_valid_point(a, present, f, 11) for f in range(257))
    # the last output frame lands exactly on the last source frame: 257 frames at 30 fps and at 60 fps, 7 frames at 30 fps
    for n, p, q in ((257, 30, 1), (257, 60, 1), (7, 30, 1), (1, 25, 1)):
        plan = loop_plan(n, p, q)
        assert plan['a'][-1] == n - 1 and plan['phase'][-1] == 0
    assert loop_plan(1000, 30000, 1001)['phases'] == 1001 and loop_plan(1000, 2997, 100)['phases'] == 500 and loop_plan(64, 25, 1)['phases'] == 3
    assert loop_plan(3597, 30000, 1001)['n_out'] == 1800
    # the speaker: no clip over a one-frame dropout that retiming by 2 preserved, more clips once it is repaired
    for sp, (dtype, videos, start, fps) in SPEAKERS.items():
        a, present = video_frames('sa', dtype)
        assert fps == (30, 1) and (a[40, :, 110] == 0).all() and np.isnan(a[151, 0, 42]) and not present[260] and present[::2].sum() == 164
        r = loop_retime(a, present, 30, 1, 'linear', kps=[110, 42])
        assert not r['valid_t'][20, 110] and r['valid_t'][19, 110] and r['valid_t'][75:77, 42].all() and not r['valid_t'][130].any()
        assert len(loop_starts(loop_keep(a[::2], present[::2]), start)) > 0


check()
