"""Seeded synthetic keypoint videos with dropouts, missing files and spikes for the repair stage of the clip builder
(speechdrivestemplates_amd/clip_builder.py).  The videos are small (n in {1, 3, 70, 257, 513}, windows of 16
frames from frame 0 or 8).  ``check()`` asserts, with a per-track loop of its own, that every case the tests rely on really occurs
in the generated data."""
import os

import numpy as np
from scipy.io import wavfile

KEPT = [0] + list(range(2, 8)) + [15, 16] + list(range(25, 137))
UNUSED = [1] + list(range(8, 15)) + list(range(17, 25))
FRAMES, STEP = 16, 5
FLAT_X, FLAT_Y = 500.0, 300.0

# video -> frames, seed, start frame and edits, applied in order:
#   ('zero', k, f0, f1)  OpenPose's (0, 0, 0) at keypoint k in frames [f0, f1)     ('missing', f)  no file (the array holds zeros)
#   ('set', f, k, x, y)  exact coordinates                                          ('nan', f, k)   x = NaN
#   ('flat', k)          the whole track at (FLAT_X, FLAT_Y) exactly                ('jump', f, k, dx, dy)  added to the point
VIDEOS = {
    'r1': dict(n=1, seed=21, start=0, edits=[('nan', 0, 45), ('zero', 10, 0, 1)]),
    'r3': dict(n=3, seed=22, start=0, edits=[('zero', 30, 1, 2), ('zero', 10, 0, 3), ('missing', 1)]),
    'r70': dict(n=70, seed=23, start=8, edits=[
        ('flat', 70), ('jump', 20, 70, 80.0, 0.0),                         # an isolated jump in x only
        ('flat', 71), ('jump', 25, 71, 0.0, -60.0),                        # a jump in y only
        ('flat', 72), ('zero', 72, 30, 32), ('jump', 32, 72, 70.0, 70.0),  # a jump next to a gap: m = 3 < 2h + 1 at h = 2
        ('flat', 73), ('jump', 0, 73, 90.0, 0.0),                          # frame 0 at h = 1: m = 2, not tested
        ('flat', 74), ('jump', 40, 74, 0.5, 0.0),                          # mad == 0: a spike with floor_px = 0, saved by a floor of 1
        ('flat', 75), ('jump', 50, 75, 40.0, 0.0), ('jump', 51, 75, 40.0, 0.0),  # two adjacent spikes
        ('flat', 76), ('jump', 69, 76, 0.0, 55.0),                         # a spike in the last frame: no b, keeps value and confidence
        ('flat', 77),                                                      # a flat track with nothing on it
    ] + [('zero', 110, f, f + 1) for f in range(10, 70, 10)]),             # one finger joint lost for one frame, every 10 frames
    'r257': dict(n=257, seed=24, start=0, edits=[
        ('missing', 100), ('missing', 101),           # two adjacent missing files: not recovered at G = 1
        ('zero', 10, 140, 257), ('missing', 150),     # an unused keypoint that cannot be filled under a missing frame whose 121 can
        ('zero', 11, 0, 257),                         # a track without a valid frame: a gap longer than the video
        ('zero', 30, 200, 201), ('zero', 43, 255, 257),
    ]),
    'r513': dict(n=513, seed=25, start=8, edits=[
        ('zero', 30, 20, 21), ('zero', 30, 30, 32),       # gaps of 1 and 2
        ('zero', 31, 40, 44), ('zero', 31, 50, 55),       # 4 and 5
        ('zero', 32, 100, 164), ('zero', 32, 200, 265),   # 64 and 65
        ('zero', 33, 0, 2), ('zero', 34, 511, 513),       # touching frame 0 and frame n - 1
        ('zero', 35, 300, 302), ('zero', 35, 303, 305),   # two gaps separated by one valid frame
        ('zero', 36, 320, 324), ('zero', 37, 322, 327),   # two keypoints with different, overlapping gaps
        ('missing', 350),                                 # a missing file alone
        ('zero', 38, 398, 403), ('missing', 400),         # a missing file inside a longer per-keypoint gap
        ('zero', 10, 420, 421),                           # a zero at an unused keypoint only
        ('set', 430, 40, 2.0, 50.0), ('zero', 40, 431, 432),  # x <= 3, y > 3: valid, and the anchor of the gap behind it
        ('set', 440, 41, 3.0, 3.0),                       # x == 3, y == 3 exactly: invalid
        ('nan', 450, 42),                                 # a NaN inside a fillable gap
        ('zero', 43, 254, 258),                           # a gap across the 256-frame tile boundary
    ]),
}
# (video, max_gap, despike): what the model and the device stage are compared on
PARAMS = [('r1', 1, None), ('r1', 64, (1, 3.0, 0.0)), ('r3', 1, None), ('r3', 64, (3, 3.0, 2.0)),
          ('r70', 1, None), ('r70', 4, (1, 3.0, 10.0)), ('r70', 4, (2, 3.0, 10.0)), ('r70', 4, (2, 3.0, 0.0)), ('r70', 4, (2, 3.0, 1.0)),
          ('r70', 64, (3, 2.5, 10.0)),
          ('r257', 1, None), ('r257', 4, None), ('r257', 64, (2, 3.0, 10.0)),
          ('r513', 1, None), ('r513', 4, None), ('r513', 64, None), ('r513', 4, (2, 3.0, 10.0))]
# speaker -> (dtype, videos, start frame)
SPEAKERS = {'rp_f32': ('float32', ['r257', 'r70'], 8), 'rp_f64': ('float64', ['r257', 'r70'], 8), 'rp_nan_f32': ('float32', ['r1'], 0)}
RATE = 16000


def video_frames(name, dtype):
    """-> (frames (n, 3, 137) in dtype, zero where the file is missing; present (n,) bool)"""
    v = VIDEOS[name]
    n = v['n']
    g = np.random.Generator(np.random.PCG64(v['seed']))
    base = g.uniform(200.0, 900.0, (2, 137))
    base[0, 2], base[0, 5] = 400.0, 640.0  # the shoulders
    drift = np.linspace(0.0, 30.0, n)[:, None, None] * g.uniform(-1.0, 1.0, (2, 137))[None]
    a = np.concatenate([base[None] + drift + g.normal(0.0, 2.0, (n, 2, 137)), g.uniform(0.1, 1.0, (n, 1, 137))], axis=1)
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
        elif e[0] == 'flat':
            a[:, 0, e[1]], a[:, 1, e[1]] = FLAT_X, FLAT_Y
        elif e[0] == 'jump':
            a[e[1], 0, e[2]] += e[3]
            a[e[1], 1, e[2]] += e[4]
        else:
            raise KeyError(e[0])
    a[~present] = 0.0
    return a.astype(dtype), present


def video_audio(name):
    g = np.random.Generator(np.random.PCG64(2000 + VIDEOS[name]['seed']))
    return RATE, np.round(g.uniform(-0.9, 0.9, int(RATE * VIDEOS[name]['n'] / 15.0) + 1) * 32767).astype(np.int16)


def write_speaker(root, speaker):
    dtype, videos, _ = SPEAKERS[speaker]
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


# ------------------------------------------------------------------------------------------- an independent per-track reference

def loop_valid(a, present):
    n = a.shape[0]
    v = np.zeros((n, 137), bool)
    for f in range(n):
        for k in range(137):
            x, y = a[f, 0, k], a[f, 1, k]
            v[f, k] = bool(present[f]) and bool(np.isfinite(x)) and bool(np.isfinite(y)) and not (x <= 3 and y <= 3)
    return v


def _median(values):
    s = sorted(values)
    m = len(s)
    return 0.5 * (s[(m - 1) // 2] + s[m // 2])


def loop_despike(a, valid, h, kappa, floor_px):
    n = a.shape[0]
    spike = np.zeros((n, 137), bool)
    for k in range(137):
        for f in range(n):
            if not valid[f, k]:
                continue
            fr = [g for g in range(max(0, f - h), min(n, f + h + 1)) if valid[g, k]]
            if len(fr) < 3:
                continue
            for c in (0, 1):
                vals = [float(a[g, c, k]) for g in fr]
                med = _median(vals)
                mad = _median([abs(v - med) for v in vals])
                if abs(float(a[f, c, k]) - med) > kappa * (1.4826 * mad) + floor_px:
                    spike[f, k] = True
    return spike


def loop_repair(a, present, max_gap, despike=None):
    """per-track python loops, np.interp for the values (in float64, rounded once to a's dtype)
    -> dict(src_r, present_r, valid, spike, filled, repaired_per_frame, anchors {(f, k): (a, b)})"""
    n = a.shape[0]
    valid0 = loop_valid(a, present)
    spike = loop_despike(a, valid0, *despike) if despike is not None else np.zeros((n, 137), bool)
    valid = valid0 & ~spike
    out = a.copy()
    filled = np.zeros((n, 137), bool)
    anchors = {}
    for k in range(137):
        good = [f for f in range(n) if valid[f, k]]
        for f in range(n):
            if valid[f, k]:
                continue
            before = [g for g in good if g < f]
            after = [g for g in good if g > f]
            if not before or not after or after[0] - before[-1] - 1 > max_gap:
                continue
            lo, hi = before[-1], after[0]
            for c in (0, 1):
                out[f, c, k] = np.interp(float(f), [float(lo), float(hi)], [float(a[lo, c, k]), float(a[hi, c, k])])
            out[f, 2, k] = 0.0
            filled[f, k] = True
            anchors[(f, k)] = (lo, hi)
    per_frame = np.array([sum(filled[f, k] for k in KEPT) for f in range(n)], np.int32)
    return {'src_r': out, 'present_r': np.asarray(present, bool) | (per_frame == 121), 'valid': valid, 'spike': spike, 'filled': filled,
            'repaired_per_frame': per_frame, 'anchors': anchors}


def loop_keep(a, present):
    return np.array([bool(present[f]) and not bool(((a[f, 0, KEPT] <= 3) & (a[f, 1, KEPT] <= 3)).any()) for f in range(a.shape[0])])


def loop_starts(keep, start, frames=FRAMES):
    return [s for s in range(start, len(keep) - frames, STEP) if keep[s:s + frames].all()]


_LOOP = {}


def reference(name, dtype, max_gap, despike):
    """loop_repair of a video and a parameter set, computed once and shared (do not write to it)"""
    key = (name, dtype, max_gap, despike)
    if key not in _LOOP:
        a, present = video_frames(name, dtype)
        _LOOP[key] = loop_repair(a, present, max_gap, despike)
    return _LOOP[key]


def check():
    assert sorted({v['n'] for v in VIDEOS.values()}) == [1, 3, 70, 257, 513] and 70 % 4 != 0
    assert {v['start'] for v in VIDEOS.values()} == {0, 8}
    for dtype in ('float32', 'float64'):
        a, present = video_frames('r513', dtype)
        valid = loop_valid(a, present)
        r1, r4, r64 = (reference('r513', dtype, g, None) for g in (1, 4, 64))
        f1, f4, f64 = r1['filled'], r4['filled'], r64['filled']
        # a gap of exactly G is filled, one of G + 1 untouched, for G in 1, 4, 64
        assert f1[20, 30] and not f1[30:32, 30].any() and f4[30:32, 30].all()
        assert f4[40:44, 31].all() and not f4[50:55, 31].any() and f64[50:55, 31].all() and not f1[40:44, 31].any()
        assert f64[100:164, 32].all() and not f64[200:265, 32].any() and not valid[200:265, 32].any() and valid[199, 32] and valid[265, 32]
        assert np.array_equal(r64['src_r'][200:265, :, 32], a[200:265, :, 32])
        # gaps touching frame 0 and frame n - 1 stay
        assert not valid[0:2, 33].any() and not f64[0:2, 33].any() and not valid[511:513, 34].any() and not f64[511:513, 34].any()
        # two gaps separated by one valid frame
        assert not valid[300:302, 35].any() and valid[302, 35] and not valid[303:305, 35].any() and f4[300:302, 35].all() and f4[303:305, 35].all()
        assert r4['anchors'][(301, 35)] == (299, 302) and r4['anchors'][(303, 35)] == (302, 305)
        # two keypoints with different, overlapping gaps in one frame
        assert f4[322, 36] and not f4[322, 37] and f64[322, 36] and f64[322, 37] and r64['anchors'][(322, 36)] != r64['anchors'][(322, 37)]
        # a missing file alone: every point filled, the frame is back
        assert not present[350] and f1[350].all() and r1['present_r'][350]
        # a missing file inside a longer per-keypoint gap
        assert not present[400] and not valid[398:403, 38].any() and not f4[400, 38] and not r4['present_r'][400] and r64['present_r'][400]
        assert r64['anchors'][(400, 38)] == (397, 403) and r64['anchors'][(400, 39)] == (399, 401)
        # a zero at an unused keypoint only: filled, and the frame was never dropped
        assert 10 in UNUSED and not valid[420, 10] and valid[420, KEPT].all() and f1[420, 10] and r1['repaired_per_frame'][420] == 0
        # x <= 3, y > 3 is valid and an anchor; x == 3, y == 3 exactly is invalid
        assert a[430, 0, 40] <= 3 and a[430, 1, 40] > 3 and valid[430, 40] and r1['anchors'][(431, 40)] == (430, 432)
        assert a[440, 0, 41] == 3 and a[440, 1, 41] == 3 and not valid[440, 41] and f1[440, 41]
        # a NaN inside a fillable gap is filled
        assert np.isnan(a[450, 0, 42]) and present[450] and f1[450, 42] and np.isfinite(r1['src_r'][450, :, 42]).all()
        assert np.isfinite(r1['src_r'][loop_keep(r1['src_r'], r1['present_r'])][:, :2]).all()
        # a gap across a 256-frame tile
        assert f4[254:258, 43].all()
        assert (r4['src_r'][:, 2, :][f4] == 0).all()

        # r257: adjacent missing files, the unused keypoint that cannot be filled, a track without a valid frame
        a, present = video_frames('r257', dtype)
        valid = loop_valid(a, present)
        q1, q4 = reference('r257', dtype, 1, None), reference('r257', dtype, 4, None)
        assert not present[100] and not present[101] and not q1['present_r'][100:102].any() and q4['present_r'][100:102].all()
        assert not present[150] and not q1['filled'][150, 10] and q1['filled'][150, KEPT].all() and q1['present_r'][150]
        assert (q1['src_r'][150, :, 10] == 0).all() and not valid[140:, 10].any()
        assert not valid[:, 11].any() and not reference('r257', dtype, 64, (2, 3.0, 10.0))['filled'][:, 11].any()
        a3, p3 = video_frames('r3', dtype)
        v3 = loop_valid(a3, p3)
        t3 = reference('r3', dtype, 1, None)
        assert not p3[1] and not v3[:, 10].any() and 10 in UNUSED and not t3['filled'][1, 10] and t3['filled'][1, KEPT].all() and t3['present_r'][1]
        assert (t3['src_r'][1, :, 10] == 0).all() and 64 > 3  # a max_gap longer than the video is accepted (PARAMS)
        a1, p1 = video_frames('r1', dtype)
        assert np.isnan(a1[0, 0, 45]) and p1[0] and 45 in KEPT and loop_keep(a1, p1)[0]  # a NaN on a kept frame: the existing error
        assert not reference('r1', dtype, 64, (1, 3.0, 0.0))['filled'].any()

        # r70: the despike cases, by the loop reference
        a, present = video_frames('r70', dtype)
        valid = loop_valid(a, present)
        h1 = reference('r70', dtype, 4, (1, 3.0, 10.0))
        h2 = reference('r70', dtype, 4, (2, 3.0, 10.0))
        z0 = reference('r70', dtype, 4, (2, 3.0, 0.0))
        z1 = reference('r70', dtype, 4, (2, 3.0, 1.0))
        for r in (h1, h2):
            assert list(np.flatnonzero(r['spike'][:, 70])) == [20] and list(np.flatnonzero(r['spike'][:, 71])) == [25]
            assert r['filled'][20, 70] and r['src_r'][20, 0, 70] == FLAT_X and r['src_r'][20, 2, 70] == 0
        assert a[20, 1, 70] == FLAT_Y and a[25, 0, 71] == FLAT_X
        assert not valid[30:32, 72].any() and h2['spike'][32, 72] and h2['filled'][30:33, 72].all() and h2['anchors'][(32, 72)] == (29, 33)
        assert a[0, 0, 73] == FLAT_X + 90.0 and not h1['spike'][0, 73] and h2['spike'][0, 73] and not h2['filled'][0, 73]
        assert z0['spike'][40, 74] and not z1['spike'][40, 74] and not h2['spike'][40, 74] and list(np.flatnonzero(z0['spike'][:, 77])) == []
        assert h2['spike'][50:52, 75].all() and h2['filled'][50:52, 75].all() and h2['anchors'][(50, 75)] == (49, 52)
        assert h2['spike'][69, 76] and not h2['filled'][69, 76] and np.array_equal(h2['src_r'][69, :, 76], a[69, :, 76]) and a[69, 2, 76] > 0
    # the speakers: r70 gives no clip without the repair and some with it
    for sp, (dtype, videos, start) in SPEAKERS.items():
        if 'r70' not in videos:
            continue
        a, present = video_frames('r70', dtype)
        assert loop_starts(loop_keep(a, present), start) == []
        for g, d in ((1, None), (4, (2, 3.0, 10.0))):
            r = reference('r70', dtype, g, d)
            assert len(loop_starts(loop_keep(r['src_r'], r['present_r']), start)) > 0
        a, present = video_frames('r257', dtype)
        assert len(loop_starts(loop_keep(a, present), start)) > 0


check()
