"""Seeded inputs and plain-loop restatements for the audio activity gate of the clip builder (speechdrivestemplates_amd/clip_builder.py;
DESIGN.md section 28): tests/test_speech_gate_host.py checks the numpy models against the loops, tests/test_speech_gate_gpu.py the
kernels against the models on the same inputs."""
import os
import struct

import numpy as np
from scipy.io import wavfile

import synth_keypoint_videos as K

HOP = 160


# ------------------------------------------------------------------------------------------------------------------ plain loops
def loop_hop_energy(x):
    """lane by lane, sample by sample, python floats (IEEE double, each operation rounded on its own)"""
    x = [float(v) for v in np.asarray(x, np.float32)]
    out = []
    for h in range(len(x) // HOP):
        lanes = [0.0] * 64
        for lane in range(64):
            for i in range(lane, HOP, 64):
                n = HOP * h + i
                d = x[n] - (31.0 / 32.0) * (x[n - 1] if n > 0 else 0.0)
                lanes[lane] = lanes[lane] + d * d
        for o in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[l] + lanes[l ^ o] for l in range(64)]
        out.append(lanes[0])
    return np.array(out, np.float64)


def loop_floor(e, floor_pct):
    e = [float(v) for v in e]
    if not e:
        return None
    return sorted(e, key=lambda v: struct.unpack('<Q', struct.pack('<d', v))[0])[(floor_pct * (len(e) - 1)) // 100]


def runs(mask):
    """-> [(value, first, length)] of the maximal runs"""
    out, i, m = [], 0, [bool(v) for v in mask]
    while i < len(m):
        j = i
        while j < len(m) and m[j] == m[i]:
            j += 1
        out.append((m[i], i, j - i))
        i = j
    return out


def loop_smooth(mask, min_run_hops, hang_hops):
    """a serial walk over the runs: open (drop the short active runs), then close (fill the short inner gaps)"""
    m = [bool(v) for v in mask]
    for val, first, length in runs(m):
        if val and length < min_run_hops:
            m[first:first + length] = [False] * length
    for val, first, length in runs(list(m)):
        if not val and length <= hang_hops and first > 0 and first + length < len(m):
            m[first:first + length] = [True] * length
    return np.array(m, bool)


def loop_window_counts(active, n_samples, offsets):
    out = []
    for a0, a1 in offsets:
        a0, a1 = max(a0, 0), min(a1, n_samples)
        inside = [h for h in range(len(active)) if HOP * h >= a0 and HOP * (h + 1) <= a1]
        out.append((sum(1 for h in inside if active[h]), len(inside)))
    return np.array(out, np.int32).reshape(-1, 2)


# --------------------------------------------------------------------------------------------------------------------- tracks
SIZES_ENERGY = (0, 159, 160, 161, 319, 320, 160 * 64 + 1, 160 * 257)


def track(n, seed=0):
    """n float32 samples in (-0.9, 0.9) with signed zeros and a float32 subnormal among them"""
    g = np.random.Generator(np.random.PCG64(7000 + seed + n))
    x = g.uniform(-0.9, 0.9, n).astype(np.float32)
    if n >= 8:
        x[0], x[3], x[5] = -0.0, 0.0, np.float32(1e-41)
        x[n - 1] = -0.0
    if n >= 2 * HOP:  # a whole hop of signed zeros and subnormals: its energy is tiny but the order of the sum is the same
        x[HOP:2 * HOP] = np.where(np.arange(HOP) % 2 == 0, np.float32(-0.0), np.float32(3e-42))
    return x


def energies(h, kind, seed=0):
    """h hop energies: 'random' (distinct), 'ties' (a handful of values, many repeats), 'equal' (one value)"""
    g = np.random.Generator(np.random.PCG64(8000 + seed + h))
    if kind == 'random':
        return (10.0 ** g.uniform(-9.0, 1.0, h)).astype(np.float64)
    if kind == 'ties':
        return g.choice(np.array([0.0, 1e-300, 2.5e-7, 2.5e-7 * (1 + 2 ** -52), 0.125, 3.0]), h)
    return np.full(h, 0.3125, np.float64)


def smoothing_pattern(min_run, hang):
    """one mask that holds, for rule limits min_run and hang (each >= 2): active runs of min_run - 1, min_run and min_run + 1, inner gaps
    of hang and hang + 1, a short run and a short gap at each end of the track, and a place where opening first changes what closing
    does (a short run between two short gaps: closing first would have merged it with its neighbours)"""
    parts = [(0, 1), (1, min_run + 1), (0, hang), (1, min_run), (0, hang + 1), (1, min_run - 1), (0, hang), (1, min_run + 2),
             (0, 1), (1, 1), (0, 1), (1, min_run), (0, hang + 1), (1, 1)]
    return np.concatenate([np.full(n, v, bool) for v, n in parts])


def laid_across(pattern, h, at):
    """a mask of h hops, inactive but for ``pattern`` starting at hop ``at`` (cut at the end of the track)"""
    m = np.zeros(h, bool)
    n = max(0, min(len(pattern), h - at))
    m[at:at + n] = pattern[:n]
    return m


# ---------------------------------------------------------------------------------------------------- the end-to-end speaker
SPEAKER, VIDEOS = 'kp_gate', ('vidA', 'vidB')
GATE = {'min_permille': 500, 'margin_db': 12.0, 'floor_pct': 10, 'abs_dbfs': -60.0, 'hang_hops': 1, 'min_run_hops': 2}
TRACK_SECONDS = {'vidA': 16.7, 'vidB': 9.41}  # vidB's track ends inside its last windows


def hop_plan(video, n_hops):
    """which hops of the cut track are loud: three loud / three quiet hops throughout (a window of an even number of hops that is a
    multiple of 6 is exactly half active), then a silent stretch and a loud stretch"""
    loud = (np.arange(n_hops) % 6) < 3
    if video == 'vidA':
        loud[300:640] = False
        loud[702:] = True  # (behind a whole gap of three: hang_hops = 1 fills nothing in this plan, min_run_hops = 2 removes nothing)
    return loud


def video_audio(video):
    """-> (16000, int16 samples of the whole wav): quiet noise everywhere, loud noise in the planned hops behind the cut at frame START"""
    n = int(16000 * TRACK_SECONDS[video])
    cut = int(round(K.START / 15.0, 6) * 16000)  # the builder's cut: the start time rounded to the microsecond, truncated to a sample
    g = np.random.Generator(np.random.PCG64(9000 + K.VIDEOS[video]['seed']))
    x = g.uniform(-1.0, 1.0, n)
    amp = np.full(n, 2e-4)
    n_hops = (n - cut) // HOP
    amp[cut:cut + n_hops * HOP] = np.where(np.repeat(hop_plan(video, n_hops), HOP), 0.5, 2e-4)
    amp[cut + HOP - 1::HOP] = 2e-4  # the last sample of every hop is quiet: d[n] reads x[n-1], and a loud one would leak into a quiet hop
    return 16000, np.round(x * amp * 32767).astype(np.int16)


def write_speaker(root, name=SPEAKER):
    """the keypoints of synth_keypoint_videos' float32 videos next to the gate's own 16 kHz tracks"""
    base = os.path.join(root, name)
    os.makedirs(os.path.join(base, 'audio_full'), exist_ok=True)
    for video in VIDEOS:
        d = os.path.join(base, 'tmp', 'raw_pose_2d', video)
        os.makedirs(d, exist_ok=True)
        a, present = K.video_frames(video, 'float32')
        for f in np.flatnonzero(present):
            np.save(os.path.join(d, '%s_%06d.npy' % (video, f)), a[f])
        rate, x = video_audio(video)
        wavfile.write(os.path.join(base, 'audio_full', video + '.wav'), rate, x)
    return base
