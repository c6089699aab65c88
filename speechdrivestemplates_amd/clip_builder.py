"""A custom speaker's clips, built on the GPU from per-frame keypoints and one wav per video (csrc/clip_builder.hip): the
reference's data_preprocess/2_2_remove_outlier.py, 2_3_rescale_shoulder_width.py, 3_1_generate_clips.py and
3_2_split_train_val_test.py without librosa, ffmpeg or tqdm, ending in the ``processed_137.csv`` and clip npz files that
``GestureDataset`` and ``speaker_stats`` read.

Inputs:  <root>/<speaker>/tmp/raw_pose_2d/<video>/<video>_<000123>.npy, (3, 137) float32 or float64 (one dtype per speaker)
         <root>/<speaker>/audio_full/<video>.wav, PCM, any rate, covering the video from t = 0
Outputs: <root>/<speaker>/clips/npz/<speaker>-<video>-<start>-<end>.npz (pose, imgs, audio), tmp/intermediate_csv/tmp_<video>.csv,
         processed_137.csv (validation label ``dev``) and clips.csv (``val``, the reference's file)

Contract: every arithmetic stage has a numpy model below (``model_*``), and the GPU result equals it bit for
bit.  The models exist for the tests; ``build_clips`` has no CPU fallback.

    python -m speechdrivestemplates_amd.clip_builder --root DIR --speaker NAME [--start-frame 80] [--frames 64]
                                                     [--shoulder-chunks 1] [--no-write]
                                                     [--repair-max-gap G] [--despike H KAPPA [FLOOR_PX]]   (section 26, off by default)
                                                     [--source-fps P[/Q]] [--retime nearest|linear|smooth] [--retime-min-support S]
                                                                                    (section 27: keypoints not recorded at 15 fps)
                                                     [--speech-gate PERMILLE] [--gate-margin-db DB] [--gate-floor-pct PCT] [--gate-abs-dbfs DBFS]
                                                     [--gate-hang-ms MS] [--gate-min-ms MS]     (section 28: windows without audio activity dropped)
    python -m speechdrivestemplates_amd.clip_builder --activity-report WAV [--gate-...]          (the gate's hop statistics of one wav)
"""
import argparse
import ctypes as C
import os
import time
from concurrent.futures import ThreadPoolExecutor
from math import gcd

import numpy as np

KP = 137
KEEP_121 = [0] + list(range(2, 8)) + [15, 16] + list(range(25, 137))  # 2_2's pose137_to_pose121 (not the dataset's _KEEP_137)
OLIVER_SHOULDER = 331.0850066245443  # 2_3:68
FPS, SR, STEP, IDLE = 15, 16000, 5, 13  # 3_1:13-14, :167 (FPS // 3); 3_2:21
TRAIN_RATIO = 0.8  # 3_2:17
MAX_READ_THREADS = 16  # keypoint-file reading threads: a fixed cap, not os.cpu_count(), which counts every CPU of a shared host
COLUMNS = ['dataset', 'start', 'end', 'interval_id', 'pose_fn', 'audio_fn', 'video_fn', 'speaker']  # 3_1:140-141
_PCM_FMT = {'uint8': 0, 'int16': 1, 'int32': 2, 'float32': 3}


# ---------------------------------------------------------------------------------------------------------- planning (names only)

def plan_clips(root_dir, speaker):
    """-> [{'video', 'dir', 'frames': {index: path}, 'n_frames': highest index + 1, 'wav'}], videos sorted by name; lists
    directories and opens no file"""
    base = os.path.join(root_dir, speaker)
    pose_root = os.path.join(base, 'tmp', 'raw_pose_2d')
    if not os.path.isdir(pose_root):
        raise FileNotFoundError('No keypoint directory: %s' % pose_root)
    plan = []
    for video in sorted(os.listdir(pose_root)):
        d = os.path.join(pose_root, video)
        if not os.path.isdir(d):
            continue
        frames = {}
        for fn in sorted(os.listdir(d)):
            stem, ext = os.path.splitext(fn)
            head, _, num = stem.rpartition('_')
            if ext != '.npy' or head != video or not num.isdigit():
                raise ValueError('%s: not a keypoint file of video %s (<video>_<frame index>.npy expected)' % (os.path.join(d, fn), video))
            frames[int(num)] = os.path.join(d, fn)
        plan.append({'video': video, 'dir': d, 'frames': frames, 'n_frames': (max(frames) + 1) if frames else 0,
                     'wav': os.path.join(base, 'audio_full', video + '.wav')})
    if not plan:
        raise ValueError('%s holds no video directory' % pose_root)
    return plan


# ------------------------------------------------------------------------------------------------------------------ contract models

def model_frame_flags(src, present):
    """src (n, 3, 137), present (n,) bool -> keep (n,) bool, dist (n,) float64 (0 for dropped frames).  2_2:15-23, 2_3:23-25."""
    p = src[:, :2, :][:, :, KEEP_121]
    outlier = ((p[:, 0] <= 3) & (p[:, 1] <= 3)).any(axis=1)
    keep = np.asarray(present, bool) & ~outlier
    x = src[:, :2, :].astype(np.float64)
    dx, dy = x[:, 0, 2] - x[:, 0, 5], x[:, 1, 2] - x[:, 1, 5]
    with np.errstate(invalid='ignore'):
        dist = np.sqrt(dx * dx + dy * dy)
    return keep, np.where(keep, dist, 0.0)


def model_shoulder_means(dist_kept, chunks):
    """the kept frames' distances in file-name order -> (per-chunk running means (chunks,), frames dropped by the chunking).
    2_3:28-43 and :50-52, in float64, every operation rounded on its own"""
    n = len(dist_kept)
    stride = n // chunks
    means = np.zeros(chunks, np.float64)
    for c in range(chunks):
        avg, num = np.float64(0.0), 0
        for d in dist_kept[c * stride:(c + 1) * stride]:
            weight = num / (num + 1)
            avg = avg * weight + (1 - weight) * np.float64(d)
            num += 1
        means[c] = avg
    return means, n - stride * chunks


def model_scalar(means):
    """2_3:59, :71 (oliver_scalar = 1.0)"""
    return float(OLIVER_SHOULDER * 1.0 / np.average(np.asarray(means, np.float64), axis=0))


def scales_confidence(shoulder_chunks, scale_confidence=None):
    """the reference multiplies the whole (3, 137) array with -np 1 (2_3:92-95) and rows 0 and 1 only with -np > 1 (:75-79)"""
    return (shoulder_chunks == 1) if scale_confidence is None else bool(scale_confidence)


def model_scale(frames, scalar, scale_conf):
    """frames (..., 3, 137) in the file's dtype times the scalar as a python float: the product is formed in that dtype"""
    out = frames.copy()
    if scale_conf:
        return out * float(scalar)
    out[..., :2, :] = out[..., :2, :] * float(scalar)
    return out


def model_clip_starts(keep, start_frame, num_frames):
    """3_1:168-215: a window is a clip iff every one of its frames has a file"""
    n = len(keep)
    pre = np.concatenate([[0], np.cumsum(np.asarray(keep, np.int64))])
    return [s for s in range(start_frame, n - num_frames, STEP) if pre[s + num_frames] - pre[s] == num_frames]


def frame_idx_to_time(frame_idx):
    """3_1:90-97"""
    all_seconds = frame_idx / float(FPS)
    hour = int(all_seconds // 3600)
    minute = int((all_seconds % 3600) // 60)
    seconds = (all_seconds % 3600) % 60
    return f"{hour:02d}:{minute:02d}:{seconds:09.6f}"


def time_to_us(text):
    """the microseconds pandas.to_timedelta reads from frame_idx_to_time's string"""
    h, m, s = text.split(':')
    whole, frac = s.split('.')
    return (int(h) * 3600 + int(m) * 60 + int(whole)) * 1000000 + int(frac)


def audio_offsets(frame_idx, start_frame, num_frames):
    """3_1:172-175: (int(audio_start), int(audio_end)) in 16 kHz samples from the cut at start_frame"""
    t0 = time_to_us(frame_idx_to_time(start_frame))
    a0 = (time_to_us(frame_idx_to_time(frame_idx)) - t0) / 1e6 * SR
    a1 = (time_to_us(frame_idx_to_time(frame_idx + num_frames)) - t0) / 1e6 * SR
    return int(a0), int(a1)


def source_cut(start_frame, sr_in):
    """the source sample the track is cut at: int(start_seconds * sr_in), start_seconds rounded to the microsecond"""
    return int(time_to_us(frame_idx_to_time(start_frame)) / 1e6 * sr_in)


def model_pcm_to_mono(a):
    """wavfile.read's array -> float32 mono, gesture_dataset._demo_item's conversion"""
    if a.dtype.kind == 'i':
        a = a.astype(np.float32) / float(2 ** (8 * a.dtype.itemsize - 1))
    elif a.dtype.kind == 'u':
        a = (a.astype(np.float32) - 128.0) / 128.0
    else:
        a = a.astype(np.float32)
    if a.ndim == 2:
        a = a.mean(axis=1)
    return a


def design_taps(sr_in, sr_out=SR):
    """-> (up, down, taps float64 with the leading zero pad, n_pre_remove): scipy.signal.resample_poly's default filter
    (firwin(2*10*max(up, down) + 1, 1/max(up, down), window=('kaiser', 5.0)) * up) and its centring"""
    from scipy.signal import firwin
    g = gcd(int(sr_in), int(sr_out))
    up, down = int(sr_out) // g, int(sr_in) // g
    max_rate = max(up, down)
    half_len = 10 * max_rate
    h = firwin(2 * half_len + 1, 1. / max_rate, window=('kaiser', 5.0)).astype(np.float64)
    h *= up
    n_pre_pad = down - half_len % down
    return up, down, np.concatenate([np.zeros(n_pre_pad), h]), (half_len + n_pre_pad) // down


def resampled_length(n_in, up, down):
    n = n_in * up
    return n // down + bool(n % down)


def model_resample(x, sr_in, sr_out=SR, dtype=np.float32):
    """polyphase FIR of float32 (or float64) samples: y[j] = sum_q taps[k0 + up*q] * x[t//up - q], t = (j + n_pre_remove)*down,
    k0 = t % up, accumulated in float64 in ascending q with x zero outside the track, rounded once to ``dtype``"""
    x = np.asarray(x)
    if int(sr_in) == int(sr_out):
        return x.astype(dtype)
    up, down, taps, n_pre = design_taps(sr_in, sr_out)
    n_in = len(x)
    n_out = resampled_length(n_in, up, down)
    t = (np.arange(n_out, dtype=np.int64) + n_pre) * down
    k0, ib = t % up, t // up
    x64 = x.astype(np.float64)
    acc = np.zeros(n_out, np.float64)
    for q in range((len(taps) + up - 1) // up):
        k, i = k0 + up * q, ib - q
        ok = (k < len(taps)) & (i >= 0) & (i < n_in)
        prod = taps[np.where(ok, k, 0)] * x64[np.where(ok, i, 0)]
        acc = np.where(ok, acc + prod, acc)
    return acc.astype(dtype)


def split_labels(n, val_label='dev'):
    """3_2:31-43: the first int(0.8 n) clips train, the next 13 idle, the rest validation"""
    n_train = int(n * TRAIN_RATIO)
    n_idle = min(IDLE, n - n_train)
    return ['train'] * n_train + ['idle'] * n_idle + [val_label] * (n - n_train - n_idle)


# ---------------------------------------------------------------------------------------- repair of dropouts and spikes (section 26)

MAX_GAP, MAX_HALF = 64, 3  # the library's limits (sdt_clip_repair_fill, sdt_clip_repair_valid)


def repair_params(max_gap, despike=None):
    """-> (max_gap, None or (h, kappa, floor_px)) as ints / floats; a ValueError names what is out of range"""
    if int(max_gap) != max_gap or not 1 <= int(max_gap) <= MAX_GAP:
        raise ValueError('repair_max_gap must be an integer in 1..%d, not %r' % (MAX_GAP, max_gap))
    if despike is None:
        return int(max_gap), None
    d = tuple(despike)
    if len(d) == 2:
        d = d + (0.0,)
    if len(d) != 3:
        raise ValueError('despike is (h, kappa) or (h, kappa, floor_px), not %r' % (despike,))
    h, kappa, floor_px = d
    if int(h) != h or not 1 <= int(h) <= MAX_HALF:
        raise ValueError('despike h must be an integer in 1..%d, not %r' % (MAX_HALF, h))
    if not (np.isfinite(kappa) and kappa > 0) or not (np.isfinite(floor_px) and floor_px >= 0):
        raise ValueError('despike kappa must be positive and floor_px not negative, both finite, not %r, %r' % (kappa, floor_px))
    return int(max_gap), (int(h), float(kappa), float(floor_px))


def model_valid(src, present):
    """src (n, 3, 137), present (n,) -> (n, 137) bool: the 2_2 rule per point (x <= 3 and y <= 3 is invalid, compared in src's dtype)
    on frames with a file; a non-finite coordinate is invalid"""
    x, y = src[:, 0, :], src[:, 1, :]
    with np.errstate(invalid='ignore'):
        low = (x <= 3) & (y <= 3)
    return np.asarray(present, bool)[:, None] & np.isfinite(x) & np.isfinite(y) & ~low


def _window_median(s, m):
    """s (w, ...) ascending along axis 0 with +inf behind the m values -> 0.5 * (s[(m-1)//2] + s[m//2])"""
    lo = np.take_along_axis(s, ((m - 1) // 2)[None], axis=0)[0]
    hi = np.take_along_axis(s, (m // 2)[None], axis=0)[0]
    return 0.5 * (lo + hi)


def model_despike(src, valid, h, kappa, floor_px):
    """-> spike (n, 137) bool.  A valid point is tested against the m >= 3 valid points of frames f-h..f+h of its track (centre
    included, clipped to the video), per coordinate in float64: |v - med| > kappa * (1.4826 * mad) + floor_px in x or in y.  Every
    verdict comes from ``valid`` as given, none from another verdict."""
    n = src.shape[0]
    ok = np.zeros((2 * h + 1, n, KP), bool)
    for i, d in enumerate(range(-h, h + 1)):
        lo, hi = max(0, -d), min(n, n - d)  # frames f with 0 <= f + d < n
        if lo < hi:
            ok[i, lo:hi] = valid[lo + d:hi + d]
    m = ok.sum(axis=0)
    m_safe = np.maximum(m, 1)
    spike = np.zeros((n, KP), bool)
    with np.errstate(invalid='ignore', over='ignore'):
        for c in (0, 1):
            v = src[:, c, :].astype(np.float64)
            win = np.full((2 * h + 1, n, KP), np.inf)
            for i, d in enumerate(range(-h, h + 1)):
                lo, hi = max(0, -d), min(n, n - d)
                if lo < hi:
                    win[i, lo:hi] = np.where(ok[i, lo:hi], v[lo + d:hi + d], np.inf)
            s = np.sort(win, axis=0)
            med = _window_median(s, m_safe)
            dev = np.sort(np.where(np.arange(2 * h + 1)[:, None, None] < m[None], np.abs(s - med[None]), np.inf), axis=0)
            mad = _window_median(dev, m_safe)
            bar = kappa * (1.4826 * mad) + floor_px
            spike |= valid & (m >= 3) & (np.abs(v - med) > bar)
    return spike


def model_repair(src, present, max_gap, despike=None):
    """-> dict(src_r, present_r (n,) bool, valid, spike, filled (n, 137) bool, repaired_per_frame (n,) int32).  An invalid point with
    valid frames a < f < b nearest on its track and b - a - 1 <= max_gap becomes xa + (xb - xa) * ((f - a) / (b - a)) in float64,
    every operation rounded on its own, rounded once to src's dtype, with confidence 0; nothing else changes"""
    max_gap, despike = repair_params(max_gap, despike)
    n = src.shape[0]
    present = np.asarray(present, bool)
    valid0 = model_valid(src, present)
    spike = model_despike(src, valid0, *despike) if despike is not None else np.zeros((n, KP), bool)
    valid = valid0 & ~spike
    idx = np.arange(n, dtype=np.int64)[:, None]
    a = np.maximum.accumulate(np.where(valid, idx, -1), axis=0)            # the last valid frame at or before f
    b = np.minimum.accumulate(np.where(valid, idx, n)[::-1], axis=0)[::-1]  # the first valid frame at or after f
    filled = ~valid & (a >= 0) & (b < n) & (b - a - 1 <= max_gap)
    a_s, b_s = np.where(filled, a, 0), np.where(filled, b, 0)
    t = (idx - a_s).astype(np.float64) / np.where(filled, b_s - a_s, 1).astype(np.float64)
    out = src.copy()
    for c in (0, 1):
        v = src[:, c, :].astype(np.float64)
        va, vb = np.take_along_axis(v, a_s, axis=0), np.take_along_axis(v, b_s, axis=0)
        with np.errstate(invalid='ignore', over='ignore'):
            fill = (va + (vb - va) * t).astype(src.dtype)
        out[:, c, :] = np.where(filled, fill, src[:, c, :])
    out[:, 2, :] = np.where(filled, src.dtype.type(0), src[:, 2, :])
    per_frame = filled[:, KEEP_121].sum(axis=1).astype(np.int32)
    return {'src_r': out, 'present_r': present | (per_frame == len(KEEP_121)), 'valid': valid, 'spike': spike, 'filled': filled,
            'repaired_per_frame': per_frame}


def model_repaired_per_clip(repaired_per_frame, starts, num_frames):
    """the filled kept keypoints of each window, through an integer prefix sum"""
    pre = np.concatenate([[0], np.cumsum(np.asarray(repaired_per_frame, np.int64))])
    return np.array([pre[s + num_frames] - pre[s] for s in starts], np.int32)


def model_repair_summary(present, keep0, keep_r, rep, starts0, starts_r, per_clip, num_frames):
    """the ``repair`` entry of a video's summary from the stage's records (counts on the host, exact integers)"""
    return {'points_filled': int(rep['filled'].sum()), 'spikes': int(rep['spike'].sum()),
            'spikes_unfilled': int((rep['spike'].astype(bool) & ~rep['filled'].astype(bool)).sum()),
            'frames_recovered': int((np.asarray(keep_r, bool) & ~np.asarray(keep0, bool)).sum()),
            'missing_recovered': int((np.asarray(rep['present_r'], bool) & ~np.asarray(present, bool)).sum()),
            'clips_without_repair': len(starts0), 'clips_with_repair': len(starts_r),
            'max_repaired_share': float(max(per_clip) / (num_frames * len(KEEP_121))) if len(per_clip) else 0.0}


# ------------------------------------------------------------------------- keypoints recorded at any frame rate -> 15 fps (section 27)

RETIME_MODES = ('nearest', 'linear', 'smooth')
MAX_FPS_NUM, MAX_FPS_DEN, MAX_RATE, MAX_PHASES, MAX_TAPS = 1 << 20, 1 << 16, 240, 16384, 32  # the library's limits (sdt_clip_retime)


def parse_fps(fps, name='fps'):
    """an int, an (int, int) pair or a string 'P' / 'P/Q' -> (P, Q) in lowest terms; a ValueError names ``name``.  A float is refused:
    29.97 is not 30000/1001, and the time map is exact integer arithmetic"""
    if isinstance(fps, (float, np.floating)):
        raise ValueError("%s must be an exact fraction, not the float %r: give it as 'P/Q', for example '30000/1001'" % (name, fps))
    try:
        if isinstance(fps, str):
            parts = fps.strip().split('/')
            if not 1 <= len(parts) <= 2 or not all(s.strip().isdigit() for s in parts):
                raise TypeError
            p, q = int(parts[0]), int(parts[1]) if len(parts) == 2 else 1
        elif isinstance(fps, (tuple, list)):
            if len(fps) != 2 or any(isinstance(v, (bool, float, np.floating)) or int(v) != v for v in fps):
                raise TypeError
            p, q = int(fps[0]), int(fps[1])
        else:
            if isinstance(fps, bool) or int(fps) != fps:
                raise TypeError
            p, q = int(fps), 1
    except (TypeError, ValueError):
        raise ValueError("%s must be an int, an (int, int) pair or a string 'P/Q' such as '30000/1001', not %r" % (name, fps)) from None
    if p < 1 or q < 1:
        raise ValueError('%s must be positive, not %d/%d' % (name, p, q))
    c = gcd(p, q)
    p, q = p // c, q // c
    if p > MAX_FPS_NUM or q > MAX_FPS_DEN or p < q or p > MAX_RATE * q:
        raise ValueError('%s = %d/%d: in lowest terms the numerator must be at most 2^20, the denominator at most 2^16 and the rate in '
                         '[1, %d] fps' % (name, p, q, MAX_RATE))
    if FPS * q // gcd(p, FPS * q) > MAX_PHASES:
        raise ValueError('%s = %d/%d has %d phases against the %d fps grid (at most %d)' % (name, p, q, FPS * q // gcd(p, FPS * q), FPS, MAX_PHASES))
    return p, q


def retime_params(mode, min_support, names=('mode', 'min_support')):
    """-> (mode, float(min_support)); a ValueError names the argument (``names``: what the caller calls them)"""
    if mode not in RETIME_MODES:
        raise ValueError('%s must be one of %s, not %r' % (names[0], ', '.join(RETIME_MODES), mode))
    try:
        s = float(min_support)
    except (TypeError, ValueError):
        s = float('nan')
    if not 0.0 < s <= 1.0:
        raise ValueError('%s must lie in (0, 1], not %r' % (names[1], min_support))
    return mode, s


def model_retime_plan(n_src, p, q):
    """the time map, int64 only: output frame j sits at source time j * P / D frames, D = 15 * Q
    -> dict(D, g, phases, n_out, a (n_out,), r, phase int64, nearest_src (n_out,) int32)"""
    n_src, p, q = int(n_src), int(p), int(q)
    if n_src < 1:
        raise ValueError('n_src must be at least 1, not %d' % n_src)
    d = FPS * q
    g = gcd(p, d)
    n_out = (n_src - 1) * d // p + 1
    prod = np.arange(n_out, dtype=np.int64) * np.int64(p)
    a, r = prod // d, prod % d
    return {'D': d, 'g': g, 'phases': d // g, 'n_out': n_out, 'a': a, 'r': r, 'phase': r // g,
            'nearest_src': np.minimum(a + (2 * r >= d), n_src - 1).astype(np.int32)}


def model_retime_taps(p, q, mode):
    """-> h (phases, L) float64, not normalised.  Tap i of phase phi weighs source frame a_j + i_lo + i, i_lo = 1 - L // 2, at distance
    d = i_lo + i - t, t = (phi * g) / D.  nearest: (1, 0) if 2 r < D else (0, 1); linear: (1 - t, t); smooth: a raised cosine of half
    width W = max(1, P / D) source frames, 0.5 * (1 + cos(pi * d / W)) for |d| < W, L = 2 * ceil(W)"""
    from math import cos, pi
    p, q = int(p), int(q)
    if mode not in RETIME_MODES:
        raise ValueError('mode must be one of %s, not %r' % (', '.join(RETIME_MODES), mode))
    d = FPS * q
    g = gcd(p, d)
    phases = d // g
    if mode == 'smooth':
        width = max(1.0, p / d)
        taps = 2 * max(1, -(-p // d))
    else:
        width, taps = 1.0, 2
    if phases > MAX_PHASES or taps > MAX_TAPS:
        raise ValueError('fps = %d/%d needs a tap table of %d x %d (at most %d x %d)' % (p, q, phases, taps, MAX_PHASES, MAX_TAPS))
    i_lo = 1 - taps // 2
    h = np.zeros((phases, taps), np.float64)
    for phi in range(phases):
        r = phi * g
        t = float(r) / float(d)
        if mode == 'nearest':
            h[phi] = (1.0, 0.0) if 2 * r < d else (0.0, 1.0)
        elif mode == 'linear':
            h[phi] = (1.0 - t, t)
        else:
            for i in range(taps):
                dist = float(i_lo + i) - t
                if abs(dist) < width:
                    h[phi, i] = 0.5 * (1.0 + cos(pi * dist / width))
    return h


def model_retime(src, present, p, q, mode='linear', min_support=0.75):
    """src (n_src, 3, 137), present (n_src,) at P/Q fps -> dict(src_t (n_out, 3, 137) in src's dtype, present_t (n_out,) bool, valid_t
    (n_out, 137) bool, taps_used (n_out, 137) uint8, nearest_src (n_out,) int32, counts (3,) int64 = invalid source points, source points
    with a non-finite x or y, invalid output points).  Per output point, over the non-zero taps with a valid source point (``model_valid``;
    a frame outside the video is invalid) in ascending order, in float64, every operation rounded on its own: num = sum h * v for x, y and
    the confidence, den = sum h; full = sum h over all non-zero taps.  Valid iff den > 0 and den >= min_support * full: then num / den,
    rounded once to src's dtype; else (0, 0, 0)"""
    mode, min_support = retime_params(mode, min_support)
    n_src = src.shape[0]
    present = np.asarray(present, bool)
    plan = model_retime_plan(n_src, p, q)
    h = model_retime_taps(p, q, mode)
    n_out, taps = plan['n_out'], h.shape[1]
    i_lo = 1 - taps // 2
    valid_src = model_valid(src, present)
    s64 = src.astype(np.float64)
    num = np.zeros((3, n_out, KP), np.float64)
    den = np.zeros((n_out, KP), np.float64)
    full = np.zeros(n_out, np.float64)
    used = np.zeros((n_out, KP), np.uint8)
    present_t = np.zeros(n_out, bool)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(taps):
            hi = h[plan['phase'], i]
            nz = hi != 0
            f = plan['a'] + (i_lo + i)
            inside = nz & (f >= 0) & (f < n_src)
            fs = np.where(inside, f, 0)
            full = np.where(nz, full + hi, full)
            present_t |= inside & present[fs]
            ok = inside[:, None] & valid_src[fs]
            for c in range(3):
                prod = hi[:, None] * s64[fs, c, :]
                num[c] = np.where(ok, np.where(used == 0, prod, num[c] + prod), num[c])
            den = np.where(ok, den + hi[:, None], den)
            used = used + ok.astype(np.uint8)
        valid_t = (den > 0) & (den >= (np.float64(min_support) * full)[:, None])
        out = np.zeros((n_out, 3, KP), src.dtype)
        for c in range(3):
            out[:, c, :] = np.where(valid_t, (num[c] / np.where(valid_t, den, 1.0)).astype(src.dtype), src.dtype.type(0))
    x, y = src[:, 0, :], src[:, 1, :]
    counts = np.array([(~valid_src).sum(), (~(np.isfinite(x) & np.isfinite(y))).sum(), (~valid_t).sum()], np.int64)
    return {'src_t': out, 'present_t': present_t, 'valid_t': valid_t, 'taps_used': used, 'nearest_src': plan['nearest_src'], 'counts': counts}


def model_retime_summary(rec, n_src, p, q, mode):
    """the ``retime`` entry of a video's summary from the stage's records (exact integers)"""
    counts = [int(v) for v in np.asarray(rec['counts']).reshape(-1)]
    return {'source_frames': int(n_src), 'frames': int(len(rec['nearest_src'])), 'points_invalid_in': counts[0], 'points_invalid_out': counts[2],
            'nonfinite_in': counts[1], 'mode': mode, 'P': int(p), 'Q': int(q), 'phases': FPS * int(q) // gcd(int(p), FPS * int(q))}


# ------------------------------------------------------------------------------- windows without audio activity dropped (section 28)

HOP, PRE_EMPHASIS = 160, 31.0 / 32.0  # 10 ms at 16 kHz; a coefficient that is exact in binary, so its product with a float32 sample is exact
MAX_HOPS, MAX_RUN_HOPS = 1 << 24, 1024  # the library's limits (sdt_clip_speech_*)
GATE_DEFAULTS = {'margin_db': 12.0, 'floor_pct': 10, 'abs_dbfs': -60.0, 'hang_hops': 20, 'min_run_hops': 5}  # untuned: no real footage
_GATE_INT = {'min_permille': (1, 1000), 'floor_pct': (0, 50), 'hang_hops': (0, MAX_RUN_HOPS), 'min_run_hops': (0, MAX_RUN_HOPS)}
_GATE_REAL = {'margin_db': (0.0, 60.0), 'abs_dbfs': (-120.0, 0.0)}


def speech_gate_params(gate):
    """a dict with 'min_permille' and any of margin_db, floor_pct, abs_dbfs, hang_hops, min_run_hops (GATE_DEFAULTS for the rest) -> all six
    as ints / floats; a ValueError names what is unknown, missing or out of range"""
    if not isinstance(gate, dict):
        raise ValueError("speech_gate is None or a dict such as {'min_permille': 500}, not %r" % (gate,))
    unknown = sorted(set(gate) - set(_GATE_INT) - set(_GATE_REAL))
    if unknown:
        raise ValueError('speech_gate: unknown key %s (known: %s)' % (', '.join(map(repr, unknown)), ', '.join(sorted(set(_GATE_INT) | set(_GATE_REAL)))))
    if 'min_permille' not in gate:
        raise ValueError('speech_gate needs min_permille (1..1000): the share of active hops, in thousandths, a window must reach')
    full = dict(GATE_DEFAULTS)
    full.update(gate)
    out = {}
    for k, (lo, hi) in _GATE_INT.items():
        v = full[k]
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or int(v) != v \
                or not lo <= int(v) <= hi:
            raise ValueError('speech_gate %s must be an integer in %d..%d, not %r' % (k, lo, hi, v))
        out[k] = int(v)
    for k, (lo, hi) in _GATE_REAL.items():
        v = full[k]
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) \
                or not lo <= float(v) <= hi:
            raise ValueError('speech_gate %s must be finite and in %g..%g, not %r' % (k, lo, hi, v))
        out[k] = float(v)
    return out


def gate_ms_to_hops(ms, name):
    """a duration in ms that is a whole multiple of the 10 ms hop -> hops; a ValueError names the argument"""
    if isinstance(ms, (bool, np.bool_)) or not isinstance(ms, (int, float, np.integer, np.floating)) or not np.isfinite(ms) or int(ms) != ms \
            or int(ms) < 0 or int(ms) % 10:
        raise ValueError('%s must be a whole, non-negative multiple of 10 ms (one hop), not %r' % (name, ms))
    return int(ms) // 10


def gate_constants(params):
    """-> (M, A): the margin as a power ratio and the absolute floor as the energy of one hop, python floats (passed to the device as doubles)"""
    return 10 ** (params['margin_db'] / 10), HOP * 10 ** (params['abs_dbfs'] / 10)


def model_hop_energy(x):
    """x (N,) float32 -> e (N // 160,) float64: the sum over each hop of (x[n] - (31/32) x[n-1])^2, x[-1] = 0, in float64, every operation
    rounded on its own, in the order of the kernel: lane l of 64 adds samples l, l + 64, l + 128 (below 160) from +0.0, then the xor
    butterfly 32, 16, 8, 4, 2, 1"""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    n_hops = len(x64) // HOP
    lanes = np.zeros((n_hops, 64), np.float64)
    if n_hops == 0:
        return lanes[:, 0].copy()
    with np.errstate(invalid='ignore', over='ignore'):
        d = x64 - PRE_EMPHASIS * np.concatenate([[0.0], x64[:-1]])
        sq = (d * d)[:n_hops * HOP].reshape(n_hops, HOP)
        for j in range(0, HOP, 64):
            w = min(64, HOP - j)
            lanes[:, :w] = lanes[:, :w] + sq[:, j:j + w]
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, idx ^ o]
    return lanes[:, 0].copy()


def model_floor(energy, floor_pct):
    """the energy of rank (floor_pct * (H - 1)) // 100 in ascending order of the bit patterns (energies are not negative, so that is the
    order of the values); None without a hop"""
    e = np.ascontiguousarray(energy, np.float64)
    if len(e) == 0:
        return None
    k = (int(floor_pct) * (len(e) - 1)) // 100
    return float(np.sort(e.view(np.uint64))[k:k + 1].view(np.float64)[0])


def model_mask(energy, floor, margin, abs_floor):
    """-> (active_raw (H,) bool, thr): thr = floor * margin (rounded once) where that is greater than abs_floor, else abs_floor"""
    with np.errstate(invalid='ignore', over='ignore'):
        scaled = np.float64(floor) * np.float64(margin)
        thr = float(scaled) if scaled > abs_floor else float(abs_floor)
        return np.asarray(energy, np.float64) > thr, thr


def _nearest_marks(mark):
    """mark (H,) bool -> (the last marked index at or before h or -1, the first at or after h or H)"""
    n = len(mark)
    idx = np.arange(n, dtype=np.int64)
    prev = np.maximum.accumulate(np.where(mark, idx, -1)) if n else idx
    nxt = np.minimum.accumulate(np.where(mark, idx, n)[::-1])[::-1] if n else idx
    return prev, nxt


def model_smooth(active_raw, min_run_hops, hang_hops):
    """(a) every maximal run of active hops shorter than min_run_hops becomes inactive; then (b) every maximal run of inactive hops of at
    most hang_hops with an active hop on both sides becomes active.  0 disables a rule.  Integers only"""
    m = np.asarray(active_raw, bool)
    n = len(m)
    prev, nxt = _nearest_marks(~m)
    opened = m & (nxt - prev - 1 >= int(min_run_hops))
    prev, nxt = _nearest_marks(opened)
    return opened | ((prev >= 0) & (nxt < n) & (nxt - prev - 1 <= int(hang_hops)))


def model_window_counts(active, n_samples, offsets):
    """offsets [(a0, a1)] in samples -> (n, 2) int32 of (c, n_h): the hops wholly inside [a0, min(a1, N)) (a0 below 0 counts as 0) and the
    active ones among them, through an integer prefix sum"""
    pre = np.concatenate([[0], np.cumsum(np.asarray(active, bool).astype(np.int64))])
    n_hops = len(pre) - 1
    out = np.zeros((len(offsets), 2), np.int32)
    for i, (a0, a1) in enumerate(offsets):
        h0 = -(-max(int(a0), 0) // HOP)
        h1 = min(max(min(int(a1), int(n_samples)), 0) // HOP, n_hops)
        if h1 > h0:
            out[i] = (pre[h1] - pre[h0], h1 - h0)
    return out


def model_windows_kept(counts, min_permille):
    """(n, 2) of (c, n_h) -> (n,) bool: n_h > 0 and 1000 c >= min_permille n_h, in int64"""
    c = np.asarray(counts, np.int64).reshape(-1, 2)
    return (c[:, 1] > 0) & (1000 * c[:, 0] >= int(min_permille) * c[:, 1])


def _db(v):
    return float(10.0 * np.log10(v)) if v is not None and v > 0 else float('-inf') if v is not None else None


def speech_gate_summary(n_hops, n_raw, n_active, floor, thr, n_windows, n_kept):
    """the ``speech_gate`` entry of a video's summary (floor_db / thr_db: 10 log10 on the host, for reading only)"""
    share = n_active / n_hops if n_hops else 0.0
    note = None
    if n_hops and not 0.05 <= share <= 0.95:
        note = ('%.1f %% of the hops are active: ' % (100 * share)) + (
            'the floor may lie inside the speech (see floor_pct, abs_dbfs)' if share < 0.05 else 'the gate drops next to nothing here')
    return {'hops': int(n_hops), 'active_raw': int(n_raw), 'active': int(n_active), 'floor_db': _db(floor), 'thr_db': _db(thr) if n_hops else None,
            'windows': int(n_windows), 'kept': int(n_kept), 'active_share': share, 'note': note, 'clips': 'clips %d -> %d' % (n_windows, n_kept)}


def model_speech_gate(x, starts, start_frame, num_frames, gate):
    """the whole stage on one video's cut 16 kHz track x and the window starts the keypoints allow -> dict(energy, floor, thr, active_raw,
    active, offsets, counts_all, kept (bool per start), starts, counts, summary)"""
    p = speech_gate_params(gate)
    margin, abs_floor = gate_constants(p)
    x = np.asarray(x, np.float32)
    e = model_hop_energy(x)
    if not np.isfinite(e).all():
        raise ValueError('non-finite hop energy')
    floor = model_floor(e, p['floor_pct'])
    if len(e):
        raw, thr = model_mask(e, floor, margin, abs_floor)
    else:
        raw, thr = np.zeros(0, bool), None
    active = model_smooth(raw, p['min_run_hops'], p['hang_hops'])
    offs = [audio_offsets(int(s), start_frame, num_frames) for s in starts]
    counts = model_window_counts(active, len(x), offs)
    kept = model_windows_kept(counts, p['min_permille'])
    return {'energy': e, 'floor': floor, 'thr': thr, 'active_raw': raw, 'active': active, 'offsets': offs, 'counts_all': counts, 'kept': kept,
            'starts': np.asarray(starts, np.int64)[kept], 'counts': counts[kept],
            'summary': speech_gate_summary(len(e), raw.sum(), active.sum(), floor, thr, len(offs), kept.sum())}


# ----------------------------------------------------------------------------------------------------------------------- host I/O

def _read_frames(video, dtype, pool):
    """-> (src (n, 3, 137) pinned torch tensor, present (n,) uint8 numpy); missing frames stay zero"""
    import torch
    n = video['n_frames']
    src = torch.zeros((n, 3, KP), dtype=dtype).pin_memory()
    dst = src.numpy()
    present = np.zeros(n, np.uint8)

    def one(item):
        idx, path = item
        a = np.load(path)
        if a.shape != (3, KP):
            raise ValueError('%s: shape %s, expected (3, 137)' % (path, a.shape))
        if a.dtype != dst.dtype:
            raise ValueError('%s: dtype %s, but the first keypoint file of the speaker is %s (one dtype per speaker)' % (path, a.dtype, dst.dtype))
        dst[idx] = a
        present[idx] = 1
    for f in [pool.submit(one, it) for it in video['frames'].items()]:
        f.result()
    return src, present


def _read_wav(path):
    from scipy.io import wavfile
    if not os.path.exists(path):
        raise FileNotFoundError('No audio track: %s' % path)
    sr, a = wavfile.read(path)
    if str(a.dtype) not in _PCM_FMT:
        raise ValueError('%s: %s samples (uint8, int16, int32 or float32 PCM expected)' % (path, a.dtype))
    if a.ndim == 2 and a.shape[1] > 8:
        raise ValueError('%s: %d channels (at most 8)' % (path, a.shape[1]))
    return int(sr), np.ascontiguousarray(a)


def frame_image_paths(root_dir, speaker, video, start, num_frames, nearest_src=None):
    """3_1:113-118, :187-189: the frame paths, from names alone.  ``nearest_src``: the source frame of each 15 fps frame of a retimed
    video (section 27), so that the names are those of frames that were shot"""
    d = os.path.join(root_dir, speaker, 'frames', video)
    idx = [start + i if nearest_src is None else int(nearest_src[start + i]) for i in range(num_frames)]
    return np.array([os.path.join(d, video + f"_{str(f).zfill(6)}.jpg") for f in idx])


def clip_relpath(speaker, video, start, num_frames):
    return os.path.join('clips', 'npz', '%s-%s-%s-%s.npz' % (speaker, video, start, start + num_frames))


def video_table(speaker, video, starts, num_frames):
    """the rows 3_1 writes to tmp_<video>.csv; pose_fn relative to <root>/<speaker> (the form speaker_stats and GestureDataset join)"""
    import pandas as pd
    rows = {c: [] for c in COLUMNS}
    for s in starts:
        rows['dataset'].append('train')
        rows['start'].append(int(s))
        rows['end'].append(int(s) + num_frames)
        rows['interval_id'].append(video)
        rows['pose_fn'].append(clip_relpath(speaker, video, int(s), num_frames))
        rows['audio_fn'].append(os.path.join('audio_full', video + '.wav'))
        rows['video_fn'].append(video)
        rows['speaker'].append(speaker)
    return pd.DataFrame(rows, columns=COLUMNS)


def split_table(tables, val_label='dev'):
    """3_2:28-47 over the per-video tables (videos sorted by name): all train rows, then all idle rows, then all validation rows"""
    import pandas as pd
    parts = [[], [], []]
    for df in tables:
        df = df.copy()
        df['dataset'] = split_labels(len(df), val_label)
        for i, lab in enumerate(('train', 'idle', val_label)):
            parts[i].append(df[df['dataset'] == lab])
    return pd.concat([pd.concat(p) for p in parts])


def write_split_csv(root_dir, speaker, tables):
    """processed_137.csv (label ``dev``: what GestureDataset and speaker_stats select) and clips.csv (``val``: the reference's file)"""
    base = os.path.join(root_dir, speaker)
    out = {}
    for name, label in (('processed_137.csv', 'dev'), ('clips.csv', 'val')):
        out[name] = os.path.join(base, name)
        split_table(tables, label).to_csv(out[name], index=False)
    return out


# ------------------------------------------------------------------------------------------------------------------------ the GPU

def _p(t):
    return C.c_void_p(t.data_ptr() if t.numel() else None)


class _Timer:
    """HIP-event time per stage, summed after the video's last kernel"""

    def __init__(self, stream):
        import torch
        self.torch, self.stream, self.spans = torch, stream, []

    def run(self, stage, fn):
        a, b = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        a.record(self.stream)
        fn()
        b.record(self.stream)
        self.spans.append((stage, a, b))

    def totals(self):
        out = {}
        for stage, a, b in self.spans:
            out[stage] = out.get(stage, 0.0) + a.elapsed_time(b)
        return out


def device_frame_stages(src, present, start_frame, num_frames, shoulder_chunks, timer=None):
    """the per-video pose stages up to the clip starts.  src (n, 3, 137) and present (n,) uint8 on the device ->
    dict(keep, dist, bad, prefix, dist_kept, means, starts (capacity), n_clips (device int32))"""
    import torch
    from . import _lib
    lib = _lib.load()
    dev, n = src.device, src.shape[0]
    raw = torch.cuda.current_stream(dev).cuda_stream
    esize = src.element_size()
    run = timer.run if timer is not None else (lambda stage, fn: fn())
    ws_bytes = lib.sdt_clip_workspace_bytes(n)
    n_cand = lib.sdt_clip_window_candidates(n, start_frame, num_frames, STEP)
    if ws_bytes < 0 or n_cand < 0:
        raise ValueError('unsupported frame count / start / window (%d, %d, %d)' % (n, start_frame, num_frames))
    o = {'keep': torch.empty(n, dtype=torch.int32, device=dev), 'dist': torch.empty(n, dtype=torch.float64, device=dev),
         'bad': torch.empty(n, dtype=torch.int32, device=dev), 'prefix': torch.empty(n + 1, dtype=torch.int32, device=dev),
         'dist_kept': torch.zeros(n, dtype=torch.float64, device=dev), 'means': torch.empty(shoulder_chunks, dtype=torch.float64, device=dev),
         'starts': torch.empty(max(n_cand, 1), dtype=torch.int32, device=dev), 'n_clips': torch.empty(1, dtype=torch.int32, device=dev)}
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
    run('flags', lambda: _lib.check(lib.sdt_clip_frame_flags(esize, _p(src), _p(present), n, _p(o['keep']), _p(o['dist']), _p(o['bad']), raw)))
    run('scan', lambda: _lib.check(lib.sdt_clip_scan(_p(o['keep']), _p(o['dist']), n, _p(o['prefix']), _p(o['dist_kept']), raw)))
    run('shoulder', lambda: _lib.check(lib.sdt_clip_shoulder_means(_p(o['dist_kept']), _p(o['prefix']), n, shoulder_chunks, _p(o['means']), raw)))
    run('windows', lambda: _lib.check(lib.sdt_clip_windows(_p(o['prefix']), n, start_frame, num_frames, STEP, _p(ws), ws.numel(),
                                                          _p(o['starts']), o['starts'].numel(), _p(o['n_clips']), raw)))
    return o


def _check_size(status):
    """as ``_lib.check``; the library's "unsupported size" status becomes a ValueError"""
    from . import _lib
    if status == -3:  # SDT_ERR_UNSUPPORTED
        raise ValueError('libsdt_hip: %s' % _lib.load().sdt_last_error().decode())
    _lib.check(status)


def device_repair(src, present, max_gap, despike=None, timer=None):
    """the repair stage of one video (section 26).  src (n, 3, 137) and present (n,) uint8 on the device, neither written ->
    dict(src_r, present_r (n,) uint8, valid, spike, filled (n, 137) uint8, repaired_per_frame (n,) int32).  The sizes are the
    library's to refuse: an unsupported max_gap, h or n is a ValueError"""
    import torch
    from . import _lib
    lib = _lib.load()
    dev, n = src.device, src.shape[0]
    h, kappa, floor_px = (0, 1.0, 0.0) if despike is None else (despike if len(despike) == 3 else tuple(despike) + (0.0,))
    if despike is not None and (not (np.isfinite(kappa) and kappa > 0) or not (np.isfinite(floor_px) and floor_px >= 0)):
        raise ValueError('despike kappa must be positive and floor_px not negative, both finite, not %r, %r' % (kappa, floor_px))
    if lib.sdt_clip_repair_workspace_bytes(n) < 0:
        raise ValueError('unsupported frame count %d' % n)
    raw = torch.cuda.current_stream(dev).cuda_stream
    esize = src.element_size()
    o = {'src_r': torch.empty_like(src), 'present_r': torch.empty(n, dtype=torch.uint8, device=dev),
         'valid': torch.empty((n, KP), dtype=torch.uint8, device=dev), 'spike': torch.empty((n, KP), dtype=torch.uint8, device=dev),
         'filled': torch.empty((n, KP), dtype=torch.uint8, device=dev), 'repaired_per_frame': torch.empty(n, dtype=torch.int32, device=dev)}

    def launch():
        _check_size(lib.sdt_clip_repair_valid(esize, _p(src), _p(present), n, int(h), float(kappa), float(floor_px), _p(o['valid']),
                                              _p(o['spike']), raw))
        _check_size(lib.sdt_clip_repair_fill(esize, _p(src), _p(present), _p(o['valid']), n, int(max_gap), _p(o['src_r']), _p(o['present_r']),
                                             _p(o['filled']), _p(o['repaired_per_frame']), raw))
    if timer is not None:
        timer.run('repair', launch)
    else:
        launch()
    return o


def device_retime(src, present, fps, mode='linear', min_support=0.75, timer=None):
    """the retime stage of one video (section 27).  src (n_src, 3, 137) and present (n_src,) uint8 on the device, recorded at ``fps``
    (an int, an (int, int) pair or 'P/Q'; never a float), neither written -> dict(src_t (n_out, 3, 137), present_t (n_out,) uint8,
    valid_t, taps_used (n_out, 137) uint8, nearest_src (n_out,) int32, counts (3,) int64: invalid source points, non-finite source
    points, invalid output points; and P, Q, phases, mode).  Sizes outside the library's limits are a ValueError"""
    import torch
    from . import _lib
    p, q = parse_fps(fps, 'fps')
    mode, min_support = retime_params(mode, min_support)
    lib = _lib.load()
    dev, n_src = src.device, src.shape[0]
    h = model_retime_taps(p, q, mode)
    ws_bytes = lib.sdt_clip_retime_workspace_bytes(n_src, p, q, h.shape[0], h.shape[1])
    if ws_bytes < 0:
        raise ValueError('unsupported source frame count %d at fps = %d/%d (1 to 2^30 frames, before and after retiming)' % (n_src, p, q))
    n_out = (n_src - 1) * (FPS * q) // p + 1
    raw = torch.cuda.current_stream(dev).cuda_stream
    taps = torch.from_numpy(h).to(dev)
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
    o = {'src_t': torch.empty((n_out, 3, KP), dtype=src.dtype, device=dev), 'present_t': torch.empty(n_out, dtype=torch.uint8, device=dev),
         'valid_t': torch.empty((n_out, KP), dtype=torch.uint8, device=dev), 'taps_used': torch.empty((n_out, KP), dtype=torch.uint8, device=dev),
         'nearest_src': torch.empty(n_out, dtype=torch.int32, device=dev), 'counts': torch.empty(3, dtype=torch.int64, device=dev)}

    def launch():
        _check_size(lib.sdt_clip_retime(src.element_size(), _p(src), _p(present), n_src, p, q, _p(taps), h.shape[0], h.shape[1], min_support,
                                        n_out, _p(o['src_t']), _p(o['present_t']), _p(o['valid_t']), _p(o['taps_used']), _p(o['nearest_src']),
                                        _p(o['counts']), _p(ws), ws.numel(), raw))
    if timer is not None:
        timer.run('retime', launch)
    else:
        launch()
    o.update(P=p, Q=q, phases=h.shape[0], mode=mode)
    return o


def device_repaired_per_clip(repaired_per_frame, starts, n_clips, num_frames):
    """-> (n_clips,) int32: the filled kept keypoints of each window"""
    import torch
    from . import _lib
    lib = _lib.load()
    dev, n = repaired_per_frame.device, repaired_per_frame.shape[0]
    out = torch.empty(n_clips, dtype=torch.int32, device=dev)
    if n_clips:
        ws = torch.empty(lib.sdt_clip_repair_workspace_bytes(n), dtype=torch.uint8, device=dev)
        _check_size(lib.sdt_clip_repair_clip_counts(_p(repaired_per_frame), n, _p(starts), n_clips, num_frames, _p(ws), ws.numel(), _p(out),
                                                    torch.cuda.current_stream(dev).cuda_stream))
    return out


def device_gather_poses(src, starts, n_clips, num_frames, scalar, scale_conf):
    """-> (n_clips, num_frames, 3, 137) in src's dtype"""
    import torch
    from . import _lib
    lib = _lib.load()
    out = torch.empty((n_clips, num_frames, 3, KP), dtype=src.dtype, device=src.device)
    if n_clips:
        _lib.check(lib.sdt_clip_gather_poses(src.element_size(), _p(src), src.shape[0], _p(starts), n_clips, num_frames, float(scalar),
                                             int(bool(scale_conf)), _p(out), out.numel(), torch.cuda.current_stream(src.device).cuda_stream))
    return out


def upload_pcm(pcm, device='cuda'):
    import torch
    return torch.from_numpy(np.ascontiguousarray(pcm).view(np.uint8).reshape(-1)).to(device)


def device_pcm_to_mono(pcm, first=0, device='cuda', raw=None):
    """wavfile.read's array (host; ``raw``: its bytes already on the device) -> float32 mono on the device, from source sample
    ``first`` on"""
    import torch
    from . import _lib
    lib = _lib.load()
    n = pcm.shape[0]
    ch = pcm.shape[1] if pcm.ndim == 2 else 1
    if first >= n:
        return torch.empty(0, dtype=torch.float32, device=device)
    if raw is None:
        raw = upload_pcm(pcm, device)
    out = torch.empty(n - first, dtype=torch.float32, device=device)
    _lib.check(lib.sdt_clip_pcm_to_mono_f32(_PCM_FMT[str(pcm.dtype)], _p(raw), n, ch, first, _p(out), out.numel(),
                                            torch.cuda.current_stream(out.device).cuda_stream))
    return out


def device_resample(x, sr_in, sr_out=SR):
    """float32 mono on the device at sr_in -> at sr_out (the same tensor when the rates are equal)"""
    import torch
    from . import _lib
    lib = _lib.load()
    if int(sr_in) == int(sr_out) or x.numel() == 0:
        return x
    up, down, taps, n_pre = design_taps(sr_in, sr_out)
    if lib.sdt_clip_resample_lds_bytes(len(taps), up, down) < 0:
        raise ValueError('unsupported sample rate %d (ratio %d/%d, %d taps)' % (sr_in, up, down, len(taps)))
    n_out = resampled_length(x.numel(), up, down)
    y = torch.empty(n_out, dtype=torch.float32, device=x.device)
    t = torch.from_numpy(taps).to(x.device)
    _lib.check(lib.sdt_clip_resample_f32(_p(x), x.numel(), _p(t), len(taps), up, down, n_pre, _p(y), n_out,
                                         torch.cuda.current_stream(x.device).cuda_stream))
    return y


def device_gather_audio(audio, a0, a1):
    """audio (float32, device), a0 / a1 sequences of slice bounds -> ((n_clips, L_max) zero-padded, lengths int32)"""
    import torch
    from . import _lib
    lib = _lib.load()
    dev, n = audio.device, len(a0)
    l_max = max(1, max((int(b) - int(a) for a, b in zip(a0, a1)), default=1))
    out = torch.zeros((n, l_max), dtype=torch.float32, device=dev)
    lengths = torch.zeros(n, dtype=torch.int32, device=dev)
    if n and audio.numel():
        t0 = torch.tensor(list(a0), dtype=torch.int64).to(dev)
        t1 = torch.tensor(list(a1), dtype=torch.int64).to(dev)
        _lib.check(lib.sdt_clip_gather_audio(_p(audio), audio.numel(), _p(t0), _p(t1), n, l_max, _p(out), out.numel(), _p(lengths),
                                             torch.cuda.current_stream(dev).cuda_stream))
    return out, lengths


def _speech_workspace(lib, n_samples, n_windows, dev):
    import torch
    ws_bytes = lib.sdt_clip_speech_workspace_bytes(int(n_samples), int(n_windows))
    if ws_bytes < 0:
        raise ValueError('unsupported track length / window count (%d samples, %d windows; at most 160 * 2^24 + 159 and 2^30)' % (n_samples, n_windows))
    return torch.empty(ws_bytes, dtype=torch.uint8, device=dev)


def device_hop_energy(audio):
    """audio (N,) float32 on the device -> (e (N // 160,) float64, flag (1,) int32: an energy is not finite); ``model_hop_energy``"""
    import torch
    from . import _lib
    lib = _lib.load()
    if audio.dtype != torch.float32 or audio.dim() != 1 or not audio.is_contiguous():
        raise ValueError('the track must be a contiguous 1-d float32 tensor')
    n = audio.numel()
    if lib.sdt_clip_speech_workspace_bytes(n, 0) < 0:
        raise ValueError('unsupported track length %d (at most 160 * 2^24 + 159 samples)' % n)
    e = torch.empty(n // HOP, dtype=torch.float64, device=audio.device)
    flag = torch.empty(1, dtype=torch.int32, device=audio.device)
    _check_size(lib.sdt_clip_speech_energy(_p(audio), n, _p(e), _p(flag), torch.cuda.current_stream(audio.device).cuda_stream))
    return e, flag


def device_speech_mask(energy, floor_pct, margin, abs_floor):
    """-> (active_raw (H,) uint8, stats (2,) float64 = floor, thr); ``model_floor`` and ``model_mask``"""
    import torch
    from . import _lib
    lib = _lib.load()
    dev, h = energy.device, energy.numel()
    ws = _speech_workspace(lib, min(h, MAX_HOPS) * HOP, 0, dev)
    raw = torch.empty(h, dtype=torch.uint8, device=dev)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    _check_size(lib.sdt_clip_speech_mask(_p(energy), h, int(floor_pct), float(margin), float(abs_floor), _p(raw), _p(stats), _p(ws), ws.numel(),
                                         torch.cuda.current_stream(dev).cuda_stream))
    return raw, stats


def device_speech_smooth(active_raw, min_run_hops, hang_hops):
    """-> active (H,) uint8; ``model_smooth``"""
    import torch
    from . import _lib
    lib = _lib.load()
    dev, h = active_raw.device, active_raw.numel()
    ws = _speech_workspace(lib, min(h, MAX_HOPS) * HOP, 0, dev)
    out = torch.empty(h, dtype=torch.uint8, device=dev)
    _check_size(lib.sdt_clip_speech_smooth(_p(active_raw), h, int(min_run_hops), int(hang_hops), _p(out), _p(ws), ws.numel(),
                                           torch.cuda.current_stream(dev).cuda_stream))
    return out


def device_speech_windows(active, n_samples, starts, offsets, min_permille):
    """active (H,) uint8 and starts (>= n int32, ascending) on the device, offsets [(a0, a1)] of the n candidate windows on the host ->
    dict(prefix (H + 1,), counts_all (n, 2), starts (n,), index (n,), counts (n, 2) int32: the first n_kept rows hold the kept windows,
    n_kept (1,) int32); ``model_window_counts`` and ``model_windows_kept``"""
    import torch
    from . import _lib
    lib = _lib.load()
    dev, h, n = active.device, active.numel(), len(offsets)
    if h != int(n_samples) // HOP:
        raise ValueError('%d hops do not belong to a track of %d samples' % (h, n_samples))
    ws = _speech_workspace(lib, n_samples, n, dev)
    a = torch.tensor([[int(a0), int(a1)] for a0, a1 in offsets], dtype=torch.int64).reshape(n, 2).t().contiguous().to(dev)
    o = {'prefix': torch.empty(h + 1, dtype=torch.int32, device=dev), 'counts_all': torch.empty((n, 2), dtype=torch.int32, device=dev),
         'starts': torch.empty(n, dtype=torch.int32, device=dev), 'index': torch.empty(n, dtype=torch.int32, device=dev),
         'counts': torch.empty((n, 2), dtype=torch.int32, device=dev), 'n_kept': torch.empty(1, dtype=torch.int32, device=dev)}
    _check_size(lib.sdt_clip_speech_windows(_p(active), h, int(n_samples), _p(starts), _p(a[0]) if n else None, _p(a[1]) if n else None, n,
                                            int(min_permille), _p(o['prefix']), _p(o['counts_all']), _p(o['starts']), _p(o['index']),
                                            _p(o['counts']), _p(o['n_kept']), _p(ws), ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
    return o


def device_speech_gate(audio, starts, offsets, params, timer=None):
    """the whole stage of section 28 on one video: audio (N,) float32 and starts (int32, ascending) on the device, offsets the windows'
    audio spans -> dict(energy, flag, active_raw, stats, active and ``device_speech_windows``' entries)"""
    margin, abs_floor = gate_constants(params)
    run = timer.run if timer is not None else (lambda stage, fn: fn())
    o = {}
    run('gate_energy', lambda: o.update(zip(('energy', 'flag'), device_hop_energy(audio))))
    run('gate_mask', lambda: o.update(zip(('active_raw', 'stats'), device_speech_mask(o['energy'], params['floor_pct'], margin, abs_floor))))
    run('gate_smooth', lambda: o.__setitem__('active', device_speech_smooth(o['active_raw'], params['min_run_hops'], params['hang_hops'])))
    run('gate_windows', lambda: o.update(device_speech_windows(o['active'], audio.numel(), starts, offsets, params['min_permille'])))
    return o


def build_clips(root_dir, speaker, start_frame=80, num_frames=64, shoulder_chunks=1, scale_confidence=None, write=True, device='cuda',
                repair_max_gap=0, despike=None, source_fps=None, retime='linear', retime_min_support=0.75, speech_gate=None):
    """-> {'videos': {name: summary}, 'table' (processed_137 order), 'timing'} and, with write=False, 'poses' (n_clips, num_frames, 3, 137),
    'audio' (n_clips, L_max), 'audio_lengths' (n_clips,) on the device in per-video, ascending-start order, with 'order' giving
    each table row's position in them.  ``repair_max_gap`` G >= 1 (with ``despike`` = (h, kappa, floor_px) or None) runs the repair
    stage of section 26 in front of the frame flags: each video's summary gains 'repair' and, with write=False, the result
    'repaired_per_clip' (n_clips,) int32; with 0 nothing new is launched.  ``source_fps`` (an int, an (int, int) pair or 'P/Q') says the
    keypoints were recorded at that rate and runs the retime stage of section 27 in front of everything else (``retime``: nearest, linear
    or smooth; ``retime_min_support``): every count and index is then in 15 fps frames, each video's summary gains 'retime', and a clip's
    ``imgs`` name the nearest source frames; with None, or a rate equal to 15, nothing new is launched.  ``speech_gate`` (a dict with
    'min_permille' and optionally margin_db, floor_pct, abs_dbfs, hang_hops, min_run_hops) runs the audio activity gate of section 28
    between the window search and the gathers: a window stays a clip only if that share of the 10 ms hops inside its audio span lie
    above the track's noise floor; each video's summary gains 'speech_gate', the result 'speech_counts' (n_clips, 2) int32 of (active
    hops, hops) with write=False, and tmp/activity/<video>.npz is written with write=True; with None nothing new is launched"""
    import torch
    from . import _lib
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('clips are built on the GPU (csrc/clip_builder.hip); there is no CPU fallback')
    _lib.load()
    if int(shoulder_chunks) < 1 or int(num_frames) < 1 or int(start_frame) < 0:
        raise ValueError('shoulder_chunks and num_frames must be at least 1, start_frame at least 0')
    repair = bool(repair_max_gap)
    if despike is not None and not repair:
        raise ValueError('despike needs repair_max_gap >= 1: a marked spike is repaired by the gap filling')
    if repair:
        repair_max_gap, despike = repair_params(repair_max_gap, despike)
    fps_pq = None
    if source_fps is not None:
        fps_pq = parse_fps(source_fps, 'source_fps')
        retime, retime_min_support = retime_params(retime, retime_min_support, ('retime', 'retime_min_support'))
    retiming = fps_pq is not None and fps_pq[0] != FPS * fps_pq[1]
    gate = None if speech_gate is None else speech_gate_params(speech_gate)
    plan = plan_clips(root_dir, speaker)
    first = next((p for v in plan for p in v['frames'].values()), None)
    if first is None:
        raise ValueError('no keypoint file under %s' % os.path.join(root_dir, speaker, 'tmp', 'raw_pose_2d'))
    np_dtype = np.load(first).dtype
    if np_dtype not in (np.float32, np.float64):
        raise ValueError('%s: dtype %s (float32 or float64 expected)' % (first, np_dtype))
    dtype = torch.float32 if np_dtype == np.float32 else torch.float64
    scale_conf = scales_confidence(shoulder_chunks, scale_confidence)
    base = os.path.join(root_dir, speaker)
    if write:
        os.makedirs(os.path.join(base, 'clips', 'npz'), exist_ok=True)
        os.makedirs(os.path.join(base, 'tmp', 'intermediate_csv'), exist_ok=True)
        if gate is not None:
            os.makedirs(os.path.join(base, 'tmp', 'activity'), exist_ok=True)
    st = torch.cuda.current_stream(dev)
    pool = ThreadPoolExecutor(max_workers=MAX_READ_THREADS)
    summary, tables, all_poses, all_audio, all_len, all_rep, all_gate = {}, [], [], [], [], [], []
    t_all = time.perf_counter()
    try:
        for video in plan:
            name, n = video['video'], video['n_frames']
            if not video['frames']:
                raise ValueError('%s: no kept frame (the directory is empty)' % video['dir'])
            t0 = time.perf_counter()
            src_host, present = _read_frames(video, dtype, pool)
            sr_in, pcm = _read_wav(video['wav'])
            t_read = time.perf_counter() - t0
            timer = _Timer(st)
            src = src_host.to(dev, non_blocking=True)
            present_dev = torch.from_numpy(present).to(dev)
            rt = None
            if retiming:  # from here on every frame index is a 15 fps frame
                rt = device_retime(src, present_dev, fps_pq, retime, retime_min_support, timer)
                src, present_dev, n = rt['src_t'], rt['present_t'], rt['src_t'].shape[0]
                present = rt['present_t'].cpu().numpy()
                nearest = rt['nearest_src'].cpu().numpy()
            if repair:
                o0 = device_frame_stages(src, present_dev, start_frame, num_frames, shoulder_chunks)  # what the unrepaired tracks give
                rep = device_repair(src, present_dev, repair_max_gap, despike, timer)
                src, present_dev = rep['src_r'], rep['present_r']
            o = device_frame_stages(src, present_dev, start_frame, num_frames, shoulder_chunks, timer)
            n_clips = int(o['n_clips'].item())  # (synchronises)
            bad = o['bad'].cpu().numpy()
            if bad.any():
                f_bad = int(np.flatnonzero(bad)[0])
                raise ValueError('%s: non-finite keypoint coordinates' % video['frames'].get(f_bad, '%s frame %d' % (video['dir'], f_bad)))
            n_kept = int(o['prefix'][n].item())
            if n_kept == 0:
                raise ValueError('%s: no kept frame (every frame is an outlier)' % video['dir'])
            means = o['means'].cpu().numpy()
            mean = np.average(means, axis=0)
            if not mean > 0:
                raise ValueError('%s: mean shoulder distance %r over %d kept frames in %d chunk(s); cannot rescale'
                                 % (video['dir'], float(mean), n_kept, shoulder_chunks))
            scalar = float(OLIVER_SHOULDER * 1.0 / mean)
            starts = o['starts'][:n_clips].cpu().numpy().astype(np.int64)
            starts_dev, n_windows = o['starts'], n_clips  # (the windows the keypoints allow)
            holder = {}
            if gate is None:
                timer.run('gather_poses', lambda: holder.__setitem__('poses', device_gather_poses(src, o['starts'], n_clips, num_frames, scalar, scale_conf)))
            cut = source_cut(start_frame, sr_in)
            raw_pcm = upload_pcm(pcm, dev)
            timer.run('pcm', lambda: holder.__setitem__('mono', device_pcm_to_mono(pcm, cut, dev, raw_pcm)))
            timer.run('resample', lambda: holder.__setitem__('audio', device_resample(holder['mono'], sr_in)))
            offs = [audio_offsets(int(s), start_frame, num_frames) for s in starts]
            if gate is not None:  # the gate reads the resampled track, so the poses are gathered behind it, for the kept windows only
                sg = device_speech_gate(holder['audio'], o['starts'], offs, gate, timer)
                n_clips = int(sg['n_kept'].item())  # (synchronises)
                if int(sg['flag'].item()):
                    raise ValueError('%s: non-finite audio samples (a hop energy is not finite)' % video['wav'])
                index = sg['index'][:n_clips].cpu().numpy()
                starts_all, starts, offs, starts_dev = starts, starts[index], [offs[i] for i in index], sg['starts']
                timer.run('gather_poses', lambda: holder.__setitem__('poses', device_gather_poses(src, starts_dev, n_clips, num_frames, scalar, scale_conf)))
            timer.run('gather_audio', lambda: holder.__setitem__('clips', device_gather_audio(holder['audio'], [a for a, _ in offs], [b for _, b in offs])))
            torch.cuda.synchronize(dev)
            poses, (audio, lengths) = holder['poses'], holder['clips']
            n_present = int(present.sum())
            rep_summary = None
            if repair:
                per_clip = device_repaired_per_clip(rep['repaired_per_frame'], starts_dev, n_clips, num_frames)
                host = {k: rep[k].cpu().numpy() for k in ('filled', 'spike', 'present_r')}
                n0 = int(o0['n_clips'].item())
                rep_summary = model_repair_summary(present, o0['keep'].cpu().numpy(), o['keep'].cpu().numpy(), host,
                                                   range(n0), range(n_windows), per_clip.cpu().numpy(), num_frames)
                n_present = int(host['present_r'].sum())  # (the files and the frames the stage gave back)
                if not write:
                    all_rep.append(per_clip)
            table = video_table(speaker, name, starts, num_frames)
            tables.append(table)
            t_write = 0.0
            if write:
                t0 = time.perf_counter()
                ph, ah, lh = poses.cpu().numpy(), audio.cpu().numpy(), lengths.cpu().numpy()

                def save(i):
                    np.savez(os.path.join(base, table['pose_fn'].iloc[i]), pose=ph[i],
                             imgs=frame_image_paths(root_dir, speaker, name, int(starts[i]), num_frames, nearest if retiming else None),
                             audio=ah[i, :lh[i]])
                for f in [pool.submit(save, i) for i in range(n_clips)]:
                    f.result()
                table.to_csv(os.path.join(base, 'tmp', 'intermediate_csv', 'tmp_%s.csv' % name), index=False)
                if gate is not None:
                    np.savez(os.path.join(base, 'tmp', 'activity', name + '.npz'), energy=sg['energy'].cpu().numpy(),
                             active_raw=sg['active_raw'].cpu().numpy(), active=sg['active'].cpu().numpy(), starts_all=starts_all,
                             counts_all=sg['counts_all'].cpu().numpy())
                t_write = time.perf_counter() - t0
            else:
                all_poses.append(poses)
                all_audio.append(audio)
                all_len.append(lengths)
            labels = split_labels(n_clips)
            summary[name] = {'frames': n, 'missing': n - int(present.sum()), 'kept': n_kept, 'dropped': n - n_kept, 'outliers': n_present - n_kept,
                             'shoulder_dropped': n_kept - (n_kept // shoulder_chunks) * shoulder_chunks, 'scalar': scalar,
                             'scale_confidence': scale_conf, 'sample_rate': sr_in, 'audio_samples': int(holder['audio'].numel()),
                             'clips': {lab: labels.count(lab) for lab in ('train', 'idle', 'dev')},
                             'timing': {'kernel_ms': timer.totals(), 'read_s': t_read, 'write_s': t_write}}
            if repair:
                summary[name]['repair'] = rep_summary
            if gate is not None:
                n_hops = sg['energy'].numel()
                floor, thr = (float(v) for v in sg['stats'].cpu().numpy()) if n_hops else (None, None)
                summary[name]['speech_gate'] = speech_gate_summary(n_hops, int(sg['active_raw'].sum().item()), int(sg['active'].sum().item()),
                                                                   floor, thr, n_windows, n_clips)
                if not write:
                    all_gate.append(sg['counts'][:n_clips])
            if retiming:
                summary[name]['retime'] = model_retime_summary({'counts': rt['counts'].cpu().numpy(), 'nearest_src': nearest},
                                                               video['n_frames'], fps_pq[0], fps_pq[1], retime)
    finally:
        pool.shutdown()
    import pandas as pd
    offsets = np.cumsum([0] + [len(t) for t in tables])
    tagged = [t.assign(_pos=np.arange(offsets[i], offsets[i + 1])) for i, t in enumerate(tables)]
    full = split_table(tagged, 'dev')
    out = {'videos': summary, 'table': full[COLUMNS].reset_index(drop=True), 'order': full['_pos'].to_numpy().astype(np.int64),
           'dtype': str(np_dtype), 'timing': {'total_s': time.perf_counter() - t_all}}
    if write:
        out['files'] = write_split_csv(root_dir, speaker, tables)
    else:
        l_max = max([a.shape[1] for a in all_audio] + [1])
        out['poses'] = torch.cat(all_poses) if all_poses else torch.empty((0, num_frames, 3, KP), dtype=dtype, device=dev)
        out['audio'] = torch.cat([torch.nn.functional.pad(a, (0, l_max - a.shape[1])) for a in all_audio])
        out['audio_lengths'] = torch.cat(all_len)
        if repair:
            out['repaired_per_clip'] = torch.cat(all_rep)
        if gate is not None:
            out['speech_counts'] = torch.cat(all_gate) if all_gate else torch.empty((0, 2), dtype=torch.int32, device=dev)
    assert isinstance(out['table'], pd.DataFrame)
    return out


def add_repair_options(ap):
    ap.add_argument('--repair-max-gap', type=int, default=0, metavar='G',
                    help='fill gaps of at most G (1..64) frames in a keypoint track by interpolation, confidence 0 (0: off)')
    ap.add_argument('--despike', nargs='+', type=float, default=None, metavar=('H', 'KAPPA'),
                    help='H KAPPA [FLOOR_PX]: mark a point more than KAPPA * 1.4826 * MAD + FLOOR_PX from the median of frames -H..H (H in 1..3) '
                         'of its track and fill it like a gap (needs --repair-max-gap)')


def add_retime_options(ap):
    ap.add_argument('--source-fps', default=None, metavar='P[/Q]',
                    help="the rate the keypoints were recorded at, as an exact fraction (25, 30, 30000/1001): they are retimed onto the 15 fps "
                         "grid first (default: they are 15 fps already)")
    ap.add_argument('--retime', choices=RETIME_MODES, default='linear',
                    help='how: the nearest source frame, interpolation between the two neighbours, or a raised-cosine low-pass (with --source-fps)')
    ap.add_argument('--retime-min-support', type=float, default=0.75, metavar='S',
                    help='a retimed point is kept if the valid source points under its taps carry at least S of their weight (0 < S <= 1)')


def add_speech_gate_options(ap):
    d = GATE_DEFAULTS
    ap.add_argument('--speech-gate', type=int, default=None, metavar='PERMILLE',
                    help='keep a window only if at least PERMILLE (1..1000) thousandths of the 10 ms hops in its audio span lie above the '
                         "track's noise floor (section 28; it measures audio energy, not speech: music passes; default: off)")
    ap.add_argument('--gate-margin-db', type=float, default=d['margin_db'], metavar='DB', help='a hop is active this far above the floor (0..60)')
    ap.add_argument('--gate-floor-pct', type=int, default=d['floor_pct'], metavar='PCT',
                    help='the floor is the hop energy at this percentile of the track (0..50)')
    ap.add_argument('--gate-abs-dbfs', type=float, default=d['abs_dbfs'], metavar='DBFS',
                    help='no hop below this mean square level is active, whatever the floor (-120..0)')
    ap.add_argument('--gate-hang-ms', type=int, default=10 * d['hang_hops'], metavar='MS',
                    help='an inactive stretch of at most MS between active hops counts as active (a multiple of 10, at most 10240; 0: off)')
    ap.add_argument('--gate-min-ms', type=int, default=10 * d['min_run_hops'], metavar='MS',
                    help='an active stretch shorter than MS is dropped first (a multiple of 10, at most 10240; 0: off)')


def speech_gate_option(a, default_permille=None):
    """the parsed ``add_speech_gate_options`` arguments -> build_clips' ``speech_gate`` (without --speech-gate: None, or the --gate-*
    values with ``default_permille`` where one is given)"""
    if a.speech_gate is None and default_permille is None:
        return None
    return speech_gate_params({'min_permille': default_permille if a.speech_gate is None else a.speech_gate, 'margin_db': a.gate_margin_db, 'floor_pct': a.gate_floor_pct,
                               'abs_dbfs': a.gate_abs_dbfs, 'hang_hops': gate_ms_to_hops(a.gate_hang_ms, '--gate-hang-ms'),
                               'min_run_hops': gate_ms_to_hops(a.gate_min_ms, '--gate-min-ms')})


def activity_report(wav, gate=None, device='cuda'):
    """the hop statistics of one wav from its first sample on, without building anything -> the ``speech_gate`` summary (no windows)"""
    import torch
    params = speech_gate_params(gate if gate is not None else {'min_permille': 500})
    sr_in, pcm = _read_wav(wav)
    audio = device_resample(device_pcm_to_mono(pcm, 0, torch.device(device)), sr_in)
    sg = device_speech_gate(audio, torch.empty(0, dtype=torch.int32, device=audio.device), [], params)
    if int(sg['flag'].item()):
        raise ValueError('%s: non-finite audio samples (a hop energy is not finite)' % wav)
    n_hops = sg['energy'].numel()
    floor, thr = (float(v) for v in sg['stats'].cpu().numpy()) if n_hops else (None, None)
    return speech_gate_summary(n_hops, int(sg['active_raw'].sum().item()), int(sg['active'].sum().item()), floor, thr, 0, 0)


def _gate_text(g):
    if not g['hops']:
        return 'no audio hop'
    return '%d of %d hops active (%d before smoothing), floor %.1f dB, threshold %.1f dB%s' % (
        g['active'], g['hops'], g['active_raw'], g['floor_db'], g['thr_db'], '' if g['note'] is None else '; NOTE: ' + g['note'])


def despike_option(ap, values):
    if values is None:
        return None
    if len(values) not in (2, 3) or values[0] != int(values[0]):
        ap.error('--despike takes H KAPPA [FLOOR_PX] with an integer H')
    return (int(values[0]),) + tuple(values[1:]) + ((0.0,) if len(values) == 2 else ())


def main(argv=None):
    ap = argparse.ArgumentParser(description="a speaker's clips on the GPU from per-frame keypoints and one wav per video (the reference's "
                                             "2_2, 2_3, 3_1 and 3_2) -> clips/npz, processed_137.csv, clips.csv")
    ap.add_argument('--root', default=None, help='dataset root (DATASET.ROOT_DIR)')
    ap.add_argument('--speaker', default=None)
    ap.add_argument('--start-frame', type=int, default=80, help="frames before it are dropped (3_1's -fi)")
    ap.add_argument('--frames', type=int, default=64, help='frames per clip (DATASET.NUM_FRAMES)')
    ap.add_argument('--shoulder-chunks', type=int, default=1, help="chunks of the shoulder-distance mean (2_3's -np)")
    ap.add_argument('--no-write', action='store_true', help='build on the device and print the summary only')
    add_repair_options(ap)
    add_retime_options(ap)
    add_speech_gate_options(ap)
    ap.add_argument('--activity-report', default=None, metavar='WAV',
                    help="print the gate's hop statistics of one wav (with the --gate-* options) and build nothing")
    a = ap.parse_args(argv)
    try:
        gate = speech_gate_option(a, 500 if a.activity_report is not None else None)  # (the report counts no window: any share will do)
    except ValueError as e:
        ap.error(str(e))
    if a.activity_report is not None:
        print('%s: %s' % (a.activity_report, _gate_text(activity_report(a.activity_report, gate))))
        return 0
    if a.root is None or a.speaker is None:
        ap.error('the following arguments are required: --root, --speaker')
    res = build_clips(a.root, a.speaker, start_frame=a.start_frame, num_frames=a.frames, shoulder_chunks=a.shoulder_chunks, write=not a.no_write,
                      repair_max_gap=a.repair_max_gap, despike=despike_option(ap, a.despike), source_fps=a.source_fps, retime=a.retime,
                      retime_min_support=a.retime_min_support, speech_gate=gate)
    for name, s in res['videos'].items():
        k = s['timing']
        r = s.get('repair')
        fixed = '' if r is None else (', repair filled %d points, %d spikes (%d not filled), %d frames recovered (%d without a file), clips %d -> %d, '
                                      'largest repaired share of a clip %.4f'
                                      % (r['points_filled'], r['spikes'], r['spikes_unfilled'], r['frames_recovered'], r['missing_recovered'],
                                         r['clips_without_repair'], r['clips_with_repair'], r['max_repaired_share']))
        t = s.get('retime')
        if t is not None:
            fixed += ', source %s fps: %d -> %d frames (%s, %d of %d retimed points invalid)' % (
                '%d/%d' % (t['P'], t['Q']) if t['Q'] != 1 else '%d' % t['P'], t['source_frames'], t['frames'], t['mode'],
                t['points_invalid_out'], t['frames'] * KP)
        g = s.get('speech_gate')
        if g is not None:
            fixed += ', speech gate: %s, %s' % (_gate_text(g), g['clips'])
        print('video %s: %d frames, %d kept, %d dropped (%d missing), %d shoulder frames dropped by chunking, scalar %.9g, clips %d train / '
              '%d idle / %d dev (%.2f s reading, kernels %.3f ms, %.2f s writing)%s'
              % (name, s['frames'], s['kept'], s['dropped'], s['missing'], s['shoulder_dropped'], s['scalar'], s['clips']['train'],
                 s['clips']['idle'], s['clips']['dev'], k['read_s'], sum(k['kernel_ms'].values()), k['write_s'], fixed))
    print('speaker %s: %d clips in %.2f s%s' % (a.speaker, len(res['table']), res['timing']['total_s'],
                                                '' if a.no_write else ' -> ' + res['files']['processed_137.csv']))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
