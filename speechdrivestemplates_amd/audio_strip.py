"""The audio under the gestures: a band below every rendered picture with the waveform envelope, the onset and motion-beat marks of
sync_metrics, the mel spectrogram the audio encoder sees and, in videos, a playhead.  (SYS.AUDIO_STRIP)

The band is appended below the canvas: (n, H, W, 3) frames become (n, H + S, W, 3), and the first H rows of every image keep their bytes.
From the top of the band (``lanes``): a waveform lane of Sw = 3 S // 8 rows, three mark lanes of 8 rows (audio onsets, beats of the
prediction, beats of the ground truth), a mel lane of Sm = S - Sw - 24 rows.  The time base needs 16000 samples/s and 15 frames/s.

    columns    a host table ``bounds`` (Nc + 1,) of start samples; column c covers [max(bounds[c], 0), min(bounds[c + 1], L)).
               ``uniform_bounds``: spc = ceil(min(L, span) / W) samples per column, bounds[c] = c spc, Nc = ceil(L / spc); frame t has its
               playhead at column (t * 16000 // 15) // spc; with L <= span the band stands still, else it scrolls with the playhead at W // 2.
               ``long_image_bounds``: column x between the centres cx_j = x0_j + 480 of two windows of render.long_image_layout starts at
               sample s_j + ((x - cx_j) (s_j+1 - s_j)) // (cx_j+1 - cx_j), s_j = (8 j * 16000) // 15; left of the first and right of the
               last centre the neighbouring slope goes on.
    envelope   per column the min and max of its finite samples and a flag (EMPTY, NONFINITE, OK); the recording's peak max |x|.
    waveform   sample x sits in row clamp(floor((1 - x g) (Sw - 1) / 2 + 0.5)), g = 1 / max(peak, 2^-15), float64, every operation rounded
               on its own; an OK column is WAVE from the row of its max to the row of its min; a NONFINITE column is WARNING over the lane.
    marks      tick k of 1/300 s is at sample k * 16000 // 300: MARKS[lane] in the column that holds it and the next one (TICK_WIDTH = 2).
    mel        pixel (y, c): frame min(max((bounds[c] + bounds[c + 1]) // 2, 0) // 160, F - 1), bin (n_mels (Sm - 1 - y)) // Sm; the colour
               is COLORMAP[number of i in 1 .. 255 with p >= fl32(ref * k[i])], k[i] = fl32(10 ** ((i / 255 - 1) db_range / 10)), ref = the
               piece's largest finite power; a non-finite power is WARNING.  EMPTY columns are BACKGROUND in every lane.
    compose    row H + y of image i is row y of the band, columns [c0[i], c0[i] + W), BACKGROUND outside [0, Nc), PLAYHEAD over the
               columns [ph[i] - c0[i], + PLAYHEAD_WIDTH) unless ph[i] is -1.

Two routes run the same operations in the same order: ``envelope_model`` / ``raster_model`` / ``compose_model`` are the contract in numpy;
``strip_for_clip`` and ``strip_for_long_image`` run csrc/audio_strip.hip on CUDA tensors.  There is no CPU fallback.

    python -m speechdrivestemplates_amd.audio_strip RESULTS.npz AUDIO.wav|.npy OUT_PREFIX [--row R] [--pair] [--height S] [--span s]
                                                    [--no-marks] [--long-image]

reads ``poses_pred_batch`` (and, with --pair, ``poses_gt_batch``) of a results npz (a validation file, or the DEMO file of a long-form run),
row R, draws it with render.py, puts the band of that row's audio under it and writes OUT_PREFIX.avi (Motion-JPEG with the audio: no
ffmpeg) and, with --long-image, OUT_PREFIX.jpg; it prints the onset / beat counts and the number of non-finite columns.
"""
import ctypes as C

import numpy as np

SAMPLE_RATE, FPS, HOP, TICKS = 16000, 15, 160, 300
EMPTY, NONFINITE, OK = 0, 1, 2  # SDT_STRIP_EMPTY / _NONFINITE / _OK
MARK_LANES, MARK_ROWS, TICK_WIDTH, PLAYHEAD_WIDTH = 3, 8, 2, 2  # SDT_STRIP_MARK_LANES, ...
MIN_HEIGHT, MAX_HEIGHT, MAX_COLUMNS = 64, 1024, 1 << 24
PEAK_FLOOR = 2.0 ** -15
# colours, BGR like the renderer's frames
BACKGROUND, WAVE, WARNING, PLAYHEAD = (24, 24, 24), (230, 200, 120), (0, 0, 255), (255, 255, 255)
MARKS = ((0, 220, 255), (80, 220, 80), (255, 160, 60))  # onsets: yellow; beats of the prediction: green; of the ground truth: blue
_NO_GPU = 'the audio strip is drawn on the GPU (csrc/audio_strip.hip); there is no CPU fallback (the *_model functions are the numpy contract)'


def colormap():
    """(256, 3) uint8 BGR, black - red - yellow - white by an integer formula: R = min(3 i, 255), G = clamp(3 i - 255), B = clamp(3 i - 510)"""
    i = np.arange(256, dtype=np.int64)
    r, g, b = np.clip(3 * i, 0, 255), np.clip(3 * i - 255, 0, 255), np.clip(3 * i - 510, 0, 255)
    return np.ascontiguousarray(np.stack([b, g, r], 1).astype(np.uint8))


def factor_table(db_range=80.0):
    """k[i] = float32(10 ** ((i / 255 - 1) * db_range / 10)), i = 1 .. 255, ascending, k[255] = 1 (computed on the host in float64)"""
    db_range = float(db_range)
    if not 0 < db_range < float('inf'):
        raise ValueError('db_range must be a finite number > 0, got %r' % (db_range,))
    i = np.arange(1, 256, dtype=np.float64)
    return np.ascontiguousarray((10.0 ** ((i / 255.0 - 1.0) * db_range / 10.0)).astype(np.float32))


def lanes(S):
    """the band's row partition -> (Sw, first mark row, first mel row, Sm)"""
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not MIN_HEIGHT <= S <= MAX_HEIGHT:
        raise ValueError('the band height must be an integer in [%d, %d], got %r' % (MIN_HEIGHT, MAX_HEIGHT, S))
    Sw = 3 * int(S) // 8
    return Sw, Sw, Sw + MARK_LANES * MARK_ROWS, int(S) - Sw - MARK_LANES * MARK_ROWS


def tick_sample(k):
    return int(k) * SAMPLE_RATE // TICKS


# ---- layouts (host side, Python integers) ---------------------------------------------------------------------------------------------------
def span_samples(span_s):
    return int(np.floor(float(span_s) * SAMPLE_RATE + 0.5))


def uniform_bounds(L, W, span):
    """the layout of a video of width W over L samples with at most ``span`` samples in view -> (bounds (Nc + 1,) int64, spc, Nc, scrolls)"""
    L, W, span = int(L), int(W), int(span)
    if L < 1 or W < 1 or span < 1:
        raise ValueError('samples, width and span must be positive, got %d, %d, %d' % (L, W, span))
    spc = -(-min(L, span) // W)
    Nc = -(-L // spc)
    if Nc > MAX_COLUMNS:
        raise ValueError('%d samples at %d per column are %d columns, more than %d' % (L, spc, Nc, MAX_COLUMNS))
    return np.array([c * spc for c in range(Nc + 1)], dtype=np.int64), spc, Nc, L > span


def frame_tables(n, W, spc, Nc, scrolls):
    """per frame t < n the band's first column and the playhead's global column -> (c0 (n,) int32, ph (n,) int32; -1 = no playhead).  The
    playhead of frame t is at column (t * 16000 // 15) // spc; a standing band starts at column 0, a scrolling one keeps the playhead at
    W // 2; a playhead that would fall outside the picture is left out."""
    c0, ph = [], []
    for t in range(int(n)):
        p = (t * SAMPLE_RATE // FPS) // spc
        first = p - W // 2 if scrolls else 0
        c0.append(first)
        ph.append(p if 0 <= p - first < W else -1)
    return np.array(c0, dtype=np.int32), np.array(ph, dtype=np.int32)


def long_image_bounds(T, L):
    """the layout under render.render_long_image of T poses: (width + 1,) int64 column start samples; they are not clipped to the L samples
    of the recording (the envelope does that), L is only checked"""
    from .render import LONG_STEP, LONG_W, long_image_layout
    T, L = int(T), int(L)
    if T < 1 or L < 1:
        raise ValueError('frames and samples must be positive, got %d and %d' % (T, L))
    width, windows = long_image_layout(T)
    n = max(len(windows), 2)  # one window: the slope to where the next one would stand
    cx = [int(j * LONG_STEP) + LONG_W // 2 for j in range(n)]
    s = [(8 * j * SAMPLE_RATE) // FPS for j in range(n)]
    assert all(x0 + LONG_W // 2 == cx[j] and i == 8 * j for j, (i, x0) in enumerate(windows))
    out, j = [], 0
    for x in range(width + 1):
        while j + 2 < n and x >= cx[j + 1]:
            j += 1
        out.append(s[j] + ((x - cx[j]) * (s[j + 1] - s[j])) // (cx[j + 1] - cx[j]))
    return np.array(out, dtype=np.int64)


# ---- the numpy contract models ----------------------------------------------------------------------------------------------------------------
def _order_key(bits):
    """uint32 bit patterns of float32 -> uint32 keys that ascend with the value, -0 below +0"""
    bits = bits.astype(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def _key_bits(key):
    key = np.uint32(key)
    return np.uint32(key & np.uint32(0x7fffffff)) if key & np.uint32(0x80000000) else np.uint32(~key)


def _bounds(bounds):
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.int64))
    if b.ndim != 1 or b.size < 2 or b.size - 1 > MAX_COLUMNS or (b[1:] < b[:-1]).any():
        raise ValueError('bounds must be an ascending table of Nc + 1 >= 2 column start samples')
    return b


def envelope_model(audio, bounds):
    """audio (L,) float32, bounds (Nc + 1,) -> {'env': (Nc, 2) float32 min / max, 'flags': (Nc,) int32, 'peak': float32, 'nonfinite': int}"""
    x = np.ascontiguousarray(np.asarray(audio, dtype=np.float32))
    if x.ndim != 1 or x.size < 1:
        raise ValueError('one recording is (L,) with L >= 1, got %s' % (x.shape,))
    b = _bounds(bounds)
    bits = x.view(np.uint32)
    fin = (bits & np.uint32(0x7f800000)) != np.uint32(0x7f800000)
    mag = bits[fin] & np.uint32(0x7fffffff)
    peak = np.uint32(mag.max() if mag.size else 0).reshape(1).view(np.float32)[0]
    Nc = b.size - 1
    env, flags = np.zeros((Nc, 2), dtype=np.uint32), np.zeros(Nc, dtype=np.int32)
    for c in range(Nc):
        lo, hi = max(int(b[c]), 0), min(int(b[c + 1]), x.size)
        if lo >= hi:
            flags[c] = EMPTY
            continue
        f = fin[lo:hi]
        flags[c] = OK if f.all() else NONFINITE
        if f.any():
            keys = _order_key(bits[lo:hi][f])
            env[c] = _key_bits(keys.min()), _key_bits(keys.max())
    return {'env': env.view(np.float32), 'flags': flags, 'peak': peak, 'nonfinite': int((~fin).sum())}


def wave_rows(x, peak, Sw):
    """the lane row of samples x (float32 values): float64, every operation rounded on its own"""
    g = np.float64(1.0) / np.float64(max(np.float64(peak), PEAK_FLOOR))
    a = np.asarray(x, dtype=np.float32).astype(np.float64) * g
    t = np.floor(((np.float64(1.0) - a) * np.float64(Sw - 1)) / np.float64(2.0) + np.float64(0.5))
    return np.clip(t, 0.0, float(Sw - 1)).astype(np.int64)


def mel_ref(mel):
    """the largest finite power, at least +0 (float32)"""
    bits = np.ascontiguousarray(np.asarray(mel, dtype=np.float32)).view(np.uint32).ravel()
    ok = ((bits & np.uint32(0x7f800000)) != np.uint32(0x7f800000)) & ((bits & np.uint32(0x80000000)) == 0)
    return np.uint32(bits[ok].max() if ok.any() else 0).reshape(1).view(np.float32)[0]


def _ticks(marks):
    """None, or up to three lists of ticks (None: absent) -> three int32 arrays"""
    marks = [] if marks is None else list(marks)
    if len(marks) > MARK_LANES:
        raise ValueError('at most %d tick lists (onsets, beats of the prediction, beats of the ground truth), got %d' % (MARK_LANES, len(marks)))
    out = []
    for m in marks + [None] * (MARK_LANES - len(marks)):
        m = np.zeros(0, dtype=np.int64) if m is None else np.asarray(m).reshape(-1).astype(np.int64)
        if m.size and (m.min() < -2 ** 31 or m.max() >= 2 ** 31):
            raise ValueError('ticks must fit 32 bits')
        out.append(np.ascontiguousarray(m.astype(np.int32)))
    return out


def raster_model(envelope, bounds, mel, S, marks=None, db_range=80.0):
    """the band (S, Nc, 3) uint8 BGR from ``envelope`` (an envelope_model result, or the device route's arrays under the same names), the
    column table, the power mel (n_mels, F) float32 and up to three tick lists"""
    b = _bounds(bounds)
    Nc = b.size - 1
    Sw, y_mark, y_mel, Sm = lanes(S)
    mel = np.ascontiguousarray(np.asarray(mel, dtype=np.float32))
    if mel.ndim != 2 or mel.shape[0] < 1 or mel.shape[1] < 1:
        raise ValueError('the mel must be (n_mels, F), got %s' % (mel.shape,))
    n_mels, F = mel.shape
    env, flags = np.asarray(envelope['env'], dtype=np.float32), np.asarray(envelope['flags'])
    band = np.empty((S, Nc, 3), dtype=np.uint8)
    band[:] = BACKGROUND
    # waveform lane
    r_top, r_bottom = wave_rows(env[:, 1], envelope['peak'], Sw), wave_rows(env[:, 0], envelope['peak'], Sw)
    y = np.arange(Sw)[:, None]
    bar = (flags == OK)[None, :] & (y >= r_top[None, :]) & (y <= r_bottom[None, :])
    band[:Sw][bar] = WAVE
    band[:Sw, flags == NONFINITE] = WARNING
    # mark lanes
    for q, ticks in enumerate(_ticks(marks)):
        hit = np.zeros(Nc, dtype=bool)
        for k in ticks:
            s = tick_sample(k)
            if k < 0 or s < b[0] or s >= b[Nc]:
                continue
            c = int(np.searchsorted(b, s, side='right')) - 1  # the column that holds the sample: bounds[c] <= s < bounds[c + 1]
            hit[c:c + TICK_WIDTH] = True
        band[y_mark + q * MARK_ROWS:y_mark + (q + 1) * MARK_ROWS, hit] = MARKS[q]
    # mel lane
    mid = np.maximum((b[:-1] + b[1:]) // 2, 0)
    j = np.minimum(mid // HOP, F - 1)
    m = (n_mels * (Sm - 1 - np.arange(Sm))) // Sm
    p = mel[m][:, j]  # (Sm, Nc)
    thresholds = mel_ref(mel) * factor_table(db_range)  # one float32 multiply each
    assert thresholds.dtype == np.float32
    index = np.searchsorted(thresholds, p.ravel(), side='right').reshape(p.shape)  # the number of thresholds <= p
    finite = np.isfinite(p)
    lane = colormap()[np.where(finite, index, 0)]
    lane[~finite] = WARNING
    lane[:, flags == EMPTY] = BACKGROUND
    band[y_mel:] = lane
    return band


def compose_model(frames, band, c0, ph):
    """frames (n, H, W, 3) uint8, band (S, Nc, 3), per image the band's first column and the playhead's global column (-1: none)
    -> (n, H + S, W, 3) uint8"""
    frames, band = np.asarray(frames, dtype=np.uint8), np.asarray(band, dtype=np.uint8)
    n, H, W, _ = frames.shape
    S, Nc, _ = band.shape
    out = np.empty((n, H + S, W, 3), dtype=np.uint8)
    out[:, :H] = frames
    out[:, H:] = BACKGROUND
    for i in range(n):
        first = int(c0[i])
        a, b = max(first, 0), min(first + W, Nc)
        if a < b:
            out[i, H:, a - first:b - first] = band[:, a:b]
        if ph[i] >= 0:
            p = int(ph[i]) - first
            a, b = max(p, 0), min(p + PLAYHEAD_WIDTH, W)
            if a < b:
                out[i, H:, a:b] = PLAYHEAD
    return out


# ---- the device route (csrc/audio_strip.hip) -----------------------------------------------------------------------------------------------
def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _bytes3(colours):
    return (C.c_uint8 * (3 * len(colours)))(*[v for c in colours for v in c])


def _refuse_capture():
    import torch
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('the audio strip cannot run inside a hipGraph capture (it allocates its output and uploads host tables)')


def _on_gpu(x, what):
    import torch
    if not torch.is_tensor(x) or x.device.type != 'cuda':
        raise RuntimeError('%s must be a CUDA tensor; %s' % (what, _NO_GPU))


def _cuda(x, what, dtype, ndim):
    _on_gpu(x, what)
    if x.dtype != dtype or x.ndim != ndim or x.numel() < 1:
        raise TypeError('%s must be %d-dimensional %s and not empty, got %s %s' % (what, ndim, dtype, tuple(x.shape), x.dtype))
    return x.detach().contiguous()


def device_band(audio, mel, bounds, S, marks=None, db_range=80.0):
    """the envelope and raster launches -> {'band': (S, Nc, 3) uint8, 'env': (Nc, 2) float32, 'flags': (Nc,) int32, 'stats': (2,) int64
    (the peak's float32 bits, the number of non-finite samples)}, device tensors; nothing is read back"""
    import torch

    from . import _lib
    from .ops import _stream
    _on_gpu(audio, 'the audio')
    _refuse_capture()
    audio, mel = _cuda(audio, 'the audio', torch.float32, 1), _cuda(mel, 'the mel', torch.float32, 2)
    if mel.device != audio.device:
        raise RuntimeError('the audio and the mel are on different devices')
    lanes(S)
    b = _bounds(bounds)
    Nc, dev = b.size - 1, audio.device
    ticks = _ticks(marks)
    factors = factor_table(db_range)
    lib = _lib.load()
    with torch.cuda.device(dev):
        b_dev = torch.from_numpy(b).to(dev)
        t_dev = [torch.from_numpy(t).to(dev) for t in ticks]
        cmap, k_dev = torch.from_numpy(colormap()).to(dev), torch.from_numpy(factors).to(dev)
        env = torch.empty((Nc, 2), dtype=torch.float32, device=dev)
        flags = torch.empty(Nc, dtype=torch.int32, device=dev)
        stats = torch.empty(2, dtype=torch.int64, device=dev)
        work = torch.empty(1, dtype=torch.int64, device=dev)
        band = torch.empty((int(S), Nc, 3), dtype=torch.uint8, device=dev)
        st = _stream()
        _lib.check(lib.sdt_strip_envelope_f32(_p(audio), audio.shape[0], _p(b_dev), Nc, _p(env), _p(flags), _p(stats), st))
        _lib.check(lib.sdt_strip_raster_u8(_p(env), _p(flags), _p(stats), _p(b_dev), Nc, _p(mel), mel.shape[0], mel.shape[1], _p(cmap), _p(k_dev),
                                           _p(t_dev[0]), t_dev[0].numel(), _p(t_dev[1]), t_dev[1].numel(), _p(t_dev[2]), t_dev[2].numel(),
                                           _bytes3((BACKGROUND, WAVE, WARNING) + MARKS), int(S), _p(work), _p(band), st))
    return {'band': band, 'env': env, 'flags': flags, 'stats': stats}


def device_compose(frames, band, c0, ph):
    """the compose launch: frames (n, H, W, 3) uint8 and band (S, Nc, 3) on the GPU, host tables c0 / ph (n,) -> (n, H + S, W, 3) uint8"""
    import torch

    from . import _lib
    from .ops import _stream
    _on_gpu(frames, 'the frames')
    _refuse_capture()
    frames, band = _cuda(frames, 'the frames', torch.uint8, 4), _cuda(band, 'the band', torch.uint8, 3)
    if frames.shape[3] != 3 or band.shape[2] != 3 or band.device != frames.device:
        raise ValueError('frames must be (n, H, W, 3) and the band (S, Nc, 3) on one device, got %s and %s' % (tuple(frames.shape), tuple(band.shape)))
    n, H, W, _ = (int(v) for v in frames.shape)
    S, Nc, _ = (int(v) for v in band.shape)
    c0, ph = np.ascontiguousarray(np.asarray(c0, dtype=np.int32)), np.ascontiguousarray(np.asarray(ph, dtype=np.int32))
    if c0.shape != (n,) or ph.shape != (n,):
        raise ValueError('c0 and ph hold one entry per image (%d), got %s and %s' % (n, c0.shape, ph.shape))
    dev = frames.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        tables = torch.from_numpy(np.stack([c0, ph])).to(dev)
        out = torch.empty((n, H + S, W, 3), dtype=torch.uint8, device=dev)
        _lib.check(lib.sdt_strip_compose_u8(_p(frames), n, H, W, _p(band), S, Nc, _p(tables[0]), _p(tables[1]), _bytes3((BACKGROUND,)),
                                            _bytes3((PLAYHEAD,)), _p(out), out.numel(), _stream()))
    return out


def clip_layout(n, W, L, span_s):
    """-> (bounds, c0, ph) of an n-frame video of width W over L samples"""
    bounds, spc, Nc, scrolls = uniform_bounds(L, W, span_samples(span_s))
    c0, ph = frame_tables(n, W, spc, Nc, scrolls)
    return bounds, c0, ph


def strip_for_clip(frames, audio, mel, marks=None, height=160, span_s=4.3, db_range=80.0, details=False):
    """frames (n, H, W, 3) uint8 BGR, audio (L,) float32 and its power mel (n_mels, F) float32 on the GPU; ``marks``: None, or up to three
    lists of ticks of 1/300 s (onsets, beats of the prediction, beats of the ground truth; None = an empty lane) -> (n, H + height, W, 3)
    uint8: the frames with the band below them.  ``details``: also the device_band dict."""
    import torch
    _on_gpu(frames, 'the frames')
    _refuse_capture()  # (before any check of a shape: a capture is refused whatever the arguments)
    frames, audio = _cuda(frames, 'the frames', torch.uint8, 4), _cuda(audio, 'the audio', torch.float32, 1)
    bounds, c0, ph = clip_layout(frames.shape[0], frames.shape[2], audio.shape[0], span_s)
    d = device_band(audio, mel, bounds, height, marks, db_range)
    out = device_compose(frames, d['band'], c0, ph)
    return (out, d) if details else out


def strip_for_long_image(image, audio, mel, T, marks=None, height=160, db_range=80.0, details=False):
    """the long image (720, width, 3) uint8 BGR of T poses (render.render_long_image) -> (720 + height, width, 3): the band's columns sit
    under the poses they belong to; there is no playhead"""
    import torch
    _on_gpu(image, 'the long image')
    _refuse_capture()
    image, audio = _cuda(image, 'the long image', torch.uint8, 3), _cuda(audio, 'the audio', torch.float32, 1)
    bounds = long_image_bounds(T, audio.shape[0])
    if bounds.size - 1 != image.shape[1]:
        raise ValueError('a long image of %d poses is %d columns wide, got %d' % (T, bounds.size - 1, image.shape[1]))
    d = device_band(audio, mel, bounds, height, marks, db_range)
    out = device_compose(image[None], d['band'], [0], [-1])[0]
    return (out, d) if details else out


def nonfinite_columns(details):
    """the number of columns flagged NONFINITE (one readback)"""
    return int((details['flags'] == NONFINITE).sum().item())


def clip_marks(audio, pred, gt=None, parts=None):
    """the tick lists of one clip from sync_metrics, unchanged: audio (L,) float32, final poses (T, 2, K) float64 on the GPU -> [onsets, beats
    of part 'all' of the prediction, the same of the ground truth or None]; ``parts``: the part table of K != 121 keypoints"""
    from . import sync_metrics
    marks = [sync_metrics.onsets(audio)[0], sync_metrics.beats(pred[None].double(), parts)[0][0]]
    marks.append(None if gt is None else sync_metrics.beats(gt[None].double(), parts)[0][0])
    return marks


# ---- command line ------------------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='draw a saved clip with the band of its audio under it, on the GPU')
    ap.add_argument('results', metavar='RESULTS.npz', help='a results npz: poses_pred_batch (R, T, 2, K), and poses_gt_batch for --pair')
    ap.add_argument('audio', metavar='AUDIO.wav|.npy', help='the audio of those R clips: (R, L) or (L,) samples at 16000 Hz')
    ap.add_argument('out', metavar='OUT_PREFIX', help='OUT_PREFIX.avi and, with --long-image, OUT_PREFIX.jpg are written')
    ap.add_argument('--row', type=int, default=0, metavar='R', help='the row of the npz to draw')
    ap.add_argument('--pair', action='store_true', help='the prediction beside poses_gt_batch, and the third mark lane')
    ap.add_argument('--height', type=int, default=160, metavar='S', help='rows of the band')
    ap.add_argument('--span', type=float, default=4.3, metavar='s', help='seconds of audio in view; a longer clip scrolls')
    ap.add_argument('--no-marks', action='store_true', help='leave the mark lanes empty')
    ap.add_argument('--long-image', action='store_true', help='also write the long image with its band')
    a = ap.parse_args(argv)
    try:
        lanes(a.height)
        if not 1 <= a.span <= 60:
            raise ValueError('--span must lie in [1, 60] seconds, got %r' % (a.span,))
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None):
    a = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    from . import avi, jpeg, render
    from .mel import MelSpectrogram
    from .sync_metrics import load_audio
    with np.load(a.results) as z:
        need = ['poses_pred_batch'] + (['poses_gt_batch'] if a.pair else [])
        for k in need:
            if k not in z.files:
                raise KeyError('%s has no entry %s (it has %s)' % (a.results, k, ', '.join(z.files)))
        pred = np.asarray(z['poses_pred_batch'], dtype=np.float64)
        gt = np.asarray(z['poses_gt_batch'], dtype=np.float64) if a.pair else None
    audio = load_audio(a.audio)
    if pred.ndim != 4 or pred.shape[2] != 2 or not 0 <= a.row < pred.shape[0] or audio.shape[0] != pred.shape[0]:
        raise ValueError('poses %s must be (R, T, 2, K) with R > --row %d and the audio %s one clip per row' % (pred.shape, a.row, audio.shape))
    pred = torch.from_numpy(pred[a.row]).cuda()
    gt = None if gt is None else torch.from_numpy(gt[a.row]).cuda()
    x = torch.from_numpy(np.ascontiguousarray(audio[a.row])).cuda()
    mel = MelSpectrogram().cuda()(x[None])[0]
    marks = None if a.no_marks else clip_marks(x, pred, gt)
    frames = render.render_pose_clip(pred) if gt is None else render.render_pose_pair_clip(pred, gt)
    out, d = strip_for_clip(frames, x, mel, marks, a.height, a.span, details=True)
    H, W = int(out.shape[1]), int(out.shape[2])
    avi.write_avi(a.out + '.avi', jpeg.encode_frames(out), FPS, W, H, audio=audio[a.row], sample_rate=SAMPLE_RATE)
    print('%s.avi: %d frames of %d x %d' % (a.out, out.shape[0], W, H))
    if a.long_image:
        long_img = strip_for_long_image(render.render_long_image(pred), x, mel, pred.shape[0], marks, a.height)
        with open(a.out + '.jpg', 'wb') as f:
            f.write(jpeg.encode_frames(long_img)[0])
        print('%s.jpg: %d x %d' % (a.out, long_img.shape[1], long_img.shape[0]))
    if marks is not None:
        print('onsets: %d  beats_pred: %d  beats_gt: %s' % (len(marks[0]), len(marks[1]), 'none' if marks[2] is None else '%d' % len(marks[2])))
    print('nonfinite_samples: %d  nonfinite_columns: %d' % (int(d['stats'][1].item()), nonfinite_columns(d)))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
