"""Whole-recording demo: windowed inference, cross-fade, smoothing and a seam report (DEMO.LONG_FORM).

The generator was trained on clips of W = DATASET.NUM_FRAMES frames, so a recording of F >= W frames is generated as N overlapping windows
of W frames each and the windows' final (de-normalised, global, scaled) float64 poses are blended where they overlap:

    layout   H = W - O, N = 1 + ceil((F - W) / H), s_i = i H for i < N - 1 and s_{N-1} = F - W (the last window is moved back, not padded);
             window i reads Lw audio samples from a_i = (s_i SR) // FPS, 0.0 past the end of the recording
    blend    u_i(t) = min(t - s_i + 1, s_i + W - t), w_i(t) = min(u_i(t), max(O, 1)), out(t) = sum_i w_i x_i(t) / sum_i w_i over the covering
             windows in ascending i; a frame that one window covers is that window's value bit for bit
    smooth   y(t) = sum_{j = -m..m} c_j x(clamp(t + j, 0, F - 1)), c = ``savgol_table(m, d)``; never in place
    report   per part set all / body / face / hands: mean speed |x(t+1) - x(t)| and jerk |x(t+3) - 3 x(t+2) + 3 x(t+1) - x(t)| of the stitched
             and of the smoothed poses, and seam: the mean distance between the windows that cover a frame -- what a viewer would see as a seam

Two routes that run the same operations in the same order.  ``stitch_model`` / ``smooth_model`` / ``report_model`` are the contract in numpy;
``gather_windows`` / ``stitch`` / ``smooth`` / ``report`` run csrc/long_demo.hip on CUDA tensors.  There is no CPU fallback.  ``LongDemo`` is
what ``Voice2Pose.demo_step`` hands a long input to.

    python -m speechdrivestemplates_amd.long_demo WINDOWS.npy OUT.npz [--overlap O] [--frames F] [--smooth m d]

stitches an (N, W, 2, K) array of window poses (``poses_windows`` of a DEMO npz) on the GPU, writes ``poses_stitched``, ``poses_pred_batch``,
``window_starts`` and ``long_report`` and prints the report.
"""
import numpy as np

from ._exact_model import MAX_K, PARTS, _norm2, _ordered_sum, _part_sums, _quotient, check_parts, part_sizes

COLS = 40  # words of the report (SDT_LONG_REPORT_COLS)
GROUPS = ('speed', 'jerk', 'speed_smoothed', 'jerk_smoothed', 'seam')  # float64 words [0, 20): group g, part p at 4 g + p
N_SPEED, N_JERK, N_SEAM, NONFINITE, FRAMES, WINDOWS, SMOOTHED, PAIR_FRAMES = 20, 24, 28, 32, 33, 34, 35, 36  # int64 words
MAX_HALF, CHUNK, MAX_FRAMES = 8, 64, 1 << 24
_NO_GPU = 'the long-form demo is computed on the GPU (csrc/long_demo.hip); there is no CPU fallback (stitch_model / smooth_model / ' \
          'report_model are the numpy contract)'


# ---- layout: integers only, shared by the host module and the models ---------------------------------------------------------------------------
def check_layout(F, W, O, K=1):
    """ValueError unless K in [1, 128], W >= 2, 0 <= O <= W / 2 and F >= W (the sizes csrc/long_demo.hip takes)"""
    for name, v in (('F', F), ('W', W), ('O', O), ('K', K)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError('%s must be an integer, got %r' % (name, v))
    if not 1 <= K <= MAX_K:
        raise ValueError('K = %d keypoints outside [1, %d]' % (K, MAX_K))
    if W < 2:
        raise ValueError('a window has at least 2 frames, got W = %d' % W)
    if not 0 <= 2 * O <= W:
        raise ValueError('the overlap O = %d is outside [0, W / 2] for W = %d' % (O, W))
    if not W <= F <= MAX_FRAMES:
        raise ValueError('F = %d frames outside [W, 2^24] for W = %d: a shorter input is one window, not a long form' % (F, W))


def window_layout(F, W, O, sr=16000, fps=15):
    """-> (starts, audio offsets) of the N = 1 + ceil((F - W) / (W - O)) windows, two lists of Python ints"""
    check_layout(F, W, O)
    H = W - O
    N = 1 + -(-(F - W) // H)
    starts = [i * H for i in range(N - 1)] + [F - W]
    return starts, [(s * int(sr)) // int(fps) for s in starts]


def frames_of(N, W, O):
    """the longest recording that N windows with overlap O cover: (N - 1) (W - O) + W"""
    return (N - 1) * (W - O) + W


def covering(t, starts, W):
    """the windows that cover frame t, ascending"""
    return [i for i, s in enumerate(starts) if s <= t < s + W]


def weight(t, s, W, O):
    return min(t - s + 1, s + W - t, max(O, 1))


def savgol_table(m, d):
    """the 2 m + 1 coefficients of the Savitzky-Golay filter of half-width m and degree d: row 0 of the pseudo-inverse of the Vandermonde
    matrix on -m .. m (the value at 0 of the least-squares polynomial), float64"""
    for name, v in (('m', m), ('d', d)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError('the smoothing %s must be an integer, got %r' % (name, v))
    if not 1 <= m <= MAX_HALF:
        raise ValueError('the smoothing half-width m = %d is outside [1, %d]' % (m, MAX_HALF))
    if not 0 <= d <= 2 * m:
        raise ValueError('the smoothing degree d = %d is outside [0, 2 m] for m = %d' % (d, m))
    A = np.vander(np.arange(-m, m + 1, dtype=np.float64), int(d) + 1, increasing=True)
    return np.ascontiguousarray(np.linalg.pinv(A)[0], dtype=np.float64)


def _table(table):
    """(m, d) or the coefficients themselves -> the float64 table of 2 m + 1 entries"""
    if isinstance(table, (tuple, list)) and len(table) == 2 and all(isinstance(v, (int, np.integer)) for v in table):
        return savgol_table(*table)
    c = np.ascontiguousarray(np.asarray(table, dtype=np.float64))
    if c.ndim != 1 or c.size % 2 != 1 or not 3 <= c.size <= 2 * MAX_HALF + 1:
        raise ValueError('a smoothing table holds 2 m + 1 coefficients, m in [1, %d], got shape %s' % (MAX_HALF, c.shape))
    return c


def _windows_shape(shape, O, F):
    if len(shape) != 4 or shape[2] != 2:
        raise ValueError('window poses must be (N, W, 2, K), got %s' % (tuple(shape),))
    N, W, _, K = (int(v) for v in shape)
    F = frames_of(N, W, O) if F is None else int(F)
    check_layout(F, W, O, K)
    starts, _ = window_layout(F, W, O)
    if len(starts) != N:
        raise ValueError('%d frames with W = %d, O = %d are %d windows, got %d' % (F, W, O, len(starts), N))
    return N, W, K, F, starts


# ---- the numpy contract models ---------------------------------------------------------------------------------------------------------------
def stitch_model(windows, O, F=None):
    """(N, W, 2, K) float64 window poses -> (F, 2, K): the blend of sdt_long_stitch_f64 (F defaults to the longest recording N windows cover)"""
    windows = np.asarray(windows, dtype=np.float64)
    N, W, K, F, starts = _windows_shape(windows.shape, O, F)
    out = np.empty((F, 2, K))
    with np.errstate(all='ignore'):
        for t in range(F):
            idx = covering(t, starts, W)
            if len(idx) == 1:
                out[t] = windows[idx[0], t - starts[idx[0]]]
                continue
            num, den = None, 0
            for i in idx:
                w = weight(t, starts[i], W, O)
                p = np.float64(w) * windows[i, t - starts[i]]
                num = p if num is None else num + p
                den += w
            out[t] = num / np.float64(den)
    return out


def smooth_model(x, table):
    """(F, 2, K) -> (F, 2, K): sdt_long_smooth_f64 with ``table`` = the coefficients, or (m, d); None returns x itself"""
    x = np.asarray(x, dtype=np.float64)
    if table is None:
        return x
    c = _table(table)
    m, F = c.size // 2, x.shape[0]
    with np.errstate(all='ignore'):
        y = None
        for j in range(-m, m + 1):
            p = c[j + m] * x[np.clip(np.arange(F) + j, 0, F - 1)]
            y = p if y is None else y + p
    return y


def _motion_terms(x):
    """(F, 2, K) -> (F, K) speed terms and (F, K) jerk terms, +0.0 where the later frames do not exist"""
    F, _, K = x.shape
    speed, jerk = np.zeros((F, K)), np.zeros((F, K))
    if F > 1:
        speed[:F - 1] = np.sqrt(_norm2(x[1:, 0] - x[:-1, 0], x[1:, 1] - x[:-1, 1]))
    if F > 3:
        d = ((x[3:] - 3.0 * x[2:-1]) + 3.0 * x[1:-2]) - x[:-3]
        jerk[:F - 3] = np.sqrt(_norm2(d[:, 0], d[:, 1]))
    return speed, jerk


def report_model(windows, stitched, smoothed, O, parts=None, return_sums=False):
    """the 40 int64 words of sdt_long_report_f64 (float64 words viewed as int64); ``smoothed`` may be None.  ``return_sums``: also the 20
    float64 sums before the divisions"""
    windows, stitched = np.asarray(windows, dtype=np.float64), np.asarray(stitched, dtype=np.float64)
    N, W, K, F, starts = _windows_shape(windows.shape, O, stitched.shape[0])
    parts = check_parts(parts, K)
    sizes = part_sizes(parts)
    with np.errstate(all='ignore'):
        terms = np.zeros((F, 5, K))
        terms[:, 0], terms[:, 1] = _motion_terms(stitched)
        if smoothed is not None:
            terms[:, 2], terms[:, 3] = _motion_terms(np.asarray(smoothed, dtype=np.float64))
        pairs = np.zeros(F, dtype=np.int64)
        for t in range(F):
            idx = covering(t, starts, W)
            if len(idx) < 2:
                continue
            x = [windows[i, t - starts[i]] for i in idx]
            acc = np.zeros(K)
            for a in range(len(idx)):
                for b in range(a + 1, len(idx)):
                    acc = acc + np.sqrt(_norm2(x[a][0] - x[b][0], x[a][1] - x[b][1]))
            terms[t, 4] = acc
            pairs[t] = len(idx) * (len(idx) - 1) // 2
        frame_sums = _part_sums(terms, parts).reshape(F, 20)  # one partial per frame
        chunk_sums = np.stack([_ordered_sum(frame_sums[t0:t0 + CHUNK], 0) for t0 in range(0, F, CHUNK)])
        tot = _ordered_sum(chunk_sums, 0)
        n_pairs = int(pairs.sum())
        out = np.zeros(COLS)
        words = np.zeros(COLS, dtype=np.int64)
        for p in range(4):
            n_speed, n_jerk, n_seam = (F - 1) * sizes[p], max(F - 3, 0) * sizes[p], n_pairs * sizes[p]
            for g in range(5):
                out[4 * g + p] = _quotient(tot[4 * g + p], n_seam if g == 4 else (n_jerk if g & 1 else n_speed))
            words[N_SPEED + p], words[N_JERK + p], words[N_SEAM + p] = n_speed, n_jerk, n_seam
    words[:20] = out[:20].view(np.int64)
    words[NONFINITE] = int(not np.isfinite(tot).all())
    words[FRAMES], words[WINDOWS], words[SMOOTHED], words[PAIR_FRAMES] = F, N, int(smoothed is not None), n_pairs
    return (words, tot) if return_sums else words


def report_values(words):
    """the 40 words -> {'speed': {'all': ..}, 'jerk': .., 'speed_smoothed': .., 'jerk_smoothed': .., 'seam': .., counts and flags}; the
    smoothed groups only when smoothed poses were given"""
    words = np.ascontiguousarray(np.asarray(words, dtype=np.int64))
    f = words.view(np.float64)
    has = bool(words[SMOOTHED])
    out = {g: {p: float(f[4 * i + j]) for j, p in enumerate(PARTS)} for i, g in enumerate(GROUPS) if has or 'smoothed' not in g}
    out.update(frames=int(words[FRAMES]), windows=int(words[WINDOWS]), pair_frames=int(words[PAIR_FRAMES]), nonfinite=int(words[NONFINITE]),
               smoothed=has)
    return out


def describe(words):
    """one line for the log"""
    v = report_values(words)
    msg = '%d frames from %d windows, %d overlapping (frame, pair) terms' % (v['frames'], v['windows'], v['pair_frames'])
    for g in GROUPS:
        if g in v:
            msg += '  %s: ' % g + ' '.join('%s %.4f' % (p, v[g][p]) for p in PARTS)
    return msg + ('  NONFINITE' if v['nonfinite'] else '')


# ---- the device route (csrc/long_demo.hip) ---------------------------------------------------------------------------------------------------
def _refuse_capture():
    import torch
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('the long-form demo cannot run inside a hipGraph capture (it allocates its outputs)')


def _dev_tensor(x, dtype, what):
    import torch
    if not torch.is_tensor(x) or x.device.type != 'cuda':
        raise RuntimeError('%s must be a CUDA tensor; %s' % (what, _NO_GPU))
    if x.dtype != dtype:
        raise TypeError('%s must be %s, got %s' % (what, dtype, x.dtype))
    return x.detach().contiguous()


def _call(fn, device, *args):
    import torch
    from . import _lib
    with torch.cuda.device(device):
        _lib.check(fn(*args, torch.cuda.current_stream(device).cuda_stream))


def _ptr(t):
    import ctypes as C
    return None if t is None else C.c_void_p(t.data_ptr())


def gather_windows(audio, offsets, Lw):
    """audio (L,) float32 on the GPU, ``offsets``: n sample offsets (a list, or an int64 tensor on the same device) -> (n, Lw) float32, zero past
    the end of the recording"""
    import torch
    from . import _lib
    audio = _dev_tensor(audio, torch.float32, 'the audio')
    _refuse_capture()
    if audio.ndim != 1 or audio.numel() < 1:
        raise ValueError('the audio must be one recording of shape (L,), got %s' % (tuple(audio.shape),))
    if not torch.is_tensor(offsets):
        offsets = torch.tensor([int(o) for o in offsets], dtype=torch.int64, device=audio.device)
    offsets = _dev_tensor(offsets, torch.int64, 'the offsets')
    n, Lw = int(offsets.numel()), int(Lw)
    if offsets.ndim != 1 or offsets.device != audio.device or not 1 <= n <= 65535:
        raise ValueError('the offsets must be 1 to 65535 int64 entries on %s' % (audio.device,))
    if not 1 <= Lw <= MAX_FRAMES:
        raise ValueError('window length %d outside [1, 2^24]' % Lw)
    out = torch.empty((n, Lw), dtype=torch.float32, device=audio.device)
    _call(_lib.load().sdt_long_windows_gather_f32, audio.device, _ptr(audio), audio.numel(), _ptr(offsets), n, Lw, _ptr(out))
    return out


def stitch(windows, O, F=None):
    """(N, W, 2, K) float64 window poses on the GPU -> (F, 2, K)"""
    import torch
    from . import _lib
    windows = _dev_tensor(windows, torch.float64, 'the window poses')
    _refuse_capture()
    N, W, K, F, _ = _windows_shape(windows.shape, O, F)
    out = torch.empty((F, 2, K), dtype=torch.float64, device=windows.device)
    _call(_lib.load().sdt_long_stitch_f64, windows.device, _ptr(windows), N, W, int(O), F, K, _ptr(out))
    return out


def smooth(x, table):
    """(F, 2, K) float64 on the GPU -> a new (F, 2, K) tensor; ``table``: the coefficients, or (m, d)"""
    import ctypes as C
    import torch
    from . import _lib
    x = _dev_tensor(x, torch.float64, 'the poses')
    _refuse_capture()
    if x.ndim != 3 or x.shape[1] != 2 or not 1 <= x.shape[2] <= MAX_K or not 1 <= x.shape[0] <= MAX_FRAMES:
        raise ValueError('poses must be (F, 2, K) with K in [1, %d], got %s' % (MAX_K, tuple(x.shape)))
    c = _table(table)
    y = torch.empty_like(x)
    _call(_lib.load().sdt_long_smooth_f64, x.device, _ptr(x), int(x.shape[0]), int(x.shape[2]), (C.c_double * c.size)(*c.tolist()), c.size // 2,
          _ptr(y))
    return y


def report(windows, stitched, smoothed, O, parts=None):
    """-> the 40 int64 words on the GPU (``report_values`` names them); ``smoothed`` may be None"""
    import ctypes as C
    import torch
    from . import _lib
    windows = _dev_tensor(windows, torch.float64, 'the window poses')
    stitched = _dev_tensor(stitched, torch.float64, 'the stitched poses')
    smoothed = None if smoothed is None else _dev_tensor(smoothed, torch.float64, 'the smoothed poses')
    _refuse_capture()
    if stitched.ndim != 3:
        raise ValueError('stitched poses must be (F, 2, K), got %s' % (tuple(stitched.shape),))
    N, W, K, F, _ = _windows_shape(windows.shape, O, stitched.shape[0])
    for name, x in (('stitched', stitched), ('smoothed', smoothed)):
        if x is not None and (tuple(x.shape) != (F, 2, K) or x.device != windows.device):
            raise ValueError('the %s poses must be (%d, 2, %d) on %s, got %s' % (name, F, K, windows.device, tuple(x.shape)))
    parts = check_parts(parts, K)
    lib = _lib.load()
    parts_dev = torch.from_numpy(parts).to(windows.device)
    work = torch.empty(int(lib.sdt_long_report_workspace_bytes(F)) // 8, dtype=torch.int64, device=windows.device)
    out = torch.empty(COLS, dtype=torch.int64, device=windows.device)
    _call(lib.sdt_long_report_f64, windows.device, _ptr(windows), _ptr(stitched), _ptr(smoothed), _ptr(parts_dev),
          (C.c_int64 * 4)(*part_sizes(parts)), N, W, int(O), F, K, _ptr(work), _ptr(out))
    return out


# ---- the pipeline's long path ----------------------------------------------------------------------------------------------------------------
class LongDemo:
    """``run(batch)`` of one recording for a Voice2Pose pipeline with DEMO.LONG_FORM: the windows' audio gathered on the device, forwarded in
    groups of DEMO.LONG_BATCH with one template code for the whole recording, final poses per group, then stitch, smooth and report."""

    def __init__(self, pipeline):
        from .config import check_long_demo
        from .core.datasets.gesture_dataset import PoseTransforms, parse_audio_length
        self.pipeline, cfg = pipeline, pipeline.cfg
        self.opts = check_long_demo(cfg)
        self.W, self.sr, self.fps = int(cfg.DATASET.NUM_FRAMES), int(cfg.DATASET.AUDIO_SR), int(cfg.DATASET.FPS)
        self.Lw = parse_audio_length(cfg.DATASET.AUDIO_LENGTH, self.sr, self.fps)[0]
        self.parts = PoseTransforms.part_table()
        self.table = None if self.opts['smooth'] is None else savgol_table(*self.opts['smooth'])
        from .config import check_sync_metrics
        self.sync = check_sync_metrics(cfg)  # TEST.SYNC_METRICS: None, or the tolerance in ticks and sigma

    def _code(self, dev, interpolation_coeff):
        """one template code (1, D) for the whole recording: DEMO.CODE_PATH's vector, or DEMO.CODE_INDEX (interpolated towards CODE_INDEX_B by the step's coefficient), or
        one normal draw, or one random row of the table -- drawn once, not per window"""
        import torch
        model, cfg = self.pipeline.model, self.pipeline.cfg
        code = cfg.VOICE2POSE.GENERATOR.CLIP_CODE
        if code.DIMENSION is None:
            return None
        given = self.pipeline.demo_condition_code(1)  # DEMO.CODE_PATH: a code vector from a file (an error together with DEMO.CODE_INDEX)
        if given is not None:
            return given
        if code.SAMPLE_FROM_NORMAL:
            return torch.randn([1, code.DIMENSION], device=dev)
        table = model._code_table(dev)
        if cfg.DEMO.CODE_INDEX is not None:
            assert 0 <= cfg.DEMO.CODE_INDEX < table.size(0)
            c = table[cfg.DEMO.CODE_INDEX:cfg.DEMO.CODE_INDEX + 1]
            if interpolation_coeff is not None:
                assert cfg.DEMO.CODE_INDEX_B < table.size(0)
                c = c * (1 - interpolation_coeff) + table[cfg.DEMO.CODE_INDEX_B:cfg.DEMO.CODE_INDEX_B + 1] * interpolation_coeff
            return c.detach()
        row = int(torch.randint(table.size(0), (1,)))
        return table[row:row + 1].detach()

    @staticmethod
    def _group_stat(stat, n):
        """the recording's speaker statistics for a group of n windows (tensors of one row are repeated, arrays broadcast by themselves)"""
        import torch
        out = {}
        for k, v in stat.items():
            if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == 1:
                v = v.expand(n, *v.shape[1:])
            out[k] = v
        return out

    def generate(self, batch, interpolation_coeff=None):
        """the forward passes: -> (window poses (N, W, 2, K) float64 final, starts, the code (1, D) or None)"""
        import torch
        pipe = self.pipeline
        model, ds = pipe.model, pipe.test_dataset
        dev = model._device()
        F, W, O = int(batch['num_frames'][0]), self.W, self.opts['overlap']
        audio = batch['audio'].to(dev, non_blocking=True)
        if audio.ndim != 2 or audio.shape[0] != 1:
            raise ValueError('the long-form demo takes one recording per step, audio (1, L), got %s' % (tuple(audio.shape),))
        starts, offsets = window_layout(F, W, O, self.sr, self.fps)
        N, K = len(starts), int(pipe.cfg.DATASET.NUM_LANDMARKS)
        offs = torch.tensor(offsets, dtype=torch.int64, device=dev)
        code = self._code(dev, interpolation_coeff)
        windows = torch.empty((N, W, 2, K), dtype=torch.float64, device=dev)
        speaker = list(batch['speaker'])
        for g0 in range(0, N, self.opts['batch']):
            n = min(self.opts['batch'], N - g0)
            group = {'audio': gather_windows(audio[0].float(), offs[g0:g0 + n], self.Lw), 'speaker': speaker * n if len(speaker) == 1 else speaker,
                     'clip_index': batch['clip_index'].reshape(-1)[:1].expand(n), 'num_frames': torch.full((n,), W, dtype=torch.int64)}
            res = model(group, ds, return_loss=False, condition_code=None if code is None else code.expand(n, -1).contiguous())
            windows[g0:g0 + n] = ds.get_final_results(res['poses_pred_batch'].detach(), self._group_stat(batch['speaker_stat'], n))
        return windows, starts, code

    def run(self, batch, interpolation_coeff=None):
        import logging
        import torch
        windows, starts, code = self.generate(batch, interpolation_coeff)
        F, O = int(batch['num_frames'][0]), self.opts['overlap']
        stitched = stitch(windows, O, F)
        final = stitched if self.table is None else smooth(stitched, self.table)
        words = report(windows, stitched, None if self.table is None else final, O, self.parts).cpu()
        logging.info('[DEMO] long form: ' + describe(words.numpy()))
        out = {'poses_pred_batch': final.unsqueeze(0), 'condition_code': code, 'poses_windows': windows,
               'window_starts': torch.tensor(starts, dtype=torch.int64), 'poses_stitched': stitched.unsqueeze(0), 'long_report': words}
        if self.sync is not None:  # audio onsets against the beats of the whole recording: one row, T = F, no ground truth
            from . import sync_metrics as sm
            audio = batch['audio'].to(final.device, non_blocking=True)[0].float()
            which = [('final', final)] + ([] if self.table is None else [('stitched', stitched)])
            out['sync_report'] = torch.stack([sm.recording_report(x, audio, self.sync['tol_ticks'], self.sync['sigma'], self.parts)
                                              for _, x in which]).cpu()
            for (name, _), rec in zip(which, out['sync_report'].numpy()):
                logging.info('[DEMO] sync: %s poses: ' % name + sm.describe_row(rec, audio.numel() // sm.HOP))
        return out


OUT_KEYS = ('poses_stitched', 'poses_pred_batch', 'window_starts', 'long_report')  # entries of the command line's OUT.npz


def segments(F, limit):
    """[(first, end)) frame ranges of at most ``limit`` frames that cover F frames, as even as integers allow"""
    n = -(-F // limit)
    return [(j * F // n, (j + 1) * F // n) for j in range(n)]


# ---- command line ------------------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='stitch saved window poses into one sequence on the GPU and report speed, jerk and seams')
    ap.add_argument('windows', metavar='WINDOWS.npy', help='an (N, W, 2, K) array of final window poses (poses_windows of a DEMO npz)')
    ap.add_argument('out', metavar='OUT.npz', help='poses_stitched, poses_pred_batch, window_starts, long_report')
    ap.add_argument('--overlap', type=int, default=16, metavar='O', help='frames two neighbouring windows share, 0 <= O <= W / 2')
    ap.add_argument('--frames', type=int, default=None, metavar='F', help='frames of the recording (default: the most the windows cover)')
    ap.add_argument('--smooth', type=int, nargs=2, default=None, metavar=('m', 'd'), help='Savitzky-Golay half-width and degree')
    a = ap.parse_args(argv)
    if a.overlap < 0:
        ap.error('--overlap must be >= 0')
    if a.smooth is not None:
        try:
            savgol_table(*a.smooth)
        except ValueError as e:
            ap.error(str(e))
    return a


def main(argv=None):
    a = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    windows = np.asarray(np.load(a.windows), dtype=np.float64)
    N, W, K, F, starts = _windows_shape(windows.shape, a.overlap, a.frames)
    win = torch.from_numpy(np.ascontiguousarray(windows)).cuda()
    stitched = stitch(win, a.overlap, F)
    final = stitched if a.smooth is None else smooth(stitched, tuple(a.smooth))
    words = report(win, stitched, None if a.smooth is None else final, a.overlap).cpu().numpy()
    print(describe(words))
    np.savez(a.out, poses_stitched=stitched.cpu().numpy()[None], poses_pred_batch=final.cpu().numpy()[None],
             window_starts=np.asarray(starts, dtype=np.int64), long_report=words)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
