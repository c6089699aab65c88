"""Speech-gesture synchrony: do the hands move when the voice does?  (TEST.SYNC_METRICS)

Audio onsets of a clip, motion beats of its final float64 poses per part (all, body, face, hands) and how they line up.  The time base needs
16000 samples/s and 15 frames/s; every time is an integer in ticks of 1/300 s (an audio hop of 160 samples is 3 ticks, a pose frame 20).

    onsets   Nf = L // 160 frames, frame n covers samples [160 n, 160 n + 320) (0.0 at or past L); e[n] = sqrt(sum x^2) in float64;
             o[0] = 0, o[n] = e[n] - e[n-1] where that is > 0, else 0.  Frame 1 <= n <= Nf - 2 is a candidate if o[n] > o[n-1], o[n] >= o[n+1],
             o[n] > DELTA * mean(o[n-15 .. n+15], clipped to the clip) and o[n] > FLOOR * max e.  Candidates are accepted left to right; one
             fewer than GAP = 8 frames after the last accepted one is dropped.  An accepted frame n has tick 3 n + 3.
    beats    s_p[t] = sum over k in part p of |x(t+1) - x(t)|, t < T - 1.  t in [1, T - 3] is a beat if s[t] > s[t-1], s[t] >= s[t+1] and
             s[t] > GAMMA * mean(s).  A beat t has tick 20 t + 10.
    match    per beat d = min(distance to the nearest onset, 150) (150 without onsets): hits += d <= tol, dsum += d, align += G[d] with
             G[d] = exp(-(d / 300)^2 / (2 sigma^2)) from a host table; per onset: covered += some beat lies within tol.

DELTA, FLOOR, GAP and GAMMA are untuned.  Two routes run the same operations in the same order: ``onsets_model`` / ``beats_model`` /
``match_model`` / ``sync_model`` / ``epoch_model`` are the contract in numpy; ``SyncAccumulator``, ``onsets`` and ``beats`` run
csrc/sync_metrics.hip on CUDA tensors.  There is no CPU fallback.

    python -m speechdrivestemplates_amd.sync_metrics POSES.npz AUDIO.wav|.npy [--tolerance s] [--sigma s] [--out table.npz]

reads ``poses_pred_batch`` (and ``poses_gt_batch`` if present) of a results npz, (R, T, 2, K), and the audio of those R clips ((R, L) or (L,)
float samples at 16000 Hz; a wav file is one clip), runs the device route and prints the epoch values.
"""
from functools import partial

import numpy as np

from . import _record_table
from ._exact_model import MAX_TABLES  # noqa: F401  (public names of this module)
from ._exact_model import MAX_COPIES, PARTS, _butterfly_wave, _norm2, _ordered_sum, _part_sums, _quotient, check_parts
from ._record_table import CHUNK  # noqa: F401
from ._record_table import RecordTable, check_keypoints, check_num_clips, check_poses, chunked_records, cuda_device, ptr, stream

SAMPLE_RATE, FPS, TICKS = 16000, 15, 300
HOP, FRAME, HOP_TICKS, FRAME_TICKS = 160, 320, 3, 20
HALF, GAP, DMAX = 15, 8, 150
DELTA, FLOOR, GAMMA = 1.5, 2.0 ** -6, 1.0  # untuned detector constants (handed to the launches by value)
ROW_COLS, COLS, OUT_COLS = 24, 48, 24  # SDT_SYNC_ROW_COLS, SDT_SYNC_COLS, SDT_SYNC_OUT_COLS
INT_GROUPS = ('beats', 'hits', 'dsum', 'covered')
ROW_ONSETS, ROW_NONFINITE, ROW_FRAMES = 20, 21, 22  # a row record: float64 [0,4) align[p]; int64 [4,20) group g, part p at 4 + 4 g + p
ALIGN_PRED, ALIGN_GT, INT_PRED, INT_GT = 0, 4, 8, 24  # a clip record: float64 [0,8); int64 group g, part p at 8 (or 24) + 4 g + p
ONSETS, SEEN, COPIES, NONFINITE, FRAMES, HOPS = 40, 41, 42, 43, 44, 45
COLUMN_NAMES = tuple('align_%s_%s' % (w, p) for w in ('pred', 'gt') for p in PARTS) + tuple(
    '%s_%s_%s' % (g, w, p) for w in ('pred', 'gt') for g in INT_GROUPS for p in PARTS) + (
    'onsets', 'seen', 'copies', 'nonfinite', 'frames', 'hops', 'zero_46', 'zero_47')
# the epoch vector: float64 pairs {all, hands}, then one value, then int64 words
VALUE_PAIRS = ('sync_precision', 'sync_precision_gt', 'sync_recall', 'sync_recall_gt', 'sync_offset_ms', 'beat_align', 'beat_align_gt',
               'beats_per_s', 'beats_per_s_gt')
OUT_ONSETS_PER_S, OUT_SEEN, OUT_NONFINITE, OUT_INDEX_ERRORS = 18, 20, 21, 22
BOOKKEEPING = ('sync_clips_seen', 'sync_index_errors')  # entries of result() that are not metrics
MAX_HOPS, MAX_FRAMES = 1 << 28, 1 << 24
_NOUN = 'the synchrony metrics'
_NO_GPU = 'the synchrony metrics are computed on the GPU (csrc/sync_metrics.hip); there is no CPU fallback (sync_model is the numpy contract)'
assert len(COLUMN_NAMES) == COLS


def tolerance_ticks(seconds):
    """TEST.SYNC_TOLERANCE in seconds -> ticks: floor(300 tol + 0.5), ValueError outside [1, 150]"""
    if isinstance(seconds, bool) or not isinstance(seconds, (int, float)) or not (seconds == seconds and abs(seconds) != float('inf')):
        raise ValueError('the tolerance must be a finite number of seconds, got %r' % (seconds,))
    ticks = int(np.floor(TICKS * float(seconds) + 0.5))
    if not 1 <= ticks <= DMAX:
        raise ValueError('a tolerance of %r s is %d ticks of 1/300 s, outside [1, %d]' % (seconds, ticks, DMAX))
    return ticks


def check_tol(tol):
    if isinstance(tol, bool) or not isinstance(tol, (int, np.integer)) or not 1 <= tol <= DMAX:
        raise ValueError('the tolerance must be an integer in [1, %d] ticks, got %r' % (DMAX, tol))
    return int(tol)


def gauss_table(sigma):
    """G[d] = exp(-(d / 300)^2 / (2 sigma^2)) for d = 0 .. 150, float64, computed on the host (the exponential is not part of the contract)"""
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not (0 < sigma < float('inf')):
        raise ValueError('sigma must be a finite number of seconds > 0, got %r' % (sigma,))
    d = np.arange(DMAX + 1, dtype=np.float64) / TICKS
    return np.ascontiguousarray(np.exp(-(d * d) / (2.0 * float(sigma) * float(sigma))))


def _table(table):
    """sigma, or the 151 entries themselves -> the float64 table"""
    if isinstance(table, (int, float)) and not isinstance(table, bool):
        return gauss_table(table)
    g = np.ascontiguousarray(np.asarray(table, dtype=np.float64))
    if g.shape != (DMAX + 1,) or not (g >= 0).all():
        raise ValueError('a Gaussian table holds %d entries >= 0, got shape %s' % (DMAX + 1, g.shape))
    return g


# ---- the numpy contract models ---------------------------------------------------------------------------------------------------------------
def envelope_model(audio, return_energy=False):
    """(L,) float32 -> e (Nf,) float64; ``return_energy``: (e, the sums of squares under the roots)"""
    x = np.asarray(audio)
    if x.ndim != 1:
        raise ValueError('one clip of audio is (L,), got %s' % (x.shape,))
    L = x.shape[0]
    Nf = L // HOP
    pad = np.zeros(Nf * HOP + FRAME)
    pad[:L] = x.astype(np.float32).astype(np.float64)
    with np.errstate(all='ignore'):
        idx = np.arange(Nf)[:, None] * HOP + np.arange(64)[None, :]
        acc = None
        for j in range(5):  # lane l: samples l, l + 64, .., l + 256; the first product starts the sum
            v = pad[idx + 64 * j]
            acc = v * v if acc is None else acc + v * v
        energy = _butterfly_wave(acc)
        return (np.sqrt(energy), energy) if return_energy else np.sqrt(energy)


def onsets_model(audio, delta=DELTA, floor=FLOOR):
    """one clip (L,) float32 -> {'env', 'strength': (Nf,) float64, 'energy': the sums under the roots of env, 'candidates': frames before the
    refractory pass, 'frames': accepted frames, 'ticks': 3 n + 3 of those (int64), 'nonfinite': an e[n] is not finite}"""
    e, energy = envelope_model(audio, True)
    Nf = e.size
    delta, floor = np.float64(delta), np.float64(floor)
    with np.errstate(all='ignore'):
        o = np.zeros(Nf)
        if Nf > 1:
            d = e[1:] - e[:-1]
            o[1:] = np.where(d > 0, d, 0.0)
        emax = np.fmax.reduce(e, initial=0.0) if Nf else np.float64(0.0)
        # the ordered sum over [n - 15, n + 15] from +0.0: o >= +0.0, so the zeros that stand in for frames outside the clip change no bit
        pad = np.concatenate([np.zeros(HALF), o, np.zeros(HALF)])
        s = np.zeros(Nf)
        for j in range(2 * HALF + 1):
            s = s + pad[j:j + Nf]
        n = np.arange(Nf)
        count = np.minimum(n + HALF, Nf - 1) - np.maximum(n - HALF, 0) + 1
        mean = s / count.astype(np.float64) if Nf else s
        cand = np.zeros(Nf, dtype=bool)
        if Nf > 2:
            i = slice(1, Nf - 1)
            cand[i] = (o[i] > o[:-2]) & (o[i] >= o[2:]) & (o[i] > delta * mean[i]) & (o[i] > floor * emax)
    frames, last = [], -GAP
    for c in np.flatnonzero(cand):
        if c - last >= GAP:
            frames.append(int(c))
            last = int(c)
    frames = np.asarray(frames, dtype=np.int64)
    return {'env': e, 'strength': o, 'energy': energy, 'candidates': np.flatnonzero(cand), 'frames': frames, 'ticks': HOP_TICKS * frames + HOP_TICKS,
            'nonfinite': bool(not np.isfinite(e).all())}


def speeds_model(poses, parts):
    """(R, T, 2, K) float64 -> (R, T - 1, 4): per part the summed keypoint speeds, as clip_metrics forms speed_pred"""
    x = np.asarray(poses, dtype=np.float64)
    if x.ndim != 4 or x.shape[2] != 2:
        raise ValueError('poses must be (rows, frames, 2, K), got %s' % (x.shape,))
    parts = check_parts(parts, x.shape[3])
    if x.shape[1] < 2:
        return np.zeros((x.shape[0], 0, 4))
    with np.errstate(all='ignore'):
        return _part_sums(np.sqrt(_norm2(x[:, 1:, 0] - x[:, :-1, 0], x[:, 1:, 1] - x[:, :-1, 1])), parts)


def beats_model(poses, parts=None, gamma=GAMMA):
    """(R, T, 2, K) float64 -> {'speed': (R, T - 1, 4), 'flags': (R, 4, T) bool, 'nonfinite': (R,) bool}; ``beat_ticks`` lists the ticks"""
    s = speeds_model(poses, parts)
    R, Tm1, _ = s.shape
    T = np.asarray(poses).shape[1]
    flags = np.zeros((R, 4, T), dtype=bool)
    with np.errstate(all='ignore'):
        total = _ordered_sum(s, 1)  # (R, 4)
        if T >= 4:
            thr = np.float64(gamma) * (total / np.float64(Tm1))
            mid = s[:, 1:Tm1 - 1]
            ok = (mid > s[:, :Tm1 - 2]) & (mid >= s[:, 2:]) & (mid > thr[:, None, :])
            flags[:, :, 1:T - 2] = np.moveaxis(ok, 1, 2)
    return {'speed': s, 'flags': flags, 'nonfinite': ~np.isfinite(total).all(axis=1)}


def beat_ticks(flags):
    """(T,) bool -> the beats' ticks 20 t + 10 (int64)"""
    return FRAME_TICKS * np.flatnonzero(flags).astype(np.int64) + FRAME_TICKS // 2


def match_model(beats, onsets, tol, table):
    """ascending beat ticks against ascending onset ticks -> (beats, hits, dsum, covered, align); ``table``: sigma or the 151 entries"""
    beats, onsets = np.asarray(beats, dtype=np.int64), np.asarray(onsets, dtype=np.int64)
    tol, G = check_tol(tol), _table(table)
    d = np.full(beats.shape, DMAX, dtype=np.int64)
    if onsets.size and beats.size:
        i = np.searchsorted(onsets, beats)  # the first onset at or after the beat
        right = np.where(i < onsets.size, onsets[np.minimum(i, onsets.size - 1)] - beats, DMAX)
        left = np.where(i > 0, beats - onsets[np.maximum(i - 1, 0)], DMAX)
        d = np.minimum(np.minimum(left, right), DMAX)
    align = np.float64(0.0)
    for v in G[d]:
        align = align + v
    covered = 0
    if beats.size and onsets.size:
        j = np.searchsorted(beats, onsets)
        near = np.minimum(np.where(j < beats.size, beats[np.minimum(j, beats.size - 1)] - onsets, DMAX + 1),
                          np.where(j > 0, onsets - beats[np.maximum(j - 1, 0)], DMAX + 1))
        covered = int((near <= tol).sum())
    return int(beats.size), int((d <= tol).sum()), int(d.sum()), covered, align


def row_records_model(poses, onset_models, parts, tol, table, gamma=GAMMA):
    """the (R, 24) int64 records of sdt_sync_rows_f64; ``onset_models``: the B clips' onsets_model results, row r belongs to clip r % B"""
    poses = np.asarray(poses, dtype=np.float64)
    bm = beats_model(poses, parts, gamma)
    R, B = bm['flags'].shape[0], len(onset_models)
    rec = np.zeros((R, ROW_COLS), dtype=np.int64)
    G = _table(table)
    for r in range(R):
        om = onset_models[r % B]
        for p in range(4):
            n, hits, dsum, covered, align = match_model(beat_ticks(bm['flags'][r, p]), om['ticks'], tol, G)
            rec[r, p] = np.float64(align).view(np.int64)
            rec[r, 4 + p], rec[r, 8 + p], rec[r, 12 + p], rec[r, 16 + p] = n, hits, dsum, covered
        rec[r, ROW_ONSETS], rec[r, ROW_NONFINITE], rec[r, ROW_FRAMES] = om['ticks'].size, bool(bm['nonfinite'][r]) or om['nonfinite'], poses.shape[1]
    return rec


def sync_model(pred, gt, audio, parts, tol, table, multiple=1, delta=DELTA, floor=FLOOR, gamma=GAMMA):
    """the (B, 48) int64 clip records the device route commits: pred / gt (multiple * B, T, 2, K) float64 (gt may be None), audio (B, L)"""
    pred = np.asarray(pred, dtype=np.float64)
    audio = np.asarray(audio)
    m, R, T = int(multiple), pred.shape[0], pred.shape[1]
    if not 1 <= m <= MAX_COPIES or R % m or audio.ndim != 2 or audio.shape[0] != R // m:
        raise ValueError('%d rows and audio %s are not %d copies of a batch (copies in [1, %d])' % (R, audio.shape, m, MAX_COPIES))
    B = R // m
    oms = [onsets_model(a, delta, floor) for a in audio]
    rows = [row_records_model(pred, oms, parts, tol, table, gamma),
            np.zeros((R, ROW_COLS), dtype=np.int64) if gt is None else row_records_model(np.asarray(gt, dtype=np.float64), oms, parts, tol, table,
                                                                                         gamma)]
    rec = np.zeros((B, COLS), dtype=np.int64)
    for w, (a0, i0) in enumerate(((ALIGN_PRED, INT_PRED), (ALIGN_GT, INT_GT))):
        copies = rows[w].reshape(m, B, ROW_COLS)
        rec[:, a0:a0 + 4] = _ordered_sum(copies[:, :, :4].copy().view(np.float64), 0).view(np.int64)
        rec[:, i0:i0 + 16] = copies[:, :, 4:20].sum(axis=0)
        rec[:, NONFINITE] += copies[:, :, ROW_NONFINITE].sum(axis=0)
    rec[:, ONSETS] = rows[0].reshape(m, B, ROW_COLS)[:, :, ROW_ONSETS].sum(axis=0)
    rec[:, NONFINITE] = (rec[:, NONFINITE] != 0) | ~np.isfinite(rec[:, :8].copy().view(np.float64)).all(axis=1)
    rec[:, SEEN], rec[:, COPIES], rec[:, FRAMES], rec[:, HOPS] = 1, m, T, audio.shape[1] // HOP
    return rec


def epoch_model(tables, index_errors=0):
    """the 24 words of sdt_sync_epoch over ``tables``, a list of (N, 48) int64 record arrays, one per rank"""
    tot_f, tot_i = np.zeros(8), np.zeros(COLS, dtype=np.int64)
    with np.errstate(all='ignore'):
        for chunk in chunked_records(tables, SEEN):
            f, h = np.zeros(8), np.zeros(COLS, dtype=np.int64)
            for rec in chunk:
                h[SEEN] += 1
                if rec[NONFINITE] != 0:
                    h[NONFINITE] += 1
                    continue
                f = f + rec[:8].view(np.float64)
                h[8:ONSETS + 1] += rec[8:ONSETS + 1]
                h[COPIES] += rec[COPIES] * rec[FRAMES]
                h[HOPS] += rec[COPIES] * rec[HOPS]
            tot_f, tot_i = tot_f + f, tot_i + h
        out = np.zeros(OUT_COLS)
        for h, p in enumerate((0, 3)):
            bp, bg = int(tot_i[INT_PRED + p]), int(tot_i[INT_GT + p])
            out[0 + h] = _quotient(float(tot_i[INT_PRED + 4 + p]), bp)
            out[2 + h] = _quotient(float(tot_i[INT_GT + 4 + p]), bg)
            out[4 + h] = _quotient(float(tot_i[INT_PRED + 12 + p]), int(tot_i[ONSETS]))
            out[6 + h] = _quotient(float(tot_i[INT_GT + 12 + p]), int(tot_i[ONSETS]))
            out[8 + h] = _quotient(np.float64(tot_i[INT_PRED + 8 + p]) * np.float64(1000.0 / 300.0), bp)
            out[10 + h] = _quotient(tot_f[ALIGN_PRED + p], bp)
            out[12 + h] = _quotient(tot_f[ALIGN_GT + p], bg)
            out[14 + h] = _quotient(np.float64(bp) * np.float64(15.0), int(tot_i[COPIES]))
            out[16 + h] = _quotient(np.float64(bg) * np.float64(15.0), int(tot_i[COPIES]))
        out[OUT_ONSETS_PER_S] = _quotient(np.float64(tot_i[ONSETS]) * np.float64(100.0), int(tot_i[HOPS]))
    words = out.view(np.int64).copy()
    words[OUT_SEEN], words[OUT_NONFINITE], words[OUT_INDEX_ERRORS], words[23] = tot_i[SEEN], tot_i[NONFINITE], index_errors, 0
    return words


def epoch_values(words):
    """the 24 words of the epoch vector -> the named values; the hands values carry the suffix _hands"""
    words = np.ascontiguousarray(np.asarray(words, dtype=np.int64))
    f = words.view(np.float64)
    out = {}
    for q, name in enumerate(VALUE_PAIRS):
        out[name] = float(f[2 * q])
        out[name + '_hands'] = float(f[2 * q + 1])
    out['onsets_per_s'] = float(f[OUT_ONSETS_PER_S])
    out.update(sync_clips_nonfinite=int(words[OUT_NONFINITE]), sync_clips_seen=int(words[OUT_SEEN]), sync_index_errors=int(words[OUT_INDEX_ERRORS]))
    return out


merge_tables = partial(_record_table.merge_tables, seen=SEEN)  # (tables) -> per clip the record of the lowest rank that has seen it


def save_table(path, records, tol, sigma):
    np.savez(path, table=np.asarray(records, dtype=np.int64), columns=np.array(COLUMN_NAMES), tolerance_ticks=np.int64(tol),
             sigma=np.float64(sigma))


def row_values(rec, hops):
    """one (24,) row record of a whole recording -> per part {beats, precision, recall, offset_ms, beat_align, beats_per_s}, onsets_per_s"""
    rec = np.ascontiguousarray(np.asarray(rec, dtype=np.int64))
    f, T, onsets = rec.view(np.float64), int(rec[ROW_FRAMES]), int(rec[ROW_ONSETS])
    out = {'onsets': onsets, 'onsets_per_s': float(_quotient(onsets * 100.0, hops)), 'nonfinite': int(rec[ROW_NONFINITE]), 'frames': T}
    for p, name in enumerate(PARTS):
        n = int(rec[4 + p])
        out[name] = {'beats': n, 'precision': float(_quotient(float(rec[8 + p]), n)), 'recall': float(_quotient(float(rec[16 + p]), onsets)),
                     'offset_ms': float(_quotient(float(rec[12 + p]) * (1000.0 / 300.0), n)), 'beat_align': float(_quotient(f[p], n)),
                     'beats_per_s': float(_quotient(n * 15.0, T))}
    return out


def describe_row(rec, hops):
    """one line for the log"""
    v = row_values(rec, hops)
    msg = '%d onsets (%.2f/s) over %d frames' % (v['onsets'], v['onsets_per_s'], v['frames'])
    for name in ('all', 'hands'):
        msg += '  %s: %d beats precision %.4f recall %.4f offset %.1f ms align %.4f' % (
            name, v[name]['beats'], v[name]['precision'], v[name]['recall'], v[name]['offset_ms'], v[name]['beat_align'])
    return msg + ('  NONFINITE' if v['nonfinite'] else '')


# ---- the device route (csrc/sync_metrics.hip) ------------------------------------------------------------------------------------------------
class _Device:
    """the two launches of the detector and of a pose tensor's rows, with a workspace that is kept while the shape stays"""

    def __init__(self, K, tol, table, device, parts=None, delta=DELTA, floor=FLOOR, gamma=GAMMA):
        import torch
        from . import _lib
        self.K = check_keypoints(K)
        self.tol, self.gauss, self.parts = check_tol(tol), _table(table), check_parts(parts, self.K)
        self.delta, self.floor, self.gamma = float(delta), float(floor), float(gamma)
        self.device = cuda_device(device, _NO_GPU)
        self._lib = _lib.load()
        self._parts_dev = torch.from_numpy(self.parts).to(self.device)
        self._gauss_dev = torch.from_numpy(self.gauss).to(self.device)
        self._shape, self._bufs = None, None

    _p = staticmethod(ptr)

    def _stream(self):
        return stream(self.device)

    def buffers(self, B, L, R, T):
        """-> (work bytes, ticks (B, cap) int32, info (B, 2) int64, rows of the prediction and of the ground truth (R, 24) int64)"""
        if self._shape != (B, L, R, T):
            import torch
            nbytes, cap = int(self._lib.sdt_sync_workspace_bytes(B, L, R, T)), int(self._lib.sdt_sync_onset_capacity(L))
            if nbytes < 0 or cap < 0:
                raise ValueError('sizes outside the ranges: %d samples (at most 160 * 2^28), %d frames (at most 2^24)' % (L, T))
            self._bufs = (torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=self.device),
                          torch.empty((B, cap), dtype=torch.int32, device=self.device), torch.empty((B, 2), dtype=torch.int64, device=self.device),
                          torch.empty((R, ROW_COLS), dtype=torch.int64, device=self.device),
                          torch.empty((R, ROW_COLS), dtype=torch.int64, device=self.device))
            self._shape = (B, L, R, T)
        return self._bufs

    def audio(self, x):
        import torch
        if not torch.is_tensor(x) or x.device != self.device:
            raise RuntimeError('%s take tensors on %s; %s' % (_NOUN, self.device, _NO_GPU))
        if x.dtype != torch.float32 or x.ndim != 2 or x.shape[0] < 1:
            raise TypeError('audio must be (clips, samples) float32, got %s %s' % (tuple(x.shape), x.dtype))
        return x.detach().contiguous()

    def poses(self, x):
        return check_poses(x, self.K, self.device, _NOUN, _NO_GPU)

    def run_onsets(self, audio, bufs):
        from . import _lib
        work, ticks, info = bufs[:3]
        _lib.check(self._lib.sdt_sync_onsets_f64(self._p(audio), audio.shape[0], audio.shape[1], self.delta, self.floor, self._p(work),
                                                 self._p(ticks), ticks.shape[1], self._p(info), self._stream()))

    def run_rows(self, poses, bufs, rows):
        from . import _lib
        work, ticks, info = bufs[:3]
        _lib.check(self._lib.sdt_sync_rows_f64(self._p(poses), self._p(self._parts_dev), poses.shape[0], poses.shape[1], self.K, ticks.shape[0],
                                               self._p(ticks), ticks.shape[1], self._p(info), self._p(self._gauss_dev), self.tol, self.gamma,
                                               self._p(work), self._p(rows), self._stream()))


class SyncAccumulator(RecordTable):
    """A table of ``num_clips`` clip records on ``device`` and its epoch values.

    ``add`` enqueues the launches of one validation step on the current stream (the detector: envelope, onsets; per pose tensor: speeds,
    beats-and-matching; one commit): no host synchronisation, and no allocation once the workspace has the step's shape.  ``result`` is the
    only call that waits for the device.  The state is one (num_clips + 1, 48) int64 tensor: the records, then a header row whose word 0
    counts the clip indices outside the table (``RecordTable`` owns it, ``state``, ``table``, ``reset``, ``result`` and ``result_words``)."""

    NOUN, NO_GPU = _NOUN, _NO_GPU

    def __init__(self, num_clips, K, tol_ticks, sigma, device='cuda', parts=None):
        num_clips = check_num_clips(num_clips)
        self._dev = _Device(K, tol_ticks, gauss_table(sigma), device, parts)
        self.K, self.tol, self.sigma, self.parts = self._dev.K, self._dev.tol, float(sigma), self._dev.parts
        RecordTable.__init__(self, num_clips, self._dev.device, COLS, COLS, OUT_COLS)

    def add(self, pred, gt, audio, clip_index, multiple=1):
        """one validation step: rows (multiple * B, T, 2, K) of final poses, copy j of clip b in row j * B + b (``gt`` may be None); ``audio``
        (B, L) float32, or (multiple * B, L) as ``mutiply_batch`` leaves it: the first B rows are read, and so are the first B entries of the
        int64 ``clip_index``"""
        import torch
        from . import _lib
        d = self._dev
        pred, gt, idx, B, R, T, m = self._step(pred, gt, clip_index, multiple, gt_optional=True)
        audio = d.audio(audio)
        if audio.shape[0] not in (B, R):
            raise ValueError('audio of %d clips for %d (or %d) rows' % (audio.shape[0], B, R))
        audio = audio[:B]
        bufs = d.buffers(B, audio.shape[1], R, T)
        with torch.cuda.device(self.device):
            d.run_onsets(audio, bufs)
            d.run_rows(pred, bufs, bufs[3])
            if gt is not None:
                d.run_rows(gt, bufs, bufs[4])
            _lib.check(d._lib.sdt_sync_commit(d._p(bufs[3]), None if gt is None else d._p(bufs[4]), d._p(idx), B, m, T, audio.shape[1],
                                              d._p(self._state), self.num_clips, d._stream()))

    def _launch_epoch(self, ptrs, ranks, stream):
        d = self._dev
        return d._lib.sdt_sync_epoch(ptrs, ranks, self.num_clips, d._p(self._epoch_work), d._p(self._out), stream)

    def epoch_values(self, words):
        return epoch_values(words)


def _cuda(x, what):
    import torch
    if not torch.is_tensor(x) or x.device.type != 'cuda':
        raise RuntimeError('%s must be a CUDA tensor; %s' % (what, _NO_GPU))
    return x


def onsets(audio, delta=DELTA, floor=FLOOR, details=False):
    """audio (B, L) or (L,) float32 on the GPU -> the clips' onset ticks, a list of B int64 arrays; ``details``: also the envelopes (B, Nf),
    the onset strengths (B, Nf) and the nonfinite flags (B,) as numpy arrays"""
    import torch
    audio = _cuda(audio, 'the audio')
    audio = audio[None] if audio.ndim == 1 else audio
    d = _Device(1, 1, 1.0, audio.device, parts=[0], delta=delta, floor=floor)
    audio = d.audio(audio)
    B, L = audio.shape
    bufs = d.buffers(B, L, 0, 0)
    with torch.cuda.device(d.device):
        d.run_onsets(audio, bufs)
    info, ticks, Nf = bufs[2].cpu().numpy(), bufs[1].cpu().numpy(), L // HOP
    out = [ticks[b, :info[b, 0]].astype(np.int64) for b in range(B)]
    if not details:
        return out
    f = bufs[0][:2 * B * Nf].cpu().numpy().view(np.float64)
    return out, f[:B * Nf].reshape(B, Nf), f[B * Nf:].reshape(B, Nf), info[:, 1] != 0


def _rows_of(d, poses, audio):
    """the launches of one pose tensor (R, T, 2, K) against audio (B, L) (None: no onsets); -> (rows tensor (R, 24), bufs)"""
    import torch
    poses = d.poses(poses)
    R, T = poses.shape[:2]
    if audio is None:
        bufs = d.buffers(1, 0, R, T)
        with torch.cuda.device(d.device):
            bufs[2].zero_()
    else:
        audio = d.audio(audio)
        if R % audio.shape[0]:
            raise ValueError('%d rows are not copies of %d clips' % (R, audio.shape[0]))
        bufs = d.buffers(audio.shape[0], audio.shape[1], R, T)
        with torch.cuda.device(d.device):
            d.run_onsets(audio, bufs)
    with torch.cuda.device(d.device):
        d.run_rows(poses, bufs, bufs[3])
    return bufs[3], bufs


def beats(poses, parts=None, gamma=GAMMA, details=False):
    """poses (R, T, 2, K) float64 on the GPU -> per row the four parts' beat ticks, a list of R lists of 4 int64 arrays; ``details``: also the
    speeds (R, T - 1, 4) as a numpy array"""
    poses = _cuda(poses, 'the poses')
    if poses.ndim != 4:
        raise TypeError('poses must be (rows, frames, 2, K) float64, got %s' % (tuple(poses.shape),))
    d = _Device(poses.shape[3], 1, 1.0, poses.device, parts=parts, gamma=gamma)
    _, bufs = _rows_of(d, poses, None)
    R, T = poses.shape[:2]
    n_speed = R * (T - 1) * 4
    flags = bufs[0].view(-1).cpu().numpy().view(np.uint8)[n_speed * 8:n_speed * 8 + R * 4 * T].reshape(R, 4, T) != 0
    out = [[beat_ticks(flags[r, p]) for p in range(4)] for r in range(R)]
    if not details:
        return out
    return out, bufs[0][:n_speed].cpu().numpy().view(np.float64).reshape(R, T - 1, 4)


def row_records(poses, audio, tol, sigma, parts=None):
    """poses (R, T, 2, K) float64 and audio (B, L) float32 on the GPU (row r belongs to clip r % B) -> the (R, 24) row records on the GPU"""
    poses = _cuda(poses, 'the poses')
    if poses.ndim != 4:
        raise TypeError('poses must be (rows, frames, 2, K) float64, got %s' % (tuple(poses.shape),))
    d = _Device(poses.shape[3], tol, gauss_table(sigma), poses.device, parts=parts)
    return _rows_of(d, poses, _cuda(audio, 'the audio'))[0].clone()


def recording_report(poses, audio, tol, sigma, parts=None):
    """a whole recording: poses (F, 2, K) float64 and audio (L,) float32 on the GPU -> its (24,) row record on the GPU (one row, T = F)"""
    poses, audio = _cuda(poses, 'the poses'), _cuda(audio, 'the audio')
    if poses.ndim != 3 or audio.ndim != 1:
        raise TypeError('a recording is poses (F, 2, K) and audio (L,), got %s and %s' % (tuple(poses.shape), tuple(audio.shape)))
    return row_records(poses[None], audio[None].float(), tol, sigma, parts)[0]


# ---- command line ------------------------------------------------------------------------------------------------------------------------------
def load_audio(path):
    """-> (clips, L) float32 samples at 16000 Hz from a .npy ((R, L) or (L,)) or a 16-bit PCM .wav (one clip, the first channel)"""
    if str(path).lower().endswith('.wav'):
        import wave
        with wave.open(str(path), 'rb') as w:
            if w.getframerate() != SAMPLE_RATE or w.getsampwidth() != 2:
                raise ValueError('%s: the synchrony metrics need 16-bit PCM at %d Hz, got %d bytes at %d Hz' % (
                    path, SAMPLE_RATE, w.getsampwidth(), w.getframerate()))
            x = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2').reshape(-1, w.getnchannels())[:, 0]
        return (x.astype(np.float32) / np.float32(32768.0))[None]
    x = np.asarray(np.load(path), dtype=np.float32)
    if x.ndim not in (1, 2):
        raise ValueError('%s: audio must be (L,) or (clips, L), got %s' % (path, x.shape))
    return x[None] if x.ndim == 1 else x


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='audio onsets against motion beats of saved results, computed on the GPU')
    ap.add_argument('poses', metavar='POSES.npz', help='a results npz: poses_pred_batch (R, T, 2, K), and poses_gt_batch if it has one')
    ap.add_argument('audio', metavar='AUDIO.wav|.npy', help='the audio of those R clips: (R, L) or (L,) samples at 16000 Hz')
    ap.add_argument('--tolerance', type=float, default=0.1, metavar='s', help='a beat within this many seconds of an onset is a hit')
    ap.add_argument('--sigma', type=float, default=0.1, metavar='s', help='the width of the Gaussian of beat_align, in seconds')
    ap.add_argument('--out', default=None, metavar='table.npz', help='write the table, its column names, the tolerance in ticks and sigma')
    a = ap.parse_args(argv)
    try:
        a.tolerance_ticks = tolerance_ticks(a.tolerance)
        gauss_table(a.sigma)
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None):
    a = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    with np.load(a.poses) as z:
        if 'poses_pred_batch' not in z.files:
            raise KeyError('%s has no entry poses_pred_batch (it has %s)' % (a.poses, ', '.join(z.files)))
        pred = np.asarray(z['poses_pred_batch'], dtype=np.float64)
        gt = np.asarray(z['poses_gt_batch'], dtype=np.float64) if 'poses_gt_batch' in z.files else None
    audio = load_audio(a.audio)
    if pred.ndim != 4 or pred.shape[2] != 2 or audio.shape[0] != pred.shape[0]:
        raise ValueError('poses %s must be (R, T, 2, K) and the audio %s one clip per row' % (pred.shape, audio.shape))
    R = pred.shape[0]
    acc = SyncAccumulator(R, pred.shape[3], a.tolerance_ticks, a.sigma, 'cuda')
    acc.add(torch.from_numpy(pred).cuda(), None if gt is None else torch.from_numpy(gt).cuda(), torch.from_numpy(np.ascontiguousarray(audio)).cuda(),
            torch.arange(R, dtype=torch.int64))
    for k, v in acc.result().items():
        if gt is None and '_gt' in k:
            continue
        print('%s: %s' % (k, ('%d' % v) if isinstance(v, int) else repr(float(v))))
    if a.out:
        save_table(a.out, acc.table().cpu().numpy(), a.tolerance_ticks, a.sigma)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
