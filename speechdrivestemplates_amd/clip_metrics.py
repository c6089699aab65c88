"""Per-clip validation metrics on final poses: PCK, part errors, motion speed and diversity (TEST.CLIP_METRICS).

Inputs are final (de-normalised, global, scaled) float64 poses ``pred`` and ``gt`` of shape (R, T, 2, K) and a part table of K bytes in
{0, 1, 2} (body, face, hands; ``PoseTransforms.part_table()``).  Parts are indexed p = 0 all, 1 body, 2 face, 3 hands.  Per row:

    l2_sum[p]       sum over (t, k in p) of sqrt(dx^2 + dy^2), d = pred - gt
    pck_hit[a][p]   the number of (t, k in p) with dx^2 + dy^2 <= (alpha_a * s_t)^2, s_t the larger side of the ground truth's bounding box
                    over all K keypoints of frame t (compared on squares, ``<=``, a NaN is no hit)
    speed_pred[p], speed_gt[p]   sum over (t < T-1, k in p) of |v(t+1) - v(t)|
    vel_l2[p]       the same sum over |(pred(t+1) - pred(t)) - (gt(t+1) - gt(t))|
    nonfinite       1 if any of the row's float sums is not finite

and per clip with TEST.MULTIPLE = m copies (copy j of clip b is row j * B + b): the sum of its m row records in order j = 0..m-1 and
``div_sum[p]``, the sum over the pairs i < j (lexicographic) and (t, k in p) of |pred_i - pred_j|.

Two routes that run the same operations in the same order.  ``clip_metrics_model`` / ``epoch_model`` are the contract in numpy.
``ClipMetricsAccumulator`` (csrc/clip_metrics.hip) keeps a table of clip records on the GPU: every validation step commits its clips' records,
and one launch turns the tables -- one per rank under data parallelism, the lowest rank that has seen a clip wins -- into the epoch values.
Nothing is copied to the host before ``result()``.  There is no CPU fallback.

    python -m speechdrivestemplates_amd.clip_metrics FILE.npz [...] [--alphas 0.1 0.2] [--multiple M] [--worst N] [--out table.npz]

reads ``poses_pred_batch`` / ``poses_gt_batch`` from the results/*.npz files of TEST.SAVE_NPZ (clips are numbered in file order), runs the
device route and prints the epoch values and the N clips with the largest hand error.
"""
from functools import partial

import numpy as np

from . import _record_table
from ._exact_model import LANES, MAX_TABLES  # noqa: F401  (public names of this module)
from ._exact_model import MAX_COPIES, PARTS, _norm2, _ordered_sum, _part_sums, _quotient, check_parts, part_sizes
from ._record_table import CHUNK  # noqa: F401
from ._record_table import RecordTable, check_keypoints, check_num_clips, chunked_records

COLS = 40  # words of a record (SDT_CLIP_METRICS_COLS)
FLOAT_GROUPS = ('l2_sum', 'speed_pred', 'speed_gt', 'vel_l2', 'div_sum')  # words [0, 20): group g, part p at 4 g + p
HIT0, SEEN, COPIES, NONFINITE, FRAMES = 20, 36, 37, 38, 39  # int64 words: pck_hit[a][p] at 20 + 4 a + p
COLUMN_NAMES = tuple('%s_%s' % (g, p) for g in FLOAT_GROUPS for p in PARTS) + tuple('pck_hit_%d_%s' % (a, p) for a in range(4) for p in PARTS) + (
    'seen', 'copies', 'nonfinite', 'frames')
MAX_ALPHAS = 4
# words of the epoch vector (include/sdt_hip.h): float64 [0, 36) in groups of 4 parts, then four int64
OUT_L2, OUT_PCK, OUT_PCK_MEAN, OUT_SPEED_RATIO, OUT_VEL, OUT_DIV = 0, 4, 20, 24, 28, 32
OUT_SEEN, OUT_NONFINITE, OUT_INDEX_ERRORS, OUT_PAIR_FRAMES = 36, 37, 38, 39
_NO_GPU = 'the clip metrics are computed on the GPU (csrc/clip_metrics.hip); there is no CPU fallback (clip_metrics_model is the numpy contract)'


def check_alphas(alphas):
    """-> tuple of floats; ValueError unless one to four finite numbers > 0"""
    if not isinstance(alphas, (list, tuple)) or not 1 <= len(alphas) <= MAX_ALPHAS:
        raise ValueError('PCK alphas must be a list of one to %d numbers, got %r' % (MAX_ALPHAS, alphas))
    for a in alphas:
        if isinstance(a, bool) or not isinstance(a, (int, float)) or not (a == a and 0 < a < float('inf')):
            raise ValueError('every PCK alpha must be a finite number > 0, got %r' % (alphas,))
    return tuple(float(a) for a in alphas)


def alpha_name(a):
    return 'PCK_%g' % a


# ---- the numpy contract model ------------------------------------------------------------------------------------------------------------------
def row_records_model(pred, gt, parts, alphas):
    """the (R, 40) int64 records of sdt_clip_metrics_rows_f64 (float64 words viewed as int64)"""
    pred, gt = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    R, T, _, K = pred.shape
    parts, alphas = check_parts(parts, K), check_alphas(list(alphas))
    with np.errstate(all='ignore'):
        px, py, gx, gy = pred[:, :, 0], pred[:, :, 1], gt[:, :, 0], gt[:, :, 1]
        d2 = _norm2(px - gx, py - gy)
        floats = np.zeros((R, 20))
        floats[:, 0:4] = _ordered_sum(_part_sums(np.sqrt(d2), parts), 1)
        if T > 1:
            vpx, vpy, vgx, vgy = px[:, 1:] - px[:, :-1], py[:, 1:] - py[:, :-1], gx[:, 1:] - gx[:, :-1], gy[:, 1:] - gy[:, :-1]
            floats[:, 4:8] = _ordered_sum(_part_sums(np.sqrt(_norm2(vpx, vpy)), parts), 1)
            floats[:, 8:12] = _ordered_sum(_part_sums(np.sqrt(_norm2(vgx, vgy)), parts), 1)
            floats[:, 12:16] = _ordered_sum(_part_sums(np.sqrt(_norm2(vpx - vgx, vpy - vgy)), parts), 1)
        side_x = np.fmax.reduce(gx, axis=-1) - np.fmin.reduce(gx, axis=-1)
        side_y = np.fmax.reduce(gy, axis=-1) - np.fmin.reduce(gy, axis=-1)
        s = np.fmax(side_x, side_y)  # (R, T)
        rec = np.zeros((R, COLS), dtype=np.int64)
        for a, alpha in enumerate(alphas):
            thr = alpha * s
            hit = d2 <= (thr * thr)[..., None]
            for p in range(4):
                rec[:, HIT0 + 4 * a + p] = (hit if p == 0 else hit & (parts == p - 1)).sum(axis=(1, 2))
    rec[:, :20] = floats.view(np.int64)
    rec[:, SEEN], rec[:, COPIES], rec[:, FRAMES] = 1, 1, T
    rec[:, NONFINITE] = ~np.isfinite(floats[:, :16]).all(axis=1)
    return rec


def clip_metrics_model(pred, gt, parts, alphas, multiple=1):
    """the (B, 40) int64 clip records the device route commits for rows (R = multiple * B, T, 2, K): the same operations in the same order"""
    pred = np.asarray(pred, dtype=np.float64)
    R, T, _, K = pred.shape
    m = int(multiple)
    if not 1 <= m <= MAX_COPIES or R % m:
        raise ValueError('%d rows are not %d copies of a batch (copies in [1, %d])' % (R, m, MAX_COPIES))
    B = R // m
    rows = row_records_model(pred, gt, parts, alphas)
    parts = check_parts(parts, K)
    with np.errstate(all='ignore'):
        floats = np.zeros((B, 20))
        floats[:, :16] = _ordered_sum(rows[:, :16].view(np.float64).reshape(m, B, 16), 0)
        if m > 1:
            copies = pred.reshape(m, B, T, 2, K)
            acc = np.zeros((B, T, K))
            for i in range(m):
                for j in range(i + 1, m):
                    acc = acc + np.sqrt(_norm2(copies[i, :, :, 0] - copies[j, :, :, 0], copies[i, :, :, 1] - copies[j, :, :, 1]))
            floats[:, 16:20] = _ordered_sum(_part_sums(acc, parts), 1)
    rec = np.zeros((B, COLS), dtype=np.int64)
    rec[:, :20] = floats.view(np.int64)
    rec[:, HIT0:SEEN] = rows[:, HIT0:SEEN].reshape(m, B, 16).sum(axis=0)
    rec[:, SEEN], rec[:, COPIES], rec[:, FRAMES] = 1, m, T
    rec[:, NONFINITE] = (rows[:, NONFINITE].reshape(m, B).sum(axis=0) != 0) | ~np.isfinite(floats).all(axis=1)
    return rec


def unpack(records):
    """(n, 40) int64 records -> {'l2_sum' .. 'div_sum': (n, 4) float64, 'pck_hit': (n, 4, 4) int64, 'seen', 'copies', 'nonfinite', 'frames'}"""
    records = np.ascontiguousarray(np.asarray(records, dtype=np.int64))
    out = {g: records[:, 4 * i:4 * i + 4].copy().view(np.float64) for i, g in enumerate(FLOAT_GROUPS)}
    out['pck_hit'] = records[:, HIT0:SEEN].reshape(-1, 4, 4)
    out.update(seen=records[:, SEEN], copies=records[:, COPIES], nonfinite=records[:, NONFINITE], frames=records[:, FRAMES])
    return out


def epoch_model(tables, sizes, num_alphas, index_errors=0):
    """the 40 words of sdt_clip_metrics_epoch over ``tables``, a list of (N, 40) int64 record arrays, one per rank; ``sizes``: part_sizes()"""
    tot_f, tot_i = np.zeros(20), np.zeros(48, dtype=np.int64)
    with np.errstate(all='ignore'):
        for chunk in chunked_records(tables, SEEN):
            f, h = np.zeros(20), np.zeros(48, dtype=np.int64)
            for rec in chunk:
                h[SEEN] += 1
                if rec[NONFINITE] != 0:
                    h[NONFINITE] += 1
                    continue
                f = f + rec[:20].view(np.float64)
                h[HIT0:SEEN] += rec[HIT0:SEEN]
                copies, frames = int(rec[COPIES]), int(rec[FRAMES])
                h[37] += copies * frames
                h[39] += copies * (frames - 1)
                h[40] += copies * (copies - 1) // 2 * frames
            tot_f, tot_i = tot_f + f, tot_i + h
        out = np.zeros(COLS)
        for p in range(4):
            n_pos, n_vel, n_div = int(tot_i[37]) * sizes[p], int(tot_i[39]) * sizes[p], int(tot_i[40]) * sizes[p]
            out[OUT_L2 + p] = _quotient(tot_f[p], n_pos)
            mean = np.float64(0.0)
            for a in range(num_alphas):
                out[OUT_PCK + 4 * a + p] = _quotient(float(tot_i[HIT0 + 4 * a + p]), n_pos)
                mean = mean + out[OUT_PCK + 4 * a + p]
            out[OUT_PCK_MEAN + p] = mean / np.float64(num_alphas)
            out[OUT_SPEED_RATIO + p] = np.float64(0.0) if tot_f[8 + p] == 0 else tot_f[4 + p] / tot_f[8 + p]
            out[OUT_VEL + p] = _quotient(tot_f[12 + p], n_vel)
            out[OUT_DIV + p] = _quotient(tot_f[16 + p], n_div)
    words = out.view(np.int64).copy()
    words[OUT_SEEN], words[OUT_NONFINITE], words[OUT_INDEX_ERRORS], words[OUT_PAIR_FRAMES] = tot_i[SEEN], tot_i[NONFINITE], index_errors, tot_i[40]
    return words


def epoch_values(words, alphas):
    """the 40 words of the epoch vector -> the named values (diversity only when some clip had two or more copies)"""
    words = np.ascontiguousarray(np.asarray(words, dtype=np.int64))
    f = words.view(np.float64)
    hands = PARTS.index('hands')
    out = {alpha_name(a): float(f[OUT_PCK + 4 * i]) for i, a in enumerate(alphas)}
    out['PCK'], out['PCK_hands'] = float(f[OUT_PCK_MEAN]), float(f[OUT_PCK_MEAN + hands])
    for p in (1, 2, 3):
        out['L2_' + PARTS[p]] = float(f[OUT_L2 + p])
    out['speed_ratio'], out['speed_ratio_hands'] = float(f[OUT_SPEED_RATIO]), float(f[OUT_SPEED_RATIO + hands])
    out['vel_L2'] = float(f[OUT_VEL])
    if words[OUT_PAIR_FRAMES] > 0:
        out['diversity'], out['diversity_hands'] = float(f[OUT_DIV]), float(f[OUT_DIV + hands])
    out.update(clips_nonfinite=int(words[OUT_NONFINITE]), clips_seen=int(words[OUT_SEEN]), index_errors=int(words[OUT_INDEX_ERRORS]))
    return out


BOOKKEEPING = ('clips_seen', 'index_errors')  # entries of result() that are not metrics (the Trainer warns about the second)


# ---- the device route (csrc/clip_metrics.hip) -------------------------------------------------------------------------------------------------
class ClipMetricsAccumulator(RecordTable):
    """A table of ``num_clips`` clip records on ``device`` and its epoch values.

    ``add`` enqueues three launches (four with copies) on the current stream: no host synchronisation, and no allocation once the workspace has
    the step's shape (inputs that are not contiguous are made so, which allocates).  ``result`` is the only call that waits for the device.
    The state is one (num_clips + 1, 40) int64 tensor: the records, then a header row whose word 0 counts the clip indices outside the table
    (``RecordTable`` owns it, ``state``, ``table``, ``reset``, ``result`` and ``result_words``)."""
    NOUN, NO_GPU = 'the clip metrics', _NO_GPU

    def __init__(self, num_clips, K, alphas, device='cuda', parts=None):
        import ctypes as C
        import torch
        from . import _lib
        num_clips, self.K = check_num_clips(num_clips), check_keypoints(K)
        self.alphas, self.parts = check_alphas(list(alphas)), check_parts(parts, self.K)
        RecordTable.__init__(self, num_clips, device, COLS, 48, COLS)
        self._lib = _lib.load()
        self._parts_dev = torch.from_numpy(self.parts).to(self.device)
        self._alphas_c = (C.c_double * len(self.alphas))(*self.alphas)
        self._sizes_c = (C.c_int64 * 4)(*part_sizes(self.parts))
        self._work_shape, self._work = None, None

    def _workspace(self, R, T, m):
        if self._work_shape != (R, T, m):
            import torch
            self._work = (torch.empty(R * T * 32, dtype=torch.int64, device=self.device),
                          torch.empty((R, COLS), dtype=torch.int64, device=self.device),
                          torch.empty(R // m * T * 4, dtype=torch.float64, device=self.device) if m > 1 else None)
            self._work_shape = (R, T, m)
        return self._work

    def row_records(self, pred, gt):
        """the (R, 40) records of the rows alone (sdt_clip_metrics_rows_f64), a tensor that the next call overwrites"""
        import torch
        from . import _lib
        pred, gt = self._poses(pred), self._poses(gt)
        if pred.shape != gt.shape:
            raise ValueError('prediction %s and ground truth %s differ in shape' % (tuple(pred.shape), tuple(gt.shape)))
        R, T = pred.shape[:2]
        work, rows, _ = self._workspace(R, T, 1)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sdt_clip_metrics_rows_f64(self._p(pred), self._p(gt), self._p(self._parts_dev), self._alphas_c, len(self.alphas),
                                                           R, T, self.K, self._p(work), self._p(rows), self._stream()))
        return rows

    def add(self, pred, gt, clip_index, multiple=1):
        """one validation step: rows (multiple * B, T, 2, K) of final poses, copy j of clip b in row j * B + b; ``clip_index``: the B table rows
        (an int64 tensor of B entries, or of multiple * B as ``mutiply_batch`` leaves it: the first B are read)"""
        import torch
        from . import _lib
        pred, gt, idx, B, R, T, m = self._step(pred, gt, clip_index, multiple)
        work, rows, div = self._workspace(R, T, m)
        with torch.cuda.device(self.device):
            s = self._stream()
            _lib.check(self._lib.sdt_clip_metrics_rows_f64(self._p(pred), self._p(gt), self._p(self._parts_dev), self._alphas_c, len(self.alphas),
                                                           R, T, self.K, self._p(work), self._p(rows), s))
            if m > 1:
                _lib.check(self._lib.sdt_clip_metrics_diversity_f64(self._p(pred), self._p(self._parts_dev), B, m, T, self.K, self._p(div), s))
            _lib.check(self._lib.sdt_clip_metrics_commit(self._p(rows), self._p(div), self._p(idx), B, m, T, self._p(self._state),
                                                         self.num_clips, s))

    def _launch_epoch(self, ptrs, ranks, stream):
        return self._lib.sdt_clip_metrics_epoch(ptrs, ranks, self.num_clips, self._sizes_c, len(self.alphas), self._p(self._epoch_work),
                                                self._p(self._out), stream)

    def epoch_values(self, words):
        return epoch_values(words, self.alphas)


def device_sqrt(x):
    """sqrt of a float64 device tensor as the kernels compute it (the tests ask whether this device's square root is correctly rounded)"""
    import ctypes as C
    import torch
    from . import _lib
    if not torch.is_tensor(x) or x.device.type != 'cuda' or x.dtype != torch.float64:
        raise RuntimeError(_NO_GPU)
    x = x.contiguous()
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().sdt_clip_metrics_sqrt_f64(C.c_void_p(x.data_ptr()), x.numel(), C.c_void_p(y.data_ptr()),
                                                         torch.cuda.current_stream(x.device).cuda_stream))
    return y


# ---- command line ------------------------------------------------------------------------------------------------------------------------------
def load_poses(path):
    """-> (poses_pred_batch, poses_gt_batch) of one TEST.SAVE_NPZ results file as (R, T, 2, K) float64 arrays"""
    with np.load(path) as z:
        for key in ('poses_pred_batch', 'poses_gt_batch'):
            if key not in z.files:
                raise KeyError('%s has no entry %r (it has %s)' % (path, key, ', '.join(z.files)))
        pred, gt = np.asarray(z['poses_pred_batch'], dtype=np.float64), np.asarray(z['poses_gt_batch'], dtype=np.float64)
    if pred.ndim != 4 or pred.shape[2] != 2 or pred.shape != gt.shape:
        raise ValueError('%s: poses must be two (rows, frames, 2, K) arrays of one shape, got %s and %s' % (path, pred.shape, gt.shape))
    return pred, gt


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='per-clip PCK, part errors, motion speed and diversity of saved results, computed on the GPU')
    ap.add_argument('files', nargs='+', metavar='FILE.npz', help='results/*.npz files of TEST.SAVE_NPZ (poses_pred_batch, poses_gt_batch)')
    ap.add_argument('--alphas', nargs='+', type=float, default=[0.1, 0.2], help='PCK thresholds as fractions of the bounding box (one to four)')
    ap.add_argument('--multiple', type=int, default=1, help='TEST.MULTIPLE of the run that wrote the files (rows are copy-major)')
    ap.add_argument('--worst', type=int, default=5, metavar='N', help='print the N clips with the largest hand error')
    ap.add_argument('--out', default=None, metavar='table.npz', help='write the table, the column names and the alphas')
    a = ap.parse_args(argv)
    a.alphas = list(check_alphas(a.alphas))
    if not 1 <= a.multiple <= MAX_COPIES:
        ap.error('--multiple outside [1, %d]' % MAX_COPIES)
    if a.worst < 0:
        ap.error('--worst must be >= 0')
    return a


def hand_errors(records, sizes):
    """per record the mean hand-keypoint distance (NaN where the clip has no record or no hand keypoint)"""
    u = unpack(records)
    n = (u['copies'] * u['frames'] * sizes[3]).astype(np.float64)
    with np.errstate(all='ignore'):
        return np.where((u['seen'] != 0) & (n > 0), u['l2_sum'][:, 3] / n, np.nan)


merge_tables = partial(_record_table.merge_tables, seen=SEEN)  # (tables) -> per clip the record of the lowest rank that has seen it


def save_table(path, records, alphas):
    np.savez(path, table=np.asarray(records, dtype=np.int64), columns=np.array(COLUMN_NAMES), alphas=np.asarray(alphas, dtype=np.float64))


def main(argv=None):
    a = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    sets = [load_poses(f) for f in a.files]
    for f, (pred, _) in zip(a.files, sets):
        if pred.shape[0] % a.multiple:
            raise ValueError('%s: %d rows are not %d copies of a batch' % (f, pred.shape[0], a.multiple))
    K = sets[0][0].shape[3]
    acc = ClipMetricsAccumulator(sum(p.shape[0] // a.multiple for p, _ in sets), K, a.alphas, 'cuda')
    origin, lo = [], 0
    for f, (pred, gt) in zip(a.files, sets):
        B = pred.shape[0] // a.multiple
        acc.add(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), torch.arange(lo, lo + B, dtype=torch.int64), a.multiple)
        origin += [(f, b) for b in range(B)]
        lo += B
    res = acc.result()
    for k, v in res.items():
        print('%s: %s' % (k, ('%d' % v) if isinstance(v, int) else repr(float(v))))
    records = acc.table().cpu().numpy()
    err = hand_errors(records, part_sizes(acc.parts))
    order = [int(i) for i in np.argsort(-np.nan_to_num(err, nan=np.inf), kind='stable')[:a.worst]]
    for i in order:
        print('worst: clip %d (%s row %d) L2_hands %r' % (i, origin[i][0], origin[i][1], float(err[i])))
    if a.out:
        save_table(a.out, records, a.alphas)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
