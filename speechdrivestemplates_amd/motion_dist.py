"""Histograms of speed, acceleration and jerk magnitudes of final poses and their Hellinger distances (TEST.MOTION_DIST).

Inputs are those of ``clip_metrics``: final float64 poses ``pred`` and ``gt`` of shape (R, T, 2, K) and a part table of K bytes in {0, 1, 2}
(body, face, hands).  Parts are indexed p = 0 all, 1 body, 2 face, 3 hands; sources s = 0 prediction, 1 ground truth; orders o = 0 speed,
1 acceleration, 2 jerk.  Differences are successive, every subtraction rounded on its own, per coordinate:

    d1(t) = x(t+1) - x(t)        d2(t) = d1(t+1) - d1(t)        d3(t) = d2(t+1) - d2(t)

(not the expanded stencil), so order o has T - 1 - o terms per keypoint and none for T <= o + 1.  q = dx dx + dy dy as ``_norm2`` forms it.  Per
order there are NB = 32 bins with NB - 1 ascending inner edges; the bin of a term is the number of SQUARED inner edges <= q (the squares e e
are rounded once on the host and travel in the same table), so no count depends on the device's square root: a q equal to a squared edge
belongs to the upper bin, +inf to the last bin, a NaN is counted nowhere and sets the record's ``nonfinite`` word.  Per clip with
TEST.MULTIPLE = m copies (copy j of clip b is row j * B + b):

    count[s][o][part][b]   integers summed over the copies, part in {body, face, hands} ("all" is their sum, formed at the epoch stage)
    mag_sum[s][o][p]       the sum of sqrt(q): per frame through ``_part_sums``, then over t in order from +0.0, then over the copies in order
                           (exactly how clip_metrics forms speed_pred)
    seen, copies, nonfinite, frames

and per epoch, for every order and part, the Bhattacharyya coefficient BC = sum_b sqrt((cp_b / np) (cg_b / ng)) of the merged histograms, the
Hellinger distance H = sqrt(max(1 - BC, 0)), the same two between the ground truth of the clips with an even index and of those with an odd
index (the noise floor: how large H is between two halves of the real data at this validation-set size) and the ratio of the magnitude sums.

Two routes that run the same operations in the same order.  ``motion_dist_model`` / ``epoch_model`` are the contract in numpy.
``MotionDistAccumulator`` (csrc/motion_dist.hip) keeps a table of clip records on the GPU under the ``RecordTable`` protocol; nothing is
copied to the host before ``result()``.  There is no CPU fallback.

    python -m speechdrivestemplates_amd.motion_dist results/*.npz [--multiple M] [--worst N] [--out hist.npz]

reads ``poses_pred_batch`` / ``poses_gt_batch`` from the results/*.npz files of TEST.SAVE_NPZ (clips are numbered in file order), runs the
device route and prints the epoch values and the N clips with the largest per-clip hand-speed Hellinger distance (computed on the host from
the table).

The default edges are a geometric ladder from 2^-5 to 2^5 final-pose pixels per frame^o, the same for every order.  The constants are
untuned: nobody has looked at what they do to real speakers' motion.
"""
from functools import partial

import numpy as np

from . import _record_table
from ._exact_model import MAX_COPIES, MAX_K, PARTS, _norm2, _ordered_sum, _part_sums, check_parts
from ._record_table import RecordTable, check_keypoints, check_num_clips
from .clip_metrics import load_poses

NB, NE = 32, 31  # bins and inner edges per order
ORDERS = ('speed', 'accel', 'jerk')
SOURCES = ('pred', 'gt')
COLS = 316  # words of a record (SDT_MOTION_DIST_COLS)
FLOATS, COUNT0, NCOUNTS = 24, 24, 576  # float64 words [0, 24): mag_sum at 12 s + 4 o + p; the counts as int32 pairs in words [24, 312)
SEEN, COPIES, NONFINITE, FRAMES = 312, 313, 314, 315
MAX_T = 65536
CHUNK_WORDS = 896  # words of a chunk partial of the epoch stage (sdt_motion_dist_epoch_work_words)
# words of the epoch vector (include/sdt_hip.h): float64 in groups of 12 = (order, part), then three int64
OUT_COLS = 64
OUT_H, OUT_BC, OUT_H_FLOOR, OUT_BC_FLOOR, OUT_RATIO = 0, 12, 24, 36, 48
OUT_SEEN, OUT_NONFINITE, OUT_INDEX_ERRORS = 60, 61, 62
COLUMN_NAMES = (tuple('mag_sum_%s_%s_%s' % (s, o, p) for s in SOURCES for o in ORDERS for p in PARTS) +
                tuple('counts_%d_%d' % (2 * w, 2 * w + 1) for w in range(NCOUNTS // 2)) + ('seen', 'copies', 'nonfinite', 'frames'))
BOOKKEEPING = ('motion_clips_seen', 'motion_index_errors')  # entries of result() that are not metrics (the Trainer warns about the second)
_NO_GPU = ('the motion histograms are computed on the GPU (csrc/motion_dist.hip); there is no CPU fallback (motion_dist_model is the numpy '
           'contract)')


# ---- edges -------------------------------------------------------------------------------------------------------------------------------------
def default_edges():
    """(3, 31) float64: inner edge j of every order is 2 ** ((j - 15) / 3), from 2^-5 to 2^5 (untuned)"""
    return np.tile(np.float64(2.0) ** ((np.arange(NE, dtype=np.float64) - 15.0) / 3.0), (3, 1))


def check_edges(edges=None):
    """-> (3, 31) float64; ValueError unless three lists of 31 finite numbers > 0, strictly ascending, whose squares are finite and > 0 too.
    None is the default ladder."""
    if edges is None:
        return default_edges()
    try:
        ok = len(edges) == 3 and all(len(row) == NE for row in edges)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError('the edges must be three lists (speed, accel, jerk) of %d numbers, got %r' % (NE, edges))
    for row in edges:
        for e in row:
            if isinstance(e, (bool, np.bool_)) or not isinstance(e, (int, float, np.integer, np.floating)):
                raise ValueError('every edge must be a number, got %r' % (e,))
    e = np.array([[float(v) for v in row] for row in edges], dtype=np.float64)
    with np.errstate(all='ignore'):
        sq = e * e
    if not (np.isfinite(e).all() and (e > 0).all() and np.isfinite(sq).all() and (sq > 0).all()):
        raise ValueError('every edge must be finite and > 0, and so must its square')
    if not (e[:, 1:] > e[:, :-1]).all():
        raise ValueError('the edges of every order must be strictly ascending')
    return e


def edge_table(edges):
    """(3, 31) checked edges -> the (3, 2, 31) float64 table the kernels read: per order the edges, then their squares rounded once here"""
    e = np.asarray(edges, dtype=np.float64)
    return np.ascontiguousarray(np.stack([e, e * e], axis=1))


# ---- packing -----------------------------------------------------------------------------------------------------------------------------------
def pack(counts):
    """(n, 2, 3, 3, 32) counts in [0, 2^31) -> the (n, 288) int64 words [24, 312) of a record: two int32 per word, the even one low"""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, NCOUNTS)
    if ((c < 0) | (c >= 2 ** 31)).any():
        raise ValueError('a packed count must lie in [0, 2^31)')
    return c[:, 0::2] | (c[:, 1::2] << 32)


def unpack_counts(words):
    """(n, 288) int64 words -> (n, 2, 3, 3, 32) int64 counts [source][order][body, face, hands][bin]"""
    w = np.ascontiguousarray(np.asarray(words, dtype=np.int64)).view(np.uint64)
    c = np.empty((w.shape[0], NCOUNTS), dtype=np.int64)
    c[:, 0::2] = (w & np.uint64(0xffffffff)).astype(np.int64)
    c[:, 1::2] = (w >> np.uint64(32)).astype(np.int64)
    return c.reshape(-1, 2, 3, 3, NB)


def unpack(records):
    """(n, 316) int64 records -> {'mag_sum': (n, 2, 3, 4) float64, 'counts': (n, 2, 3, 3, 32) int64, 'seen', 'copies', 'nonfinite', 'frames'}"""
    records = np.ascontiguousarray(np.asarray(records, dtype=np.int64))
    return dict(mag_sum=records[:, :FLOATS].copy().view(np.float64).reshape(-1, 2, 3, 4), counts=unpack_counts(records[:, COUNT0:SEEN]),
                seen=records[:, SEEN], copies=records[:, COPIES], nonfinite=records[:, NONFINITE], frames=records[:, FRAMES])


# ---- the numpy contract model ------------------------------------------------------------------------------------------------------------------
def _differences(x):
    """(R, T, 2, K) -> [d1, d2, d3], successive differences along t (each subtraction rounded on its own; an order without a term is empty)"""
    out = []
    for _ in range(3):
        x = x[:, 1:] - x[:, :-1]
        out.append(x)
    return out


def row_records_model(pred, gt, parts, edges=None):
    """the (R, 316) int64 records of sdt_motion_dist_rows_f64 (float64 words viewed as int64)"""
    pred, gt = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    if pred.ndim != 4 or pred.shape[2] != 2 or pred.shape != gt.shape:
        raise ValueError('poses must be two (rows, frames, 2, K) arrays of one shape, got %s and %s' % (pred.shape, gt.shape))
    R, T, _, K = pred.shape
    if not 1 <= K <= MAX_K or not 1 <= T <= MAX_T:
        raise ValueError('K = %d outside [1, %d] or T = %d outside [1, %d]' % (K, MAX_K, T, MAX_T))
    parts = check_parts(parts, K)
    e2 = edge_table(check_edges(edges))[:, 1]
    floats, counts = np.zeros((R, 2, 3, 4)), np.zeros((R, 2, 3, 3, NB), dtype=np.int64)
    nan_term = np.zeros(R, dtype=bool)
    with np.errstate(all='ignore'):
        for s, x in enumerate((pred, gt)):
            for o, d in enumerate(_differences(x)):
                if d.shape[1] == 0:
                    continue
                q = _norm2(d[:, :, 0], d[:, :, 1])  # (R, T - 1 - o, K)
                floats[:, s, o] = _ordered_sum(_part_sums(np.sqrt(q), parts), 1)
                isnan = np.isnan(q)
                nan_term |= isnan.any(axis=(1, 2))
                bins = np.searchsorted(e2[o], q.ravel(), side='right').reshape(q.shape)
                for part in range(3):
                    for r in range(R):
                        sel = (~isnan[r]) & (parts == part)
                        counts[r, s, o, part] = np.bincount(bins[r][sel], minlength=NB)[:NB]
    rec = np.zeros((R, COLS), dtype=np.int64)
    rec[:, :FLOATS] = floats.reshape(R, FLOATS).view(np.int64)
    rec[:, COUNT0:SEEN] = pack(counts)
    rec[:, SEEN], rec[:, COPIES], rec[:, FRAMES] = 1, 1, T
    rec[:, NONFINITE] = nan_term | ~np.isfinite(floats).all(axis=(1, 2, 3))
    return rec


def motion_dist_model(pred, gt, parts, edges=None, multiple=1):
    """the (B, 316) int64 clip records the device route commits for rows (R = multiple * B, T, 2, K): the same operations in the same order"""
    pred = np.asarray(pred, dtype=np.float64)
    m = int(multiple)
    if pred.ndim != 4 or not 1 <= m <= MAX_COPIES or pred.shape[0] % m:
        raise ValueError('%d rows are not %d copies of a batch (copies in [1, %d])' % (pred.shape[0], m, MAX_COPIES))
    R, T, _, K = pred.shape
    if m * T * K >= 2 ** 31:
        raise ValueError('m * T * K = %d must stay below 2^31 (a clip\'s counts are packed as int32)' % (m * T * K))
    B = R // m
    rows = row_records_model(pred, gt, parts, edges)
    with np.errstate(all='ignore'):
        floats = _ordered_sum(rows[:, :FLOATS].copy().view(np.float64).reshape(m, B, FLOATS), 0)
    rec = np.zeros((B, COLS), dtype=np.int64)
    rec[:, :FLOATS] = floats.view(np.int64)
    rec[:, COUNT0:SEEN] = pack(unpack_counts(rows[:, COUNT0:SEEN]).reshape(m, B, NCOUNTS).sum(axis=0))
    rec[:, SEEN], rec[:, COPIES], rec[:, FRAMES] = 1, m, T
    rec[:, NONFINITE] = (rows[:, NONFINITE].reshape(m, B).sum(axis=0) != 0) | ~np.isfinite(floats).all(axis=1)
    return rec


def with_all(counts):
    """(..., 3, 32) counts per part -> (..., 4, 32) with "all", the sum of the three parts, in front"""
    counts = np.asarray(counts, dtype=np.int64)
    return np.concatenate([counts.sum(axis=-2, keepdims=True), counts], axis=-2)


def hellinger_model(cp, cg):
    """two histograms of integer counts -> (BC, H) float64: BC = sum_b sqrt((cp_b / np) (cg_b / ng)) in bin order from +0.0, every operation
    rounded on its own; H = sqrt(max(1 - BC, +0.0)); both 0.0 if either histogram is empty"""
    cp, cg = np.asarray(cp, dtype=np.int64), np.asarray(cg, dtype=np.int64)
    n_p, n_g = int(cp.sum()), int(cg.sum())
    if n_p == 0 or n_g == 0:
        return np.float64(0.0), np.float64(0.0)
    bc = np.float64(0.0)
    for a, b in zip(cp, cg):
        bc = bc + np.sqrt((np.float64(a) / np.float64(n_p)) * (np.float64(b) / np.float64(n_g)))
    d = np.float64(1.0) - bc
    return bc, np.sqrt(np.float64(0.0) if d < 0 else d)


def epoch_model(tables, index_errors=0):
    """-> (the 64 words of sdt_motion_dist_epoch, its (2, 3, 4, 32) int64 merged histograms) over ``tables``, a list of (N, 316) int64 record
    arrays, one per rank"""
    tot_f = np.zeros(FLOATS)
    pred, even, odd = (np.zeros((3, 3, NB), dtype=np.int64) for _ in range(3))
    seen = bad = 0
    tables = [np.asarray(t, dtype=np.int64) for t in tables]
    N = tables[0].shape[0]
    with np.errstate(all='ignore'):
        for c, n0 in enumerate(range(0, N, _record_table.CHUNK)):
            f = np.zeros(FLOATS)
            for n in range(n0, min(N, n0 + _record_table.CHUNK)):
                rec = next((t[n] for t in tables if t[n, SEEN] != 0), None)
                if rec is None:
                    continue
                seen += 1
                if rec[NONFINITE] != 0:
                    bad += 1
                    continue
                f = f + rec[:FLOATS].copy().view(np.float64)
                counts = unpack_counts(rec[None, COUNT0:SEEN])[0]
                pred += counts[0]
                (odd if n & 1 else even)[...] += counts[1]
            tot_f = tot_f + f
        hist = np.stack([with_all(pred), with_all(even + odd)])  # (2, 3, 4, 32)
        floor = np.stack([with_all(even), with_all(odd)])
        out = np.zeros(OUT_COLS)
        for o in range(3):
            for p in range(4):
                r = 4 * o + p
                out[OUT_BC + r], out[OUT_H + r] = hellinger_model(hist[0, o, p], hist[1, o, p])
                out[OUT_BC_FLOOR + r], out[OUT_H_FLOOR + r] = hellinger_model(floor[0, o, p], floor[1, o, p])
                out[OUT_RATIO + r] = np.float64(0.0) if tot_f[12 + r] == 0 else tot_f[r] / tot_f[12 + r]
    words = out.view(np.int64).copy()
    words[OUT_SEEN], words[OUT_NONFINITE], words[OUT_INDEX_ERRORS], words[63] = seen, bad, index_errors, 0
    return words, hist


def epoch_values(words, full=False):
    """the 64 words of the epoch vector -> the named values.  ``full``: also the body and face parts, every floor and the coefficients (the
    command line and the npz; the Trainer logs the short list)"""
    words = np.ascontiguousarray(np.asarray(words, dtype=np.int64))
    f = words.view(np.float64)
    hands = PARTS.index('hands')
    out = {}
    for o, name in enumerate(ORDERS):
        out['hellinger_' + name] = float(f[OUT_H + 4 * o])
        out['hellinger_%s_hands' % name] = float(f[OUT_H + 4 * o + hands])
        out['hellinger_%s_floor' % name] = float(f[OUT_H_FLOOR + 4 * o])
    for o, name in enumerate(ORDERS):
        if o > 0:  # (speed_ratio stays with TEST.CLIP_METRICS)
            out[name + '_ratio'] = float(f[OUT_RATIO + 4 * o])
            out[name + '_ratio_hands'] = float(f[OUT_RATIO + 4 * o + hands])
    if full:
        for o, name in enumerate(ORDERS):
            for p, part in enumerate(PARTS):
                sfx = '' if p == 0 else '_' + part
                out.setdefault('hellinger_%s%s' % (name, sfx), float(f[OUT_H + 4 * o + p]))
                out.setdefault('hellinger_%s%s_floor' % (name, sfx), float(f[OUT_H_FLOOR + 4 * o + p]))
                out['bc_%s%s' % (name, sfx)] = float(f[OUT_BC + 4 * o + p])
                out['bc_%s%s_floor' % (name, sfx)] = float(f[OUT_BC_FLOOR + 4 * o + p])
                out.setdefault('%s_ratio%s' % (name, sfx), float(f[OUT_RATIO + 4 * o + p]))
    out.update(motion_clips_nonfinite=int(words[OUT_NONFINITE]), motion_clips_seen=int(words[OUT_SEEN]),
               motion_index_errors=int(words[OUT_INDEX_ERRORS]))
    return out


def clip_hellinger(records, order=0, part=3):
    """per record the Hellinger distance between its own prediction and ground-truth histograms of ``order`` and ``part`` (host, from the
    table; NaN where the clip has no record, is nonfinite or has no term)"""
    u = unpack(records)
    counts = with_all(u['counts'])  # (n, 2, 3, 4, 32)
    out = np.full(len(counts), np.nan)
    for i in range(len(counts)):
        cp, cg = counts[i, 0, order, part], counts[i, 1, order, part]
        if u['seen'][i] != 0 and u['nonfinite'][i] == 0 and cp.sum() > 0 and cg.sum() > 0:
            out[i] = hellinger_model(cp, cg)[1]
    return out


def tb_histogram_fields(counts, edges):
    """one merged histogram of 32 counts and its 31 inner edges -> (min, max, num, sum, sum_squares, bucket_limit, bucket) for
    ``add_histogram_raw``.  The bucket limits are the edges and DBL_MAX.  The table keeps no moments, so min / max / sum / sum_squares come
    FROM THE BIN EDGES: min is the lower edge of the first bin with a count (0 for bin 0), max the upper edge of the last one (the last
    edge for bin 31), sum and sum_squares take every bin at the midpoint of those two."""
    counts, edges = np.asarray(counts, dtype=np.int64).reshape(NB), np.asarray(edges, dtype=np.float64).reshape(NE)
    lo, hi = np.concatenate([[0.0], edges]), np.concatenate([edges, edges[-1:]])
    mid = 0.5 * (lo + hi)
    nz = np.flatnonzero(counts)
    vmin, vmax = (float(lo[nz[0]]), float(hi[nz[-1]])) if len(nz) else (0.0, 0.0)
    return (vmin, vmax, float(counts.sum()), float((counts * mid).sum()), float((counts * mid * mid).sum()),
            [float(e) for e in edges] + [float(np.finfo(np.float64).max)], [float(c) for c in counts])


merge_tables = partial(_record_table.merge_tables, seen=SEEN)  # (tables) -> per clip the record of the lowest rank that has seen it


def save_table(path, records, edges, histograms):
    np.savez(path, table=np.asarray(records, dtype=np.int64), columns=np.array(COLUMN_NAMES), edges=np.asarray(edges, dtype=np.float64),
             histograms=np.asarray(histograms, dtype=np.int64), orders=np.array(ORDERS), parts=np.array(PARTS), sources=np.array(SOURCES))


# ---- the device route (csrc/motion_dist.hip) ---------------------------------------------------------------------------------------------------
class MotionDistAccumulator(RecordTable):
    """A table of ``num_clips`` clip records on ``device`` and its epoch values.

    ``add`` enqueues two launches on the current stream: no host synchronisation, and no allocation once the workspace has the step's row
    count (inputs that are not contiguous are made so, which allocates).  ``result`` is the only call that waits for the device.  The state
    is one (num_clips + 1, 316) int64 tensor (``RecordTable`` owns it, ``state``, ``table``, ``reset``, ``result`` and ``result_words``);
    ``histograms`` gives the merged histograms of the last ``result``."""

    NOUN, NO_GPU = 'the motion histograms', _NO_GPU

    def __init__(self, num_clips, K, edges=None, device='cuda', parts=None):
        import torch
        from . import _lib
        num_clips, self.K = check_num_clips(num_clips), check_keypoints(K)
        self.edges, self.parts = check_edges(edges), check_parts(parts, self.K)
        RecordTable.__init__(self, num_clips, device, COLS, CHUNK_WORDS, OUT_COLS)
        self._lib = _lib.load()
        if self._lib.sdt_motion_dist_epoch_work_words(self.num_clips) != self._epoch_work.numel():
            raise RuntimeError('the library asks for %d workspace words, this binding allocates %d'
                               % (self._lib.sdt_motion_dist_epoch_work_words(self.num_clips), self._epoch_work.numel()))
        self._parts_dev = torch.from_numpy(self.parts).to(self.device)
        self._edges_dev = torch.from_numpy(edge_table(self.edges)).to(self.device)
        self._hist = torch.zeros((2, 3, 4, NB), dtype=torch.int64, device=self.device)
        self._rows = None

    def _row_workspace(self, R):
        if self._rows is None or self._rows.shape[0] != R:
            import torch
            self._rows = torch.empty((R, COLS), dtype=torch.int64, device=self.device)
        return self._rows

    def row_records(self, pred, gt):
        """the (R, 316) records of the rows alone (sdt_motion_dist_rows_f64), a tensor that the next call overwrites"""
        import torch
        from . import _lib
        pred, gt = self._poses(pred), self._poses(gt)
        if pred.shape != gt.shape:
            raise ValueError('prediction %s and ground truth %s differ in shape' % (tuple(pred.shape), tuple(gt.shape)))
        R, T = pred.shape[:2]
        rows = self._row_workspace(R)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sdt_motion_dist_rows_f64(self._p(pred), self._p(gt), self._p(self._parts_dev), self._p(self._edges_dev),
                                                          R, T, self.K, self._p(rows), self._stream()))
        return rows

    def add(self, pred, gt, clip_index, multiple=1):
        """one validation step: rows (multiple * B, T, 2, K) of final poses, copy j of clip b in row j * B + b; ``clip_index``: the B table rows
        (an int64 tensor of B entries, or of multiple * B as ``mutiply_batch`` leaves it: the first B are read)"""
        import torch
        from . import _lib
        pred, gt, idx, B, R, T, m = self._step(pred, gt, clip_index, multiple)
        rows = self._row_workspace(R)
        with torch.cuda.device(self.device):
            s = self._stream()
            _lib.check(self._lib.sdt_motion_dist_rows_f64(self._p(pred), self._p(gt), self._p(self._parts_dev), self._p(self._edges_dev),
                                                          R, T, self.K, self._p(rows), s))
            _lib.check(self._lib.sdt_motion_dist_commit(self._p(rows), self._p(idx), B, m, T, self.K, self._p(self._state), self.num_clips, s))

    def _launch_epoch(self, ptrs, ranks, stream):
        return self._lib.sdt_motion_dist_epoch(ptrs, ranks, self.num_clips, self._p(self._epoch_work), self._p(self._out), self._p(self._hist),
                                               stream)

    def histograms(self):
        """the (2, 3, 4, 32) int64 merged histograms [source][order][part][bin] of the last ``result`` / ``result_words``, as a numpy array
        (zeros before the first one; a device-to-host copy)"""
        return self._hist.cpu().numpy()

    def epoch_values(self, words):
        return epoch_values(words)


# ---- command line ------------------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='speed, acceleration and jerk histograms of saved results and their Hellinger distances, on the GPU')
    ap.add_argument('files', nargs='+', metavar='FILE.npz', help='results/*.npz files of TEST.SAVE_NPZ (poses_pred_batch, poses_gt_batch)')
    ap.add_argument('--multiple', type=int, default=1, help='TEST.MULTIPLE of the run that wrote the files (rows are copy-major)')
    ap.add_argument('--worst', type=int, default=5, metavar='N', help='print the N clips with the largest hand-speed Hellinger distance')
    ap.add_argument('--out', default=None, metavar='hist.npz', help='write the table, the edges and the merged histograms')
    a = ap.parse_args(argv)
    if not 1 <= a.multiple <= MAX_COPIES:
        ap.error('--multiple outside [1, %d]' % MAX_COPIES)
    if a.worst < 0:
        ap.error('--worst must be >= 0')
    return a


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
    acc = MotionDistAccumulator(sum(p.shape[0] // a.multiple for p, _ in sets), K, None, 'cuda')
    origin, lo = [], 0
    for f, (pred, gt) in zip(a.files, sets):
        B = pred.shape[0] // a.multiple
        acc.add(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), torch.arange(lo, lo + B, dtype=torch.int64), a.multiple)
        origin += [(f, b) for b in range(B)]
        lo += B
    res = epoch_values(acc.result_words(), full=True)
    for k, v in res.items():
        print('%s: %s' % (k, ('%d' % v) if isinstance(v, int) else repr(float(v))))
    records = acc.table().cpu().numpy()
    h = clip_hellinger(records)
    order = [int(i) for i in np.argsort(-np.nan_to_num(h, nan=-np.inf), kind='stable')[:a.worst]]
    for i in order:
        print('worst: clip %d (%s row %d) hellinger_speed_hands %r' % (i, origin[i][0], origin[i][1], float(h[i])))
    if a.out:
        save_table(a.out, records, acc.edges, acc.histograms())
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
