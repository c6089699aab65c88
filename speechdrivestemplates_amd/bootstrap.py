"""Bootstrap intervals and paired comparison for the per-clip validation metrics (TEST.BOOTSTRAP).

Every epoch value of ``clip_metrics`` is a fixed function of column sums over one record per clip.  A non-parametric bootstrap resamples the
clips with replacement ``R`` times, sums every replicate's records, pushes the sums through the same final divisions and reports, per value,
the percentile interval between the order statistics at ranks ``a`` and ``R - 1 - a`` of the R replicate values, a = floor(R (1 - LEVEL) / 2).
For two table sets over the same clips (two checkpoints; the plain and the fitted prediction of one) both are resampled with the SAME draws:
the interval of the difference A - B and the share of replicates in which A is below resp. above B.

Four stages (the dict of ``stages_model`` / ``device_stages`` holds every word of each):

    dense      the live clips -- the lowest rank that has seen a clip gives its record; live = seen and not nonfinite, in BOTH sets of the
               paired form -- in clip order as n rows of W = 39 words: the 20 float sums, the 16 hit counts, copies * frames,
               copies * (frames - 1), copies * (copies - 1) / 2 * frames.  The point row (row R of ``sums``) adds them as the epoch stage does:
               chunks of 64 clips of the TABLE in index order, then the chunk partials in order, so its values are ``result()``'s bits.
    sums       generic (``draws_model`` / ``replicate_sums_model`` know nothing of clip metrics): draw i of replicate r is row
               (uint64(w) n) >> 32, w = word i & 3 of Philox4x32-10 with the counter (i >> 2, 3, r, 0) -- ``augment.py`` keeps the purpose
               in counter word 1 and has 0 .. 2 taken -- and the key (seed low word, seed high word).  A row's probability is off by at
               most n 2^-32.  A replicate adds its n rows in chunks of 64 DRAWS in draw order, then the chunk partials in order; float
               words with one rounding per add, integer words exactly.
    values     the final divisions of ``clip_metrics.epoch_model`` on each of the R + 1 sum rows: (R + 1, 36) float64 and the pair-frame
               count per row.  The paired form also holds A - B word by word.
    intervals  per column the two order statistics over the R replicate rows (not the point row), in the order of radix_select.h's
               ``order_key``: each is one of the inputs.  Paired: also the numbers of replicates with d < 0, d > 0, d == 0.

n == 0: no sums, values or intervals (the named results are empty).  n == 1: every replicate is the point row.  The diversity values are
named only where the point row's pair-frame count is positive.  Percentile intervals are not bias-corrected, and clips cut from one recording
are not independent: on such sets the intervals are optimistic.

Two routes that run the same operations in the same order.  ``stages_model`` / ``intervals_model`` / ``paired_model`` are the contract in numpy;
``device_stages`` / ``clip_metric_intervals`` / ``clip_metric_paired`` run csrc/bootstrap.hip on tables that live on the GPU.  There is no CPU
fallback.

    python -m speechdrivestemplates_amd.bootstrap TABLE.npz [--replicates R] [--level L] [--seed S] [--part-sizes all body face hands] [--out ci.npz]
    python -m speechdrivestemplates_amd.bootstrap compare A.npz B.npz [the same options]

read the ``*-clip_metrics.npz`` files of TEST.SAVE_NPZ (``table``, ``columns``, ``alphas``) and print ``key: point [lo, hi]`` resp.
``key: A B diff [lo, hi] share(A<B)`` (clips are paired by table row).
"""
from fractions import Fraction

import numpy as np

from . import _record_table
from . import clip_metrics as cm
from ._exact_model import MAX_TABLES, PARTS
from ._record_table import CHUNK
from .augment import _key, philox4x32

W, FLOATS, VALUES = 39, 20, 36  # words of a dense row (SDT_BOOTSTRAP_CLIP_WORDS), its float words, value words of a sum row
POS, VEL, PAIR = 36, 37, 38  # derived words of a dense row: copies * frames, copies * (frames - 1), pairs * frames
DENSE_WORK = 80  # workspace words per chunk of stage 1 (SDT_BOOTSTRAP_DENSE_WORK)
PURPOSE = 3  # counter word 1 of every draw (0 .. 2: augment.py, pose_augment.py)
MIN_REPLICATES, MAX_REPLICATES = 100, 20000
VALUE_NAMES = tuple('%s_%s' % (g, p) for g in ('L2', 'PCK_a0', 'PCK_a1', 'PCK_a2', 'PCK_a3', 'PCK', 'speed_ratio', 'vel_L2', 'diversity')
                    for p in PARTS)
GAIN_KEYS = ('L2_hands', 'PCK', 'PCK_hands')  # what the validation observer reports of the fitted-against-plain comparison
_NO_GPU = 'the bootstrap runs on the GPU (csrc/bootstrap.hip); there is no CPU fallback (intervals_model / paired_model are the numpy contract)'


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------------
def check_replicates(replicates):
    if isinstance(replicates, bool) or not isinstance(replicates, (int, np.integer)) or not MIN_REPLICATES <= replicates <= MAX_REPLICATES:
        raise ValueError('the number of replicates must be an integer from %d to %d, got %r' % (MIN_REPLICATES, MAX_REPLICATES, replicates))
    return int(replicates)


def check_seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 1 << 64:
        raise ValueError('the seed must be an integer in [0, 2^64), got %r' % (seed,))
    return int(seed)


def rank_of(replicates, level):
    """a = floor(R (1 - LEVEL) / 2), exact on the decimal form of LEVEL (0.9 means 9/10); ValueError unless 0 < LEVEL < 1 and a < R / 2"""
    if isinstance(level, bool) or not isinstance(level, (int, float)) or not 0 < level < 1:
        raise ValueError('the level must be a number in (0, 1), got %r' % (level,))
    a = int(replicates * (1 - Fraction(repr(float(level)))) / 2)
    if not 0 <= 2 * a < replicates:
        raise ValueError('level %r puts the rank %d outside [0, %d / 2)' % (level, a, replicates))
    return a


def value_columns(alphas, pair_frames):
    """[(key, word of a value row)] in the key order of ``clip_metrics.epoch_values``, led by L2 (all keypoints); the diversity only where the
    pair-frame count is positive"""
    hands = PARTS.index('hands')
    cols = [('L2', cm.OUT_L2)] + [(cm.alpha_name(a), cm.OUT_PCK + 4 * i) for i, a in enumerate(alphas)]
    cols += [('PCK', cm.OUT_PCK_MEAN), ('PCK_hands', cm.OUT_PCK_MEAN + hands)]
    cols += [('L2_' + PARTS[p], cm.OUT_L2 + p) for p in (1, 2, 3)]
    cols += [('speed_ratio', cm.OUT_SPEED_RATIO), ('speed_ratio_hands', cm.OUT_SPEED_RATIO + hands), ('vel_L2', cm.OUT_VEL)]
    if pair_frames > 0:
        cols += [('diversity', cm.OUT_DIV), ('diversity_hands', cm.OUT_DIV + hands)]
    return cols


# ---- the numpy contract model ------------------------------------------------------------------------------------------------------------------
def _dense_rows(records):
    """(m, 40) records -> (m, 39) dense rows"""
    out = np.zeros((records.shape[0], W), dtype=np.int64)
    out[:, :cm.SEEN] = records[:, :cm.SEEN]
    copies, frames = records[:, cm.COPIES], records[:, cm.FRAMES]
    out[:, POS], out[:, VEL], out[:, PAIR] = copies * frames, copies * (frames - 1), copies * (copies - 1) // 2 * frames
    return out


def _floats(words):
    return np.ascontiguousarray(words[..., :FLOATS]).view(np.float64)


def _table_order_sum(rows, live):
    """the dense rows of the live clips summed as the epoch stage sums: per chunk of 64 table rows in order, then the chunk partials in order"""
    tot_f, tot_i = np.zeros(FLOATS), np.zeros(W - FLOATS, dtype=np.int64)
    f, h = _floats(rows), rows[:, FLOATS:]
    row = 0
    with np.errstate(all='ignore'):
        for n0 in range(0, live.shape[0], CHUNK):
            pf, ph = np.zeros(FLOATS), np.zeros(W - FLOATS, dtype=np.int64)
            for n in range(n0, min(live.shape[0], n0 + CHUNK)):
                if live[n]:
                    pf, ph, row = pf + f[row], ph + h[row], row + 1
            tot_f, tot_i = tot_f + pf, tot_i + ph
    return np.concatenate([tot_f.view(np.int64), tot_i])


def dense_model(tables_a, tables_b=None):
    """-> (n, [dense (n, 39) per set], [point sums (39,) per set]); ``tables_*``: lists of (N, 40) int64 record arrays, one per rank"""
    merged = [cm.merge_tables(t) for t in ((tables_a,) if tables_b is None else (tables_a, tables_b))]
    if len(merged) == 2 and merged[0].shape != merged[1].shape:
        raise ValueError('the two table sets differ in shape: %s and %s' % (merged[0].shape, merged[1].shape))
    live = np.ones(merged[0].shape[0], dtype=bool)
    for m in merged:
        live &= (m[:, cm.SEEN] != 0) & (m[:, cm.NONFINITE] == 0)
    dense = [_dense_rows(m[live]) for m in merged]
    return int(live.sum()), dense, [_table_order_sum(d, live) for d in dense]


def draws_model(n, replicates, seed):
    """(R, n) int64: the row that draw i of replicate r takes"""
    blocks = (n + 3) // 4
    counter = np.zeros((replicates, blocks, 4), dtype=np.uint64)
    counter[..., 0], counter[..., 1], counter[..., 2] = np.arange(blocks), PURPOSE, np.arange(replicates)[:, None]
    words = philox4x32(counter, _key(seed)).reshape(replicates, blocks * 4)[:, :n].astype(np.uint64)
    return ((words * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def replicate_sums_model(dense, float_words, replicates, seed):
    """(n, words) int64 rows, the first ``float_words`` float64 -> (R, words): every replicate's drawn rows added in chunks of 64 draws in
    draw order, then the chunk partials in order"""
    dense = np.ascontiguousarray(np.asarray(dense, dtype=np.int64))
    n, words = dense.shape
    rows = draws_model(n, replicates, seed)
    f, h = np.ascontiguousarray(dense[:, :float_words]).view(np.float64), dense[:, float_words:]
    tot_f, tot_i = np.zeros((replicates, float_words)), np.zeros((replicates, words - float_words), dtype=np.int64)
    with np.errstate(all='ignore'):
        for i0 in range(0, n, CHUNK):
            pf = np.zeros((replicates, float_words))
            for i in range(i0, min(n, i0 + CHUNK)):
                pf = pf + f[rows[:, i]]
                tot_i += h[rows[:, i]]
            tot_f = tot_f + pf
    return np.concatenate([tot_f.view(np.int64), tot_i], axis=1)


def _quotients(x, n):
    return np.where(n == 0, 0.0, x / np.where(n == 0, 1, n).astype(np.float64))


def values_model(sums, sizes, num_alphas):
    """(M, 39) sum rows -> ((M, 36) float64 values, (M,) pair-frame counts): the final divisions of ``clip_metrics.epoch_model``"""
    sums = np.asarray(sums, dtype=np.int64)
    f, h = _floats(sums), sums[:, FLOATS:]
    out = np.zeros((sums.shape[0], VALUES))
    with np.errstate(all='ignore'):
        for p in range(4):
            n_pos, n_vel, n_div = h[:, POS - FLOATS] * sizes[p], h[:, VEL - FLOATS] * sizes[p], h[:, PAIR - FLOATS] * sizes[p]
            out[:, cm.OUT_L2 + p] = _quotients(f[:, p], n_pos)
            mean = np.zeros(sums.shape[0])
            for a in range(num_alphas):
                out[:, cm.OUT_PCK + 4 * a + p] = _quotients(h[:, 4 * a + p].astype(np.float64), n_pos)
                mean = mean + out[:, cm.OUT_PCK + 4 * a + p]
            out[:, cm.OUT_PCK_MEAN + p] = mean / np.float64(num_alphas)
            den = f[:, 8 + p]
            out[:, cm.OUT_SPEED_RATIO + p] = np.where(den == 0, 0.0, f[:, 4 + p] / np.where(den == 0, 1.0, den))
            out[:, cm.OUT_VEL + p] = _quotients(f[:, 12 + p], n_vel)
            out[:, cm.OUT_DIV + p] = _quotients(f[:, 16 + p], n_div)
    return out, sums[:, PAIR].copy()


_SIGN = np.uint64(1 << 63)


def order_key(v):
    """float64 -> uint64 of the same order (radix_select.h)"""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | _SIGN)


def order_value(key):
    key = np.ascontiguousarray(key, dtype=np.uint64)
    return np.where(key >> np.uint64(63) != 0, key & ~_SIGN, ~key).view(np.float64)


def select_model(values, rank):
    """(R, C) float64 -> (C, 2): per column the order statistics at ranks ``rank`` and R - 1 - rank"""
    keys = np.sort(order_key(values), axis=0)
    return np.ascontiguousarray(order_value(np.stack([keys[rank], keys[values.shape[0] - 1 - rank]], axis=1)))


def signs_model(values):
    """(R, C) -> (C, 3) int64: per column the number of values < 0, > 0, == 0"""
    return np.stack([(values < 0).sum(axis=0), (values > 0).sum(axis=0), (values == 0).sum(axis=0)], axis=1).astype(np.int64)


def stages_model(tables_a, tables_b, sizes, num_alphas, replicates, rank, seed):
    """every word of every stage: {'n', 'dense_a', 'sums_a' (R + 1, 39; row R is the point row), 'values_a' (R + 1, 36), 'pair_frames_a'
    (R + 1,), 'lohi_a' (36, 2)} and in the paired form the same with _b, 'diff' (R + 1, 36), 'lohi_diff' and 'signs' (36, 3).  With n == 0
    only 'n' and the empty dense rows."""
    n, dense, point = dense_model(tables_a, tables_b)
    out = {'n': n}
    for tag, d, pt in zip('ab', dense, point):
        out['dense_' + tag] = d
        if n == 0:
            continue
        sums = np.concatenate([replicate_sums_model(d, FLOATS, replicates, seed), pt[None]], axis=0)
        values, pairs = values_model(sums, sizes, num_alphas)
        out.update({'sums_' + tag: sums, 'values_' + tag: values, 'pair_frames_' + tag: pairs, 'lohi_' + tag: select_model(values[:replicates], rank)})
    if n and tables_b is not None:
        with np.errstate(all='ignore'):
            out['diff'] = out['values_a'] - out['values_b']
        out['lohi_diff'], out['signs'] = select_model(out['diff'][:replicates], rank), signs_model(out['diff'][:replicates])
    return out


def named_intervals(st, alphas, replicates):
    """the stages of a single table set -> {key: (point, lo, hi)}"""
    if st['n'] == 0:
        return {}
    point, lohi = st['values_a'][replicates], st['lohi_a']
    return {k: (float(point[c]), float(lohi[c, 0]), float(lohi[c, 1])) for k, c in value_columns(alphas, st['pair_frames_a'][replicates])}


def named_paired(st, alphas, replicates):
    """the stages of the paired form -> {key: {'a', 'b', 'diff', 'diff_lo', 'diff_hi', 'share_a_less', 'share_a_greater'}}"""
    if st['n'] == 0:
        return {}
    R = replicates
    pairs = min(int(st['pair_frames_a'][R]), int(st['pair_frames_b'][R]))  # diversity: only where both point rows have pairs
    return {k: {'a': float(st['values_a'][R, c]), 'b': float(st['values_b'][R, c]), 'diff': float(st['diff'][R, c]),
                'diff_lo': float(st['lohi_diff'][c, 0]), 'diff_hi': float(st['lohi_diff'][c, 1]),
                'share_a_less': int(st['signs'][c, 0]) / R, 'share_a_greater': int(st['signs'][c, 1]) / R}
            for k, c in value_columns(alphas, pairs)}


def _numpy_tables(tables):
    tables = np.asarray(tables, dtype=np.int64)
    if tables.ndim not in (2, 3) or tables.shape[-1] != cm.COLS:
        raise ValueError('tables must be (clips, 40) or (ranks, clips, 40) records, got %s' % (tables.shape,))
    return list(tables) if tables.ndim == 3 else [tables]


def intervals_model(tables, sizes, alphas, replicates=1000, level=0.95, seed=0):
    """``clip_metric_intervals`` over numpy tables ((N, 40), (ranks, N, 40) or a list of (N, 40)): {key: (point, lo, hi)}"""
    alphas, R = cm.check_alphas(list(alphas)), check_replicates(replicates)
    return named_intervals(stages_model(_numpy_tables(tables), None, sizes, len(alphas), R, rank_of(R, level), check_seed(seed)), alphas, R)


def paired_model(a, b, sizes, alphas, replicates=1000, level=0.95, seed=0):
    """``clip_metric_paired`` over numpy tables"""
    alphas, R = cm.check_alphas(list(alphas)), check_replicates(replicates)
    return named_paired(stages_model(_numpy_tables(a), _numpy_tables(b), sizes, len(alphas), R, rank_of(R, level), check_seed(seed)), alphas, R)


# ---- the device route (csrc/bootstrap.hip) -----------------------------------------------------------------------------------------------------
def _call(name, *args):
    """one entry of the library (the tests count the launches through this)"""
    from . import _lib
    _lib.check(getattr(_lib.load(), name)(*args))


def _device_tables(x, gathered=None):
    """an accumulator (with its ``gathered`` states), a (N, 40) / (ranks, N, 40) int64 CUDA tensor or a list of (N, 40) ones -> (table
    pointers, their number, N, the device, what owns the memory)"""
    import ctypes as C
    import torch
    if isinstance(x, _record_table.RecordTable):
        if x._state.shape[1] != cm.COLS:
            raise ValueError('the bootstrap takes clip-metrics tables (%d words a record)' % cm.COLS)
        ptrs, ranks, keep = x.table_pointers(gathered)  # (a state is its table followed by the header row)
        return ptrs, ranks, x.num_clips, x.device, keep
    if gathered is not None:
        raise ValueError('gathered states come with an accumulator')
    blocks = list(x.unbind(0)) if torch.is_tensor(x) and x.ndim == 3 else [x] if torch.is_tensor(x) else list(x)
    if not 1 <= len(blocks) <= MAX_TABLES:
        raise ValueError('%d tables; the bootstrap takes 1 to %d' % (len(blocks), MAX_TABLES))
    for b in blocks:
        if not torch.is_tensor(b) or b.device.type != 'cuda':
            raise RuntimeError(_NO_GPU)
        if b.dtype != torch.int64 or b.ndim != 2 or b.shape != blocks[0].shape or b.shape[0] < 1 or b.shape[1] != cm.COLS or \
                b.device != blocks[0].device or not b.is_contiguous():
            raise ValueError('every table must be a contiguous (clips, 40) int64 tensor on one device')
    return (C.c_void_p * len(blocks))(*[b.data_ptr() for b in blocks]), len(blocks), blocks[0].shape[0], blocks[0].device, blocks


def device_stages(a, b, sizes, num_alphas, replicates, rank, seed, gathered_a=None, gathered_b=None, events=None):
    """``stages_model`` on the device: the same dict, as numpy arrays copied back at the end (``a`` / ``b`` as ``_device_tables`` takes them;
    ``b`` None = one set).  ``events``: a list that receives a recorded torch.cuda.Event at the start and after every stage."""
    import ctypes as C
    import torch
    p = _record_table.ptr
    ptrs_a, ranks_a, N, device, keep_a = _device_tables(a, gathered_a)
    ptrs_b, ranks_b, keep_b = None, 0, None
    if b is not None:
        ptrs_b, ranks_b, N_b, device_b, keep_b = _device_tables(b, gathered_b)
        if N_b != N or device_b != device:
            raise ValueError('the two table sets differ: %d clips on %s and %d clips on %s' % (N, device, N_b, device_b))
    R, tags = int(replicates), ('a',) if b is None else ('a', 'b')
    sizes_c = (C.c_int64 * 4)(*[int(s) for s in sizes])

    def mark():
        if events is not None:
            events.append(torch.cuda.Event(enable_timing=True))
            events[-1].record()

    with torch.cuda.device(device):
        stream = _record_table.stream(device)
        kw = dict(dtype=torch.int64, device=device)
        t = {}
        for tag in tags:
            t['dense_' + tag], t['sums_' + tag] = torch.empty((N, W), **kw), torch.empty((R + 1, W), **kw)
        work, n_dev = torch.empty((-(-N // CHUNK), DENSE_WORK), **kw), torch.empty(1, **kw)
        mark()
        _call('sdt_clip_metrics_replicate_dense', ptrs_a, ranks_a, ptrs_b, ranks_b, N, p(work), p(t['dense_a']), p(t.get('dense_b')),
              p(t['sums_a'][R]), p(t['sums_b'][R]) if b is not None else None, p(n_dev), stream)
        n = int(n_dev.cpu()[0])  # (the one wait before the end: the grid of the next stage needs it)
        mark()
        out = {'n': n}
        if n == 0:
            for tag in tags:
                out['dense_' + tag] = np.zeros((0, W), dtype=np.int64)
            return out
        work = torch.empty(R * -(-n // CHUNK) * W, **kw)
        for tag in tags:  # (the same seed: both sets take the same draws)
            _call('sdt_bootstrap_sums', p(t['dense_' + tag]), n, W, FLOATS, R, C.c_uint64(seed), p(work), p(t['sums_' + tag]), stream)
        mark()
        for tag in tags:
            t['values_' + tag] = torch.empty((R + 1, VALUES), dtype=torch.float64, device=device)
            t['pair_frames_' + tag] = torch.empty(R + 1, **kw)
            _call('sdt_clip_metrics_replicate_values', p(t['sums_' + tag]), R + 1, sizes_c, num_alphas, p(t['values_' + tag]),
                  p(t['pair_frames_' + tag]), stream)
        if b is not None:
            t['diff'] = torch.empty_like(t['values_a'])
            _call('sdt_bootstrap_diff_f64', p(t['values_a']), p(t['values_b']), (R + 1) * VALUES, p(t['diff']), stream)
        mark()
        for tag in tags + (('diff',) if b is not None else ()):
            src = t['diff'] if tag == 'diff' else t['values_' + tag]
            t['lohi_' + tag] = torch.empty((VALUES, 2), dtype=torch.float64, device=device)
            if tag == 'diff':
                t['signs'] = torch.empty((VALUES, 3), **kw)
            _call('sdt_bootstrap_intervals_f64', p(src), R, VALUES, rank, p(t['lohi_' + tag]), p(t.get('signs')) if tag == 'diff' else None, stream)
        mark()
        for k, v in t.items():
            out[k] = v[:n].cpu().numpy() if k.startswith('dense_') else v.cpu().numpy()
    del keep_a, keep_b
    return out


def _arguments(acc, sizes, alphas, replicates, level, seed):
    if isinstance(acc, cm.ClipMetricsAccumulator):
        sizes = cm.part_sizes(acc.parts) if sizes is None else sizes
        alphas = acc.alphas if alphas is None else alphas
    if sizes is None or alphas is None:
        raise ValueError('part sizes and alphas are needed with tables (an accumulator knows its own)')
    sizes = tuple(int(s) for s in sizes)
    if len(sizes) != 4 or not all(0 <= s <= 128 for s in sizes):
        raise ValueError('part sizes must be four counts (all, body, face, hands) in [0, 128], got %r' % (sizes,))
    R = check_replicates(replicates)
    return sizes, cm.check_alphas(list(alphas)), R, rank_of(R, level), check_seed(seed)


def clip_metric_intervals(acc_or_tables, sizes=None, alphas=None, replicates=1000, level=0.95, seed=0, gathered=None, stages=None):
    """-> {key: (point, lo, hi)} for the values of ``clip_metrics.epoch_values`` (and L2 over all keypoints) of a ClipMetricsAccumulator (over
    its own table or the ``gathered`` states of all ranks) or of tables on the GPU; {} when no clip is live.  ``stages``: a dict that
    receives every word of every stage."""
    sizes, alphas, R, rank, seed = _arguments(acc_or_tables, sizes, alphas, replicates, level, seed)
    st = device_stages(acc_or_tables, None, sizes, len(alphas), R, rank, seed, gathered)
    if stages is not None:
        stages.update(st)
    return named_intervals(st, alphas, R)


def clip_metric_paired(a, b, sizes=None, alphas=None, replicates=1000, level=0.95, seed=0, gathered_a=None, gathered_b=None, stages=None):
    """two table sets over the same clips, resampled with the same draws -> {key: {'a', 'b', 'diff', 'diff_lo', 'diff_hi', 'share_a_less',
    'share_a_greater'}}: the point values over the clips live in both, the interval of a - b and the shares of replicates with a < b, a > b"""
    sizes, alphas, R, rank, seed = _arguments(a, sizes, alphas, replicates, level, seed)
    st = device_stages(a, b, sizes, len(alphas), R, rank, seed, gathered_a, gathered_b)
    if stages is not None:
        stages.update(st)
    return named_paired(st, alphas, R)


def save_replicates(path, st, alphas, sizes, replicates, level, seed):
    """the replicate values of one table set, their names, the point row and what made them"""
    R = int(replicates)
    np.savez(path, values=st['values_a'][:R], names=np.array(VALUE_NAMES), point=st['values_a'][R], pair_frames=st['pair_frames_a'],
             n=np.int64(st['n']), replicates=np.int64(R), level=np.float64(level), seed=np.uint64(seed),
             part_sizes=np.asarray(sizes, dtype=np.int64), alphas=np.asarray(alphas, dtype=np.float64))


# ---- command line ------------------------------------------------------------------------------------------------------------------------------
def load_table(path):
    """-> (table (N, 40) int64, alphas) of a *-clip_metrics.npz"""
    with np.load(path) as z:
        for key in ('table', 'columns', 'alphas'):
            if key not in z.files:
                raise KeyError('%s has no entry %r (it has %s)' % (path, key, ', '.join(z.files)))
        table, columns, alphas = np.asarray(z['table'], dtype=np.int64), tuple(str(c) for c in z['columns']), [float(a) for a in z['alphas']]
    if table.ndim != 2 or table.shape[1] != cm.COLS or columns != cm.COLUMN_NAMES:
        raise ValueError('%s: not a clip-metrics table (shape %s)' % (path, table.shape))
    return table, list(cm.check_alphas(alphas))


def parse_args(argv=None):
    import argparse
    import sys
    argv = list(sys.argv[1:] if argv is None else argv)
    compare = bool(argv) and argv[0] == 'compare'
    ap = argparse.ArgumentParser(prog='bootstrap compare' if compare else 'bootstrap',
                                 description='bootstrap intervals of the per-clip validation metrics of saved tables, computed on the GPU')
    if compare:
        ap.add_argument('files', nargs=2, metavar='TABLE.npz', help='two *-clip_metrics.npz files over the same clips (paired by table row)')
    else:
        ap.add_argument('files', nargs=1, metavar='TABLE.npz', help='a *-clip_metrics.npz file of TEST.SAVE_NPZ (table, columns, alphas)')
    ap.add_argument('--replicates', type=int, default=1000, help='resamples of the clips (%d .. %d)' % (MIN_REPLICATES, MAX_REPLICATES))
    ap.add_argument('--level', type=float, default=0.95, help='coverage of the percentile interval, in (0, 1)')
    ap.add_argument('--seed', type=int, default=0, help='Philox key, in [0, 2^64)')
    ap.add_argument('--part-sizes', nargs=4, type=int, default=None, metavar=('ALL', 'BODY', 'FACE', 'HANDS'),
                    help='keypoints per part (default: the 121-keypoint layout)')
    ap.add_argument('--out', default=None, metavar='ci.npz', help='write the keys and what is printed as arrays')
    a = ap.parse_args(argv[1:] if compare else argv)
    a.compare = compare
    try:
        a.replicates, a.seed = check_replicates(a.replicates), check_seed(a.seed)
        a.rank = rank_of(a.replicates, a.level)
    except ValueError as e:
        ap.error(str(e))
    if a.part_sizes is None:
        from .core.datasets.gesture_dataset import PoseTransforms
        a.part_sizes = list(cm.part_sizes(PoseTransforms.part_table()))
    return a


def main(argv=None):
    a = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    loaded = [load_table(f) for f in a.files]
    alphas = loaded[0][1]
    if a.compare and (loaded[0][0].shape != loaded[1][0].shape or loaded[1][1] != alphas):
        raise ValueError('%s and %s differ in shape or alphas' % tuple(a.files))
    tables = [torch.from_numpy(t).cuda() for t, _ in loaded]
    opts = dict(sizes=a.part_sizes, alphas=alphas, replicates=a.replicates, level=a.level, seed=a.seed)
    if a.compare:
        res = clip_metric_paired(tables[0], tables[1], **opts)
        fields = ('a', 'b', 'diff', 'diff_lo', 'diff_hi', 'share_a_less', 'share_a_greater')
        for k, v in res.items():
            print('%s: %r %r %r [%r, %r] %r' % (k, v['a'], v['b'], v['diff'], v['diff_lo'], v['diff_hi'], v['share_a_less']))
        arrays = {f: np.array([v[f] for v in res.values()]) for f in fields}
    else:
        res = clip_metric_intervals(tables[0], **opts)
        for k, (point, lo, hi) in res.items():
            print('%s: %r [%r, %r]' % (k, point, lo, hi))
        arrays = {f: np.array([v[i] for v in res.values()]) for i, f in enumerate(('point', 'lo', 'hi'))}
    if not res:
        print('no live clip: no intervals')
    if a.out:
        np.savez(a.out, keys=np.array(list(res), dtype=str), replicates=np.int64(a.replicates), level=np.float64(a.level), seed=np.uint64(a.seed),
                 **arrays)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
