"""Precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) between the pose-encoder features of the real and of
the generated clips (TEST.PRDC; DESIGN.md section 33 is the contract, include/sdt_hip.h the layouts).

Real rows a_i (i < Nr) and generated rows b_j (j < Ng) are float64 vectors of D columns, float32 features widened exactly; k is an integer.

    d2(x, y)   the sum over c = 0 .. D-1, in that order from +0.0, of (x_c - y_c)^2; subtract, multiply and add each rounded on its own
    rA(i)      the k-th smallest of {d2(a_i, a_l) : l != i} (self left out by position: duplicates at distance 0 count); +inf when the set
               has at most k rows.  rB(j) the same within the generated set.
    precision  #{j : some i has d2(b_j, a_i) <= rA(i)} / Ng          recall    #{i : some j has d2(a_i, b_j) <= rB(j)} / Nr
    density    sum_j #{i : d2(b_j, a_i) <= rA(i)} / (k Ng)           coverage  #{i : min_j d2(a_i, b_j) <= rA(i)} / Nr

Every comparison is made on d2: no square root, so every value is one float64 division of two integers and the device is held to the numpy
model bit for bit.  A set of at most k rows makes the four values NaN and sets a bit of ``err``; nothing raises.  Per row: for a generated row
its ball count (the inner count of density), the nearest real row (lowest position on a tie), that d2, and rB; for a real row rA, the covered
flag and the recalled flag.

Two routes that compute the same bits.  ``prdc_model`` / ``commit_model`` / ``gather_model`` / ``result_model`` are the contract in numpy, on
whole distance matrices.  ``FeatureSetAccumulator`` (csrc/prdc.hip) keeps a table of the clips' features on the GPU under the record-table
protocol (_record_table.py: one record per clip, the lowest rank that has seen a clip gives it) and ``prdc_device`` takes two plain arrays;
nothing is copied to the host before ``result()``.  There is no CPU fallback.  The ``_floor`` values are the same metric between the real rows
at even and at odd positions of the live, index-ordered list (even = "real", odd = "generated"): what two halves of the real data score at
this set size.

    python -m speechdrivestemplates_amd.prdc A B [--k 5] [--mu-only] [--worst N] [--out rows.npz] [--host]

A holds the real rows and B the generated ones: .npy files of (n, d) features, or results/*.npz files of TEST.SAVE_NPZ (mu_gt ++ logvar_gt of
A, mu_pred ++ logvar_pred of B; --mu-only: the mu columns alone).  Prints the four values, the N generated rows farthest from the real set
(largest nearest-real d2 among the rows no ball holds) and the N real rows nobody covers.  --host computes on the host with the numpy model.

K = 5 is the value of the density / coverage paper; it is untuned for validation sets of a few hundred clips.
"""
import logging

import numpy as np

from . import _record_table
from ._exact_model import MAX_COPIES
from ._record_table import RecordTable, check_num_clips

MAX_DIM, MAX_NEIGHBOURS, MAX_ROWS = 64, 16, 1 << 20
HEADER, COPIES, NONFINITE = 2, 0, 1  # words of a record before its features (SDT_PRDC_HEADER_WORDS); the seen / copies word; the non-finite word
OUT_WORDS = 16  # SDT_PRDC_OUT_WORDS
VALUES = ('precision', 'recall', 'density', 'coverage')  # float64 words 0 .. 3 of the epoch vector; int64 4 .. 7 their numerators
OUT_ROWS_REAL, OUT_ROWS_GEN, OUT_K, OUT_ERR, OUT_SEEN, OUT_NONFINITE, OUT_INDEX_ERRORS = 8, 9, 10, 11, 12, 13, 14
ERR_REAL_ROWS, ERR_GEN_ROWS = 1, 2  # bits of 'err': the real / the generated set has at most k rows
GEN_ROWS = ('gen_ball_count', 'gen_nearest', 'gen_nearest_d2', 'gen_radius')  # per generated row
REAL_ROWS = ('real_radius', 'real_covered', 'real_recalled')  # per real row
MAX_SLICES = 4096
_SLICES = None  # tests only: a forced number of slices of the streamed range (None: sdt_prdc_slices); no result may depend on it
_NO_GPU = 'the feature-set metrics are computed on the GPU (csrc/prdc.hip); there is no CPU fallback (prdc_model is the numpy contract)'


def cols(dim, copies):
    """words of a record (sdt_prdc_cols)"""
    return HEADER + dim * (1 + copies)


def check_k(k):
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_NEIGHBOURS:
        raise ValueError('k must be an integer from 1 to %d, got %r' % (MAX_NEIGHBOURS, k))
    return int(k)


def _check_sets(real, gen):
    real, gen = (np.ascontiguousarray(np.asarray(x, dtype=np.float32), dtype=np.float64) for x in (real, gen))
    if real.ndim != 2 or gen.ndim != 2 or real.shape[1] != gen.shape[1] or not 1 <= real.shape[1] <= MAX_DIM:
        raise ValueError('the sets must be (n, D) arrays of one D in [1, %d], got %s and %s' % (MAX_DIM, real.shape, gen.shape))
    if max(real.shape[0], gen.shape[0]) > MAX_ROWS:
        raise ValueError('a set holds at most %d rows, got %d and %d' % (MAX_ROWS, real.shape[0], gen.shape[0]))
    if not (np.isfinite(real).all() and np.isfinite(gen).all()):
        raise ValueError('the sets must be finite (the accumulator leaves a clip with a non-finite feature out; plain arrays are refused)')
    return real, gen


# ---- the numpy contract model ------------------------------------------------------------------------------------------------------------------
def d2_matrix(x, y):
    """(n, D), (p, D) float64 -> the (n, p) matrix of d2: column by column in order from +0.0, numpy rounds every operation on its own"""
    s = np.zeros((x.shape[0], y.shape[0]))
    for c in range(x.shape[1]):
        t = x[:, c, None] - y[None, :, c]
        s = s + t * t
    return s


def radii_model(x, k):
    """the k-th smallest d2 of every row to the other rows of its set (self left out by position), +inf in a set of at most k rows"""
    n = x.shape[0]
    d = d2_matrix(x, x)
    d[np.arange(n), np.arange(n)] = np.inf
    d = np.concatenate([d, np.full((n, k), np.inf)], axis=1)
    return np.sort(d, axis=1)[:, k - 1]


def prdc_model(real, gen, k):
    """-> {'precision', 'recall', 'density', 'coverage' (float64), 'num_<value>' (int), 'rows_real', 'rows_gen', 'k', 'err', and the per-row
    arrays GEN_ROWS + REAL_ROWS}.  ``real`` (Nr, D) and ``gen`` (Ng, D) are taken as float32 values."""
    k = check_k(k)
    real, gen = _check_sets(real, gen)
    nr, ng = real.shape[0], gen.shape[0]
    ra, rb = radii_model(real, k), radii_model(gen, k)
    d = d2_matrix(gen, real)  # (Ng, Nr)
    inside = d <= ra[None, :]
    balls = inside.sum(axis=1).astype(np.int64)
    nearest = d.argmin(axis=1).astype(np.int64) if nr else np.full(ng, -1, dtype=np.int64)
    nearest_d2 = d.min(axis=1, initial=np.inf)
    covered = d.min(axis=0, initial=np.inf) <= ra
    recalled = (d <= rb[:, None]).any(axis=0)
    err = (ERR_REAL_ROWS if nr <= k else 0) | (ERR_GEN_ROWS if ng <= k else 0)
    nums = dict(precision=int((balls > 0).sum()), recall=int(recalled.sum()), density=int(balls.sum()), coverage=int(covered.sum()))
    dens = dict(precision=ng, recall=nr, density=k * ng, coverage=nr)
    out = {v: np.float64('nan') if err else np.float64(nums[v]) / np.float64(dens[v]) for v in VALUES}
    out.update({'num_' + v: nums[v] for v in VALUES})
    out.update(rows_real=nr, rows_gen=ng, k=k, err=err, gen_ball_count=balls, gen_nearest=nearest, gen_nearest_d2=nearest_d2, gen_radius=rb,
               real_radius=ra, real_covered=covered.astype(np.int64), real_recalled=recalled.astype(np.int64))
    return out


def model_words(res, clips_seen=0, clips_nonfinite=0, index_errors=0):
    """a ``prdc_model`` result -> the 16 int64 words of sdt_prdc_reduce's ``out`` (float64 words viewed as int64)"""
    w = np.zeros(OUT_WORDS, dtype=np.int64)
    w[:4] = np.array([res[v] for v in VALUES], dtype=np.float64).view(np.int64)
    w[4:8] = [res['num_' + v] for v in VALUES]
    w[OUT_ROWS_REAL], w[OUT_ROWS_GEN], w[OUT_K], w[OUT_ERR] = res['rows_real'], res['rows_gen'], res['k'], res['err']
    w[OUT_SEEN], w[OUT_NONFINITE], w[OUT_INDEX_ERRORS] = clips_seen, clips_nonfinite, index_errors
    return w


def new_table(num_clips, dim, copies):
    """the zero state of an accumulator as a numpy array: (num_clips + 1, cols) int64, the header row last"""
    return np.zeros((num_clips + 1, cols(dim, copies)), dtype=np.int64)


def commit_model(table, mu_pred, logvar_pred, mu_gt, logvar_gt, clip_index, copies):
    """what sdt_prdc_commit writes into ``table`` (in place) for one step: rows (copies * B, Dh) float32, copy j of clip b in row j * B + b"""
    feats = [np.asarray(x, dtype=np.float32).astype(np.float64) for x in (mu_pred, logvar_pred, mu_gt, logvar_gt)]
    m, N = int(copies), table.shape[0] - 1
    B, Dh = feats[0].shape[0] // m, feats[0].shape[1]
    pred, gt = np.concatenate(feats[:2], axis=1), np.concatenate(feats[2:], axis=1)  # (m B, D)
    for b, idx in enumerate(np.asarray(clip_index, dtype=np.int64)[:B]):
        if not 0 <= idx < N:
            table[N, 0] += 1
            continue
        row = np.concatenate([gt[b]] + [pred[j * B + b] for j in range(m)])
        table[idx, HEADER:HEADER + 2 * Dh * (1 + m)] = row.view(np.int64)
        table[idx, COPIES], table[idx, NONFINITE] = m, 0 if np.isfinite(row).all() else 1
    return table


def gather_model(tables, dim, copies, dim_used=None, floor=False):
    """(N + 1, cols) int64 states, one per rank -> {'real' (Nr, Du), 'gen' (Ng, Du), 'real_clip', 'gen_clip', 'gen_copy', 'clips_seen',
    'clips_nonfinite', 'index_errors'}: per clip the record of the lowest rank that has seen it, the live clips in index order.  ``floor``:
    the ground truth of the live clips at even positions as ``real``, at odd positions as ``gen``."""
    tables = [np.asarray(t, dtype=np.int64) for t in tables]
    N, m, du = tables[0].shape[0] - 1, int(copies), dim if dim_used is None else int(dim_used)
    merged = _record_table.merge_tables([t[:N] for t in tables], COPIES)
    seen = merged[:, COPIES] != 0
    live = np.flatnonzero(seen & (merged[:, NONFINITE] == 0))
    feats = merged[:, HEADER:].copy().view(np.float64).reshape(N, 1 + m, dim)[live][:, :, :du]
    if floor:
        real, gen = feats[0::2, 0], feats[1::2, 0]
        real_clip, gen_clip, gen_copy = live[0::2], live[1::2], np.zeros(len(live) // 2, dtype=np.int64)
    else:
        real, gen = feats[:, 0], feats[:, 1:].reshape(-1, du)
        real_clip, gen_clip, gen_copy = live, np.repeat(live, m), np.tile(np.arange(m, dtype=np.int64), len(live))
    return dict(real=np.ascontiguousarray(real), gen=np.ascontiguousarray(gen), real_clip=real_clip.astype(np.int64),
                gen_clip=gen_clip.astype(np.int64), gen_copy=gen_copy, clips_seen=int(seen.sum()),
                clips_nonfinite=int((seen & (merged[:, NONFINITE] != 0)).sum()), index_errors=int(sum(t[N, 0] for t in tables)))


def result_model(tables, dim, copies, k, dim_used=None):
    """-> (the 32 words ``FeatureSetAccumulator.result_words`` gives: the usual pass, then the floor pass; the per-row outputs of the usual pass
    with their clip indices, as ``FeatureSetAccumulator.rows`` gives them)"""
    words, rows = [], None
    for floor in (False, True):
        g = gather_model(tables, dim, copies, dim_used, floor)
        res = prdc_model(g['real'], g['gen'], k)
        words.append(model_words(res, g['clips_seen'], g['clips_nonfinite'], g['index_errors']))
        if not floor:
            rows = {key: res[key] for key in GEN_ROWS + REAL_ROWS}
            rows.update(real_clip=g['real_clip'], gen_clip=g['gen_clip'], gen_copy=g['gen_copy'])
    return np.concatenate(words), rows


def result_values(words, dim_used=None):
    """the 32 words of a result -> the named values: the four metrics, their numerators, 'rows_real', 'rows_gen', 'k', 'err', each also with
    the suffix _floor, and the bookkeeping 'clips_seen', 'clips_nonfinite', 'index_errors'"""
    words = np.ascontiguousarray(np.asarray(words, dtype=np.int64))
    out = {}
    for sfx, w in (('', words[:OUT_WORDS]), ('_floor', words[OUT_WORDS:])):
        f = w.view(np.float64)
        out.update({v + sfx: float(f[i]) for i, v in enumerate(VALUES)})
        out.update({'num_' + v + sfx: int(w[4 + i]) for i, v in enumerate(VALUES)})
        out.update({'rows_real' + sfx: int(w[OUT_ROWS_REAL]), 'rows_gen' + sfx: int(w[OUT_ROWS_GEN]), 'err' + sfx: int(w[OUT_ERR])})
    out.update(k=int(words[OUT_K]), clips_seen=int(words[OUT_SEEN]), clips_nonfinite=int(words[OUT_NONFINITE]),
               index_errors=int(words[OUT_INDEX_ERRORS]), dim_used=dim_used)
    return out


def describe_error(res, suffix=''):
    """what the error bits of a result say, '' if none is set"""
    err, k = res['err' + suffix], res['k']
    msgs = ['the %s set has %d row(s), the metric needs more than k = %d' % (name, res[rows + suffix], k)
            for bit, name, rows in ((ERR_REAL_ROWS, 'real', 'rows_real'), (ERR_GEN_ROWS, 'generated', 'rows_gen')) if err & bit]
    return '; '.join(msgs)


# ---- the device route (csrc/prdc.hip) ----------------------------------------------------------------------------------------------------------
def _refuse_capture():
    import torch
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('the feature-set metrics cannot run inside a hipGraph capture (they allocate their workspace and read the result back)')


class _Sets:
    """Two dense row sets of capacities (real_cap, gen_cap) x dim on the device, their count words, every per-row output and the workspace of
    the all-pairs stages; ``run`` launches radii, cross passes and the reduction on the current stream."""

    def __init__(self, real_cap, gen_cap, dim, device):
        import torch
        from . import _lib
        self._lib, self.device, self.real_cap, self.gen_cap, self.dim = _lib.load(), device, int(real_cap), int(gen_cap), int(dim)
        if not (1 <= self.real_cap <= MAX_ROWS and 1 <= self.gen_cap <= MAX_ROWS):
            raise ValueError('a set holds 1 to %d rows, got capacities %d and %d' % (MAX_ROWS, self.real_cap, self.gen_cap))

        def buf(n, dtype):
            return torch.zeros(n, dtype=dtype, device=device)
        self.real, self.gen = buf(self.real_cap * dim, torch.float64), buf(self.gen_cap * dim, torch.float64)
        self.counts = buf(8, torch.int64)
        self.real_clip, self.gen_clip, self.gen_copy = buf(self.real_cap, torch.int64), buf(self.gen_cap, torch.int64), buf(self.gen_cap, torch.int64)
        self.rows = {'real_radius': buf(self.real_cap, torch.float64), 'real_covered': buf(self.real_cap, torch.int64),
                     'real_recalled': buf(self.real_cap, torch.int64), 'gen_radius': buf(self.gen_cap, torch.float64),
                     'gen_ball_count': buf(self.gen_cap, torch.int64), 'gen_nearest': buf(self.gen_cap, torch.int64),
                     'gen_nearest_d2': buf(self.gen_cap, torch.float64)}
        self._real_balls, self._real_nearest, self._real_d2 = (buf(self.real_cap, torch.int64), buf(self.real_cap, torch.int64),
                                                               buf(self.real_cap, torch.float64))
        self._part = None

    def _slices(self, queries, streamed):
        if _SLICES is None:
            return int(self._lib.sdt_prdc_slices(queries, streamed))
        if not 1 <= int(_SLICES) <= MAX_SLICES:
            raise ValueError('%r slices outside [1, %d]' % (_SLICES, MAX_SLICES))
        return int(_SLICES)

    def _workspace(self, words):
        import torch
        if self._part is None or self._part.numel() < words:
            self._part = torch.empty(words, dtype=torch.int64, device=self.device)
        return self._part

    def run(self, dim_used, k, out, stream):
        """``out``: 16 int64 words on the device (sdt_prdc_reduce)"""
        import ctypes as C
        from . import _lib
        lib, p, rows = self._lib, _record_table.ptr, self.rows
        n_real, n_gen = p(self.counts), C.c_void_p(self.counts.data_ptr() + 8)
        for x, n, cap, radius in ((self.real, n_real, self.real_cap, rows['real_radius']), (self.gen, n_gen, self.gen_cap, rows['gen_radius'])):
            s = self._slices(cap, cap)
            part = self._workspace(s * cap * 16)
            _lib.check(lib.sdt_prdc_knn(p(x), n, cap, dim_used, k, s, p(part), part.numel(), p(radius), stream))
        s = self._slices(self.gen_cap, self.real_cap)
        part = self._workspace(s * self.gen_cap * 3)
        _lib.check(lib.sdt_prdc_cross(p(self.gen), n_gen, self.gen_cap, p(self.real), n_real, self.real_cap, p(rows['real_radius']), dim_used, s,
                                      p(part), part.numel(), p(rows['gen_ball_count']), p(rows['gen_nearest']), p(rows['gen_nearest_d2']), stream))
        s = self._slices(self.real_cap, self.gen_cap)
        part = self._workspace(s * self.real_cap * 3)
        _lib.check(lib.sdt_prdc_cross(p(self.real), n_real, self.real_cap, p(self.gen), n_gen, self.gen_cap, p(rows['gen_radius']), dim_used, s,
                                      p(part), part.numel(), p(self._real_balls), p(self._real_nearest), p(self._real_d2), stream))
        _lib.check(lib.sdt_prdc_reduce(p(self.counts), self.real_cap, self.gen_cap, k, p(rows['real_radius']), p(rows['gen_ball_count']),
                                       p(self._real_balls), p(self._real_d2), p(rows['real_covered']), p(rows['real_recalled']), p(out), stream))

    def host_rows(self, n_real, n_gen):
        """the per-row outputs of the last ``run`` as numpy arrays cut to the row counts"""
        out = {key: self.rows[key][:n_gen if key in GEN_ROWS else n_real].cpu().numpy() for key in GEN_ROWS + REAL_ROWS}
        out.update(real_clip=self.real_clip[:n_real].cpu().numpy(), gen_clip=self.gen_clip[:n_gen].cpu().numpy(),
                   gen_copy=self.gen_copy[:n_gen].cpu().numpy())
        return out


class FeatureSetAccumulator(RecordTable):
    """A table of the features of ``num_clips`` clips on ``device`` (``dim`` = mu ++ logvar columns, ``copies`` = TEST.MULTIPLE predictions per
    clip) and the metrics between its real and its generated rows with ``k`` neighbours.

    ``add`` enqueues one launch on the current stream: no host synchronisation, no allocation (inputs that are not contiguous are made so,
    which allocates).  ``result`` allocates the workspace on its first call and is the only call that waits for the device; it cannot run
    inside a hipGraph capture.  The state is one (num_clips + 1, cols) int64 tensor (``RecordTable`` owns it, ``state``, ``table``, ``reset``)."""

    NOUN, NO_GPU = 'the feature-set metrics', _NO_GPU

    def __init__(self, num_clips, dim, copies=1, k=5, device='cuda'):
        import torch
        from . import _lib
        num_clips, dim, copies = check_num_clips(num_clips), int(dim), int(copies)
        if not 2 <= dim <= MAX_DIM or dim % 2:
            raise ValueError('the feature width %d must be even (mu ++ logvar) and lie in [2, %d]' % (dim, MAX_DIM))
        if not 1 <= copies <= MAX_COPIES:
            raise ValueError('%d copies outside [1, %d]' % (copies, MAX_COPIES))
        if num_clips * copies > MAX_ROWS:
            raise ValueError('%d clips x %d copies: a set holds at most %d rows' % (num_clips, copies, MAX_ROWS))
        self.dim, self.copies, self.k = dim, copies, check_k(k)
        RecordTable.__init__(self, num_clips, device, cols(dim, copies), 0, 2 * OUT_WORDS)
        self._lib = _lib.load()
        if self._lib.sdt_prdc_cols(dim, copies) != self._state.shape[1]:
            raise RuntimeError('the library lays a record out in %d words, this binding in %d'
                               % (self._lib.sdt_prdc_cols(dim, copies), self._state.shape[1]))
        self._torch, self._sets, self._work, self._last = torch, None, None, None

    def _features(self, x, rows=None):
        torch = self._torch
        if not torch.is_tensor(x) or x.device != self.device:
            raise RuntimeError('%s take tensors on %s; %s' % (self.NOUN, self.device, self.NO_GPU))
        if x.dtype != torch.float32 or x.ndim != 2 or x.shape[1] != self.dim // 2 or x.shape[0] < 1 or (rows is not None and x.shape[0] != rows):
            raise TypeError('features must be (%s, %d) float32, got %s %s' % ('rows' if rows is None else rows, self.dim // 2, tuple(x.shape), x.dtype))
        return x.detach().contiguous()

    def add(self, mu_pred, logvar_pred, mu_gt, logvar_gt, clip_index):
        """one validation step: four (copies * B, dim / 2) float32 tensors, copy j of clip b in row j * B + b (the ground truth of copy 0 is the
        one kept); ``clip_index``: the B table rows (an int64 tensor of B entries, or of copies * B: the first B are read)"""
        from . import _lib
        torch, m = self._torch, self.copies
        mu_pred = self._features(mu_pred)
        R = mu_pred.shape[0]
        if R % m:
            raise ValueError('%d rows are not %d copies of one batch' % (R, m))
        logvar_pred, mu_gt, logvar_gt = (self._features(x, R) for x in (logvar_pred, mu_gt, logvar_gt))
        B = R // m
        if not torch.is_tensor(clip_index) or clip_index.dtype != torch.int64 or clip_index.ndim != 1 or clip_index.numel() not in (B, R):
            raise TypeError('clip_index must be an int64 tensor of %d (or %d) entries' % (B, R))
        idx = clip_index[:B].to(self.device, non_blocking=True).contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sdt_prdc_commit(self._p(mu_pred), self._p(logvar_pred), self._p(mu_gt), self._p(logvar_gt), self._p(idx), B, m,
                                                 self.dim // 2, self._p(self._state), self.num_clips, self._stream()))

    def result_words(self, gathered=None, dim_used=None):
        """the 32 words of a result as a numpy int64 array (float64 words viewed as int64): sdt_prdc_reduce's 16 of the usual pass, then the
        16 of the floor pass"""
        from . import _lib
        _refuse_capture()
        torch = self._torch
        dim_used = self.dim if dim_used is None else int(dim_used)
        if not 1 <= dim_used <= self.dim:
            raise ValueError('dim_used %d outside [1, %d]' % (dim_used, self.dim))
        ptrs, ranks, _keep = self.table_pointers(gathered)
        N, m = self.num_clips, self.copies
        with torch.cuda.device(self.device):
            if self._sets is None:
                self._sets = _Sets(N, N * m, self.dim, self.device)
                self._work = torch.empty(2 * N, dtype=torch.int64, device=self.device)
            st, stream = self._sets, self._stream()
            for floor in (1, 0):  # (the usual pass last: its per-row outputs are the ones ``rows`` reads)
                _lib.check(self._lib.sdt_prdc_gather(ptrs, ranks, N, self.dim, m, dim_used, floor, self._p(self._work), self._p(st.real),
                                                     self._p(st.gen), self._p(st.real_clip), self._p(st.gen_clip), self._p(st.gen_copy),
                                                     self._p(st.counts), stream))
                st.run(dim_used, self.k, self._out[OUT_WORDS * floor:OUT_WORDS * (floor + 1)], stream)
            words = self._out.cpu().numpy()  # (same stream: ordered after the kernels, and the one wait of an accumulator)
        self._last = (int(words[OUT_ROWS_REAL]), int(words[OUT_ROWS_GEN]))
        return words

    def result(self, dim_used=None, gathered=None):
        """-> the named values (``result_values``) over this accumulator's table, or over ``gathered``: a (ranks, num_clips + 1, cols) int64
        tensor (or a list of such states / accumulators), one entry per rank.  ``dim_used``: the leading columns of every feature row taken
        (dim / 2: mu alone; default: all).  Too few rows: NaN values, a bit in 'err' and a logged warning."""
        res = result_values(self.result_words(gathered, dim_used), self.dim if dim_used is None else int(dim_used))
        for sfx in ('', '_floor'):
            if res['err' + sfx]:
                logging.warning('feature-set metrics%s: %s' % (sfx, describe_error(res, sfx)))
        return res

    def rows(self):
        """the per-row outputs of the last ``result`` (GEN_ROWS, REAL_ROWS) as numpy arrays, with 'real_clip', 'gen_clip' and 'gen_copy': the
        clip index (and the copy) behind every row; 'gen_nearest' is a position in the real set (real_clip[gen_nearest] is its clip)"""
        if self._last is None:
            raise RuntimeError('rows() gives the per-row outputs of the last result(); there has been none')
        return self._sets.host_rows(*self._last)

    def epoch_values(self, words):
        return result_values(words)


def prdc_device(real, gen, k=5, device='cuda'):
    """the metrics between two plain (n, D) arrays (float32 values; D 1 .. 64; non-finite values are refused) on the GPU ->
    ``prdc_model``'s dictionary, the same bits, plus 'words' (the 16 words of the epoch vector)"""
    import torch
    from . import _lib
    k = check_k(k)
    real, gen = _check_sets(real, gen)
    if real.shape[0] < 1 or gen.shape[0] < 1:
        raise ValueError('the device route takes at least one row per set, got %d and %d' % (real.shape[0], gen.shape[0]))
    device = _record_table.cuda_device(device, _NO_GPU)
    _refuse_capture()
    _lib.load()
    nr, ng, D = real.shape[0], gen.shape[0], real.shape[1]
    with torch.cuda.device(device):
        st = _Sets(nr, ng, D, device)
        st.real.copy_(torch.from_numpy(real.reshape(-1)))
        st.gen.copy_(torch.from_numpy(gen.reshape(-1)))
        st.counts.copy_(torch.tensor([nr, ng, 0, 0, 0, 0, 0, 0], dtype=torch.int64))
        out = torch.empty(OUT_WORDS, dtype=torch.int64, device=device)
        st.run(D, k, out, _record_table.stream(device))
        words = out.cpu().numpy()
        rows = st.host_rows(nr, ng)
    f = words.view(np.float64)
    res = {v: f[i] for i, v in enumerate(VALUES)}
    res.update({'num_' + v: int(words[4 + i]) for i, v in enumerate(VALUES)})
    res.update(rows_real=int(words[OUT_ROWS_REAL]), rows_gen=int(words[OUT_ROWS_GEN]), k=int(words[OUT_K]), err=int(words[OUT_ERR]), words=words)
    res.update({key: rows[key] for key in GEN_ROWS + REAL_ROWS})
    return res


def save_rows(path, rows, res, k):
    """the per-row outputs with their clip indices, k and the counts of ``res``"""
    scalars = {key: np.asarray(v) for key, v in res.items() if key not in rows and isinstance(v, (int, float, np.integer, np.floating))}
    scalars['k'] = np.int64(k)
    np.savez(path, **{key: np.asarray(v) for key, v in rows.items()}, **scalars)


# ---- command line ------------------------------------------------------------------------------------------------------------------------------
def _load_features(path, side, mu_only):
    if path.endswith('.npz'):
        with np.load(path) as z:
            keys = ['mu_' + side] + ([] if mu_only else ['logvar_' + side])
            for key in keys:
                if key not in z.files:
                    raise KeyError('%s has no entry %r (it has %s)' % (path, key, ', '.join(z.files)))
            x = np.concatenate([z[key].reshape(-1, z[key].shape[-1]) for key in keys], axis=1)
    else:
        x = np.load(path)
        x = x.reshape(-1, x.shape[-1])
        if mu_only:
            if x.shape[1] % 2:
                raise ValueError('--mu-only takes the leading half of the columns, %s has %d' % (path, x.shape[1]))
            x = x[:, :x.shape[1] // 2]
    return x


def report(res, worst, emit=print):
    """prints the four values, the counts, and the ``worst`` rows of either kind; -> the lines' row numbers (generated, real)"""
    for v in VALUES:
        emit('%s: %r' % (v, float(res[v])))
    for key in ['num_' + v for v in VALUES] + ['rows_real', 'rows_gen', 'k', 'err']:
        emit('%s: %d' % (key, res[key]))
    problem = describe_error(res)
    if problem:
        emit('error: ' + problem)
    outside = np.flatnonzero(np.asarray(res['gen_ball_count']) == 0)
    far = outside[np.argsort(-np.asarray(res['gen_nearest_d2'])[outside], kind='stable')[:worst]]
    for j in far:
        emit('outside: generated row %d, nearest real row %d at d2 %r' % (j, res['gen_nearest'][j], float(res['gen_nearest_d2'][j])))
    lonely = np.flatnonzero(np.asarray(res['real_covered']) == 0)[:worst]
    for i in lonely:
        emit('uncovered: real row %d, radius %r' % (i, float(res['real_radius'][i])))
    return [int(j) for j in far], [int(i) for i in lonely]


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='precision / recall / density / coverage of a generated feature set against a real one, on the GPU')
    ap.add_argument('a', help='the real set: .npy of (n, d) features, or a results/*.npz of TEST.SAVE_NPZ (mu_gt, logvar_gt)')
    ap.add_argument('b', help='the generated set (may be the same .npz: mu_pred, logvar_pred)')
    ap.add_argument('--k', type=int, default=5, help='neighbours of a radius, 1 .. %d (5: the density / coverage paper; untuned)' % MAX_NEIGHBOURS)
    ap.add_argument('--mu-only', action='store_true', help='the mu columns alone (the leading half of a .npy)')
    ap.add_argument('--worst', type=int, default=5, metavar='N', help='list the N generated rows farthest outside and N uncovered real rows')
    ap.add_argument('--out', default=None, metavar='rows.npz', help='write the per-row outputs')
    ap.add_argument('--host', action='store_true', help='compute with the numpy model on the host (small sets)')
    a = ap.parse_args(argv)
    if not 1 <= a.k <= MAX_NEIGHBOURS:
        ap.error('--k outside [1, %d]' % MAX_NEIGHBOURS)
    if a.worst < 0:
        ap.error('--worst must be >= 0')
    real, gen = _load_features(a.a, 'gt', a.mu_only), _load_features(a.b, 'pred', a.mu_only)
    if a.host:
        res = prdc_model(real, gen, a.k)
    else:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_GPU)
        res = prdc_device(real, gen, a.k)
    report(res, a.worst)
    if a.out:
        save_rows(a.out, {key: res[key] for key in GEN_ROWS + REAL_ROWS}, res, a.k)
    return 1 if res['err'] else 0


if __name__ == '__main__':
    raise SystemExit(main())
