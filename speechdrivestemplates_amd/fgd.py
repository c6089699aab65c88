"""Frechet gesture distance between two sets of pose-encoder codes (reference: core/utils/fgd.py:6-64).

    FGD(A, B) = |mean_A - mean_B|^2 + tr(C_A) + tr(C_B) - 2 tr((C_A C_B)^(1/2))

Two routes.  ``compute_fgd`` is the reference's: host, float64, scipy's ``sqrtm``, over features that every validation step copied to the
host.  ``FGDAccumulator`` / ``compute_fgd_device`` (csrc/fgd.hip, SYS.DEVICE_FGD) keep the features on the GPU:
every step adds its rows to a fixed-size float64 state of shifted moments, and one wave turns the states -- one per rank under data
parallelism, merged in rank order -- into the distance through two symmetric eigen-decompositions (tr (C_A C_B)^(1/2) = the sum of the
square roots of the eigenvalues of C_A^(1/2) C_B C_A^(1/2)).  Nothing is copied to the host before ``result()``.

    python -m speechdrivestemplates_amd.fgd A B [--keys mu_pred mu_gt]     (.npy files, or the results/*.npz files of TEST.SAVE_NPZ)
"""
import numpy as np
from scipy import linalg


def _trace_sqrt_product(c_a, c_b, jitter=1e-6):
    root, _ = linalg.sqrtm(c_a @ c_b, disp=False)
    if not np.all(np.isfinite(root)):  # singular product: nudge both covariances off the boundary and retry
        eye = jitter * np.eye(c_a.shape[0])
        root = linalg.sqrtm((c_a + eye) @ (c_b + eye))
    return float(np.trace(np.real(root)))  # round-off can leave a tiny imaginary part; the reference drops it


def compute_fgd(feat_a, feat_b):
    """feat_* : (n_samples, dim) arrays of codes (mu, or mu ++ logvar)."""
    feat_a, feat_b = np.asarray(feat_a, dtype=np.float64), np.asarray(feat_b, dtype=np.float64)
    if feat_a.shape[1] != feat_b.shape[1]:
        raise ValueError('feature dimensions differ: %d vs %d' % (feat_a.shape[1], feat_b.shape[1]))
    gap = feat_a.mean(axis=0) - feat_b.mean(axis=0)
    c_a = np.atleast_2d(np.cov(feat_a, rowvar=False))
    c_b = np.atleast_2d(np.cov(feat_b, rowvar=False))
    return float(gap @ gap + np.trace(c_a) + np.trace(c_b) - 2.0 * _trace_sqrt_product(c_a, c_b))


# ---- the device route (csrc/fgd.hip) ------------------------------------------------------------------------------------------------------------
MAX_DIM = 64
MAX_SWEEPS = 30  # cyclic Jacobi converges quadratically: a 64 x 64 covariance takes about ten sweeps
REL_TOL = 1e-15  # stop at off(A) <= REL_TOL * ||A||_F
MAX_STATES = 64  # states per side of one finalize: one per rank
ERR_NOT_CONVERGED, ERR_TOO_FEW_ROWS, ERR_NON_FINITE = 1, 2, 4  # bits of result()['err']
OUT_FIELDS = ('fgd', 'mean_gap_sq', 'trace_a', 'trace_b', 'trace_sqrt', 'rows_a', 'rows_b', 'sweeps_a', 'offdiag_a', 'sweeps_m', 'offdiag_m',
              'min_eig_a', 'min_eig_m', 'first_bad_row_a', 'first_bad_row_b')  # the words of sdt_fgd_finalize's ``out`` (include/sdt_hip.h)
_INT_FIELDS = ('rows_a', 'rows_b', 'sweeps_a', 'sweeps_m', 'first_bad_row_a', 'first_bad_row_b')
SIDES = ('pred', 'gt')  # side a, side b of the pipeline's accumulator


class FGDAccumulator:
    """Running moments of two sets of ``dim``-wide fp32 feature rows on ``device`` and their Frechet distance.

    ``add`` enqueues one kernel per side on the current stream: no host synchronisation, no allocation (inputs that are not contiguous are
    made so, which allocates), capturable in a hipGraph (a replay records non-finite rows under the row numbers of the capture).
    ``result`` is the only call that waits for the device."""

    def __init__(self, dim, device='cuda'):
        import ctypes as C
        import torch
        from . import _lib
        dim = int(dim)
        if not 2 <= dim <= MAX_DIM:
            raise ValueError('feature dimension %d outside [2, %d]' % (dim, MAX_DIM))
        self.dim, self.device = dim, torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('the device FGD is computed on the GPU (csrc/fgd.hip); there is no CPU fallback (compute_fgd is the host route)')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self._lib, self._C, self._torch = _lib.load(), C, torch
        self.state_bytes = int(self._lib.sdt_fgd_state_bytes(dim))
        self._states = torch.zeros((2, self.state_bytes // 8), dtype=torch.int64, device=self.device)  # the kernels expect zeroed states
        self._out = torch.empty(16, dtype=torch.float64, device=self.device)
        self._err = torch.empty(1, dtype=torch.int32, device=self.device)
        self._rows = [0, 0]  # rows handed to each side so far: the host's count, the base of the next call's row numbers

    def _stream(self):
        return self._torch.cuda.current_stream(self.device).cuda_stream

    def _features(self, x0, x1):
        torch = self._torch
        for x in (x0, x1):
            if x is None:
                continue
            if not torch.is_tensor(x) or x.device != self.device:
                raise RuntimeError('the device FGD takes tensors on %s (csrc/fgd.hip); there is no CPU fallback' % (self.device,))
            if x.dtype != torch.float32 or x.ndim != 2:
                raise TypeError('features must be (rows, d) float32, got %s %s' % (tuple(x.shape), x.dtype))
        d1 = 0 if x1 is None else x1.shape[1]
        if x0.shape[1] + d1 != self.dim or (x1 is not None and x1.shape[0] != x0.shape[0]) or x0.shape[0] < 1 or x0.shape[1] < 1:
            raise ValueError('features %s%s do not make rows of %d values' % (tuple(x0.shape), '' if x1 is None else ' ++ %s' % (tuple(x1.shape),),
                                                                            self.dim))
        return x0.detach().contiguous(), None if x1 is None or d1 == 0 else x1.detach().contiguous()

    def add_side(self, side, x0, x1=None):
        """rows of ``x0`` (++ the rows of ``x1``) -> side 0 / 1"""
        from . import _lib
        x0, x1 = self._features(x0, x1)
        n = x0.shape[0]
        with self._torch.cuda.device(self.device):
            _lib.check(self._lib.sdt_fgd_accumulate(self._C.c_void_p(x0.data_ptr()), x0.shape[1],
                                                    None if x1 is None else self._C.c_void_p(x1.data_ptr()), 0 if x1 is None else x1.shape[1], n,
                                                    self._C.c_void_p(self._states[side].data_ptr()), self.state_bytes, self._rows[side],
                                                    self._stream()))
        self._rows[side] += n

    def add(self, pred0, gt0, pred1=None, gt1=None):
        """one validation step: ``pred0`` (++ ``pred1``) to the predicted side, ``gt0`` (++ ``gt1``) to the ground-truth side"""
        if (pred1 is None) != (gt1 is None):
            raise ValueError('pred1 and gt1 come together')
        self.add_side(0, pred0, pred1)
        self.add_side(1, gt0, gt1)

    def state_tensors(self):
        """the two fixed-size states, (state_bytes / 8,) int64 views of one (2, words) tensor (``states()``: that tensor, for a collective)"""
        return self._states[0], self._states[1]

    def states(self):
        return self._states

    def reset(self):
        self._states.zero_()
        self._rows = [0, 0]

    def result(self, dim_used=None, gathered=None, strict=True, max_sweeps=MAX_SWEEPS):
        """-> {OUT_FIELDS..., 'err', 'dim_used'} over this accumulator's states, or over ``gathered``: a (ranks, 2, words) int64 tensor (or a list
        of (2, words) tensors / accumulators), one entry per rank, merged in that order.  ``dim_used``: the leading sub-block (default: all).
        strict: FloatingPointError for a recorded non-finite row (names side and row), ValueError for fewer than 2 rows on a side,
        RuntimeError when a decomposition has not converged; strict=False returns the error bits in 'err' (FGD is NaN for the first two)."""
        from . import _lib
        torch, C = self._torch, self._C
        dim_used = self.dim if dim_used is None else int(dim_used)
        if not 2 <= dim_used <= self.dim:
            raise ValueError('dim_used %d outside [2, %d]' % (dim_used, self.dim))
        if gathered is None:
            blocks = [self._states]
        elif torch.is_tensor(gathered):
            blocks = list(gathered.unbind(0)) if gathered.ndim == 3 else [gathered]
        else:
            blocks = [g.states() if isinstance(g, FGDAccumulator) else g for g in gathered]
        if not 1 <= len(blocks) <= MAX_STATES:
            raise ValueError('%d states per side; finalize takes 1 to %d' % (len(blocks), MAX_STATES))
        for b in blocks:
            if b.dtype != torch.int64 or tuple(b.shape) != tuple(self._states.shape) or b.device != self.device or not b.is_contiguous():
                raise ValueError('a gathered state must be a contiguous %s int64 tensor on %s' % (tuple(self._states.shape), self.device))
        ptrs = C.c_void_p * len(blocks)
        a, b = ptrs(*[t[0].data_ptr() for t in blocks]), ptrs(*[t[1].data_ptr() for t in blocks])
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sdt_fgd_finalize(a, b, len(blocks), self.dim, dim_used, int(max_sweeps), REL_TOL,
                                                  C.c_void_p(self._out.data_ptr()), C.c_void_p(self._err.data_ptr()), self._stream()))
            vals = self._out.cpu().tolist()  # (same stream: ordered after the kernel, and the one wait of this class)
            err = int(self._err.item())
        res = {k: (int(v) if k in _INT_FIELDS else v) for k, v in zip(OUT_FIELDS, vals)}
        res.update(err=err, dim_used=dim_used)
        if strict:
            problem = describe_error(res)
            if err & ERR_NON_FINITE:
                raise FloatingPointError(problem)
            if err & ERR_TOO_FEW_ROWS:
                raise ValueError(problem)
            if err & ERR_NOT_CONVERGED:
                raise RuntimeError(problem)
        return res


def describe_error(res):
    """what the error bits of a ``result()`` dict say, '' if none is set"""
    msgs = []
    if res['err'] & ERR_NON_FINITE:
        msgs.append('non-finite feature: ' + ', '.join('side %s first at row %d' % (SIDES[i], res['first_bad_row_' + 'ab'[i]])
                                                       for i in range(2) if res['first_bad_row_' + 'ab'[i]] >= 0))
    if res['err'] & ERR_TOO_FEW_ROWS:
        msgs.append('a covariance needs at least 2 rows per side, got %d (%s) and %d (%s)' % (res['rows_a'], SIDES[0], res['rows_b'], SIDES[1]))
    if res['err'] & ERR_NOT_CONVERGED:
        msgs.append('Jacobi did not converge: off-diagonal norms %.3e after %d sweeps and %.3e after %d sweeps'
                    % (res['offdiag_a'], res['sweeps_a'], res['offdiag_m'], res['sweeps_m']))
    return '; '.join(msgs)


def _device_features(x, device):
    import torch
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
    if x.ndim != 2:
        raise ValueError('features must be (n_samples, dim), got %s' % (tuple(x.shape),))
    return x.to(device=device, dtype=torch.float32)


def fgd_device_result(feat_a, feat_b, device='cuda', strict=True):
    """``result()`` of a fresh accumulator fed the two (n, d) sets (arrays or tensors; values are taken as float32)"""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError('the device FGD is computed on the GPU (csrc/fgd.hip); there is no CPU fallback (compute_fgd is the host route)')
    a, b = _device_features(feat_a, device), _device_features(feat_b, device)
    if a.shape[1] != b.shape[1]:
        raise ValueError('feature dimensions differ: %d vs %d' % (a.shape[1], b.shape[1]))
    acc = FGDAccumulator(a.shape[1], a.device)
    acc.add_side(0, a)
    acc.add_side(1, b)
    return acc.result(strict=strict)


def compute_fgd_device(feat_a, feat_b):
    """``compute_fgd`` on the GPU: two (n_samples, dim) arrays or tensors (float32 values) -> float"""
    return fgd_device_result(feat_a, feat_b)['fgd']


def _load_features(path, key):
    if path.endswith('.npz'):
        with np.load(path) as z:
            if key not in z.files:
                raise KeyError('%s has no entry %r (it has %s)' % (path, key, ', '.join(z.files)))
            x = z[key]
    else:
        x = np.load(path)
    return x.reshape(-1, x.shape[-1])


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='Frechet gesture distance of two feature sets, computed on the GPU')
    ap.add_argument('a', help='.npy of (n, d) features, or a results/*.npz of TEST.SAVE_NPZ')
    ap.add_argument('b', help='the other set (may be the same .npz)')
    ap.add_argument('--keys', nargs=2, default=('mu_pred', 'mu_gt'), metavar=('KEY_A', 'KEY_B'), help='entries read from .npz inputs')
    a = ap.parse_args(argv)
    res = fgd_device_result(_load_features(a.a, a.keys[0]), _load_features(a.b, a.keys[1]), strict=False)
    for k in OUT_FIELDS + ('err',):
        print('%s: %s' % (k, ('%d' % res[k]) if k in _INT_FIELDS or k == 'err' else repr(float(res[k]))))
    problem = describe_error(res)
    if problem:
        print('error: ' + problem)
    return 1 if res['err'] else 0


if __name__ == '__main__':
    raise SystemExit(main())
