"""Principal template axes and nearest template codes, on the GPU (csrc/code_axes.hip).

The reference's two demo modes ask the user for template codes and give no way to find them: ``Pose2PoseModel.forward(return_loss=False)``
(pose2pose.py:50-56) decodes ``np.load(DEMO.CODE_PATH)['v'][idx] * 10`` for idx = 0 .. DEMO.MULTIPLE-1, and ``Voice2PoseModel`` takes rows
DEMO.CODE_INDEX / DEMO.CODE_INDEX_B of the learned table.  This tool decomposes the code table along all of its principal axes, measures
the populated range of every axis by exact order statistics, walks each axis between two quantiles and finds the table row nearest to
every point of the walk.  Its npz is what both demos consume: ``v`` holds the axes, ``code_index`` the rows.

    python -m speechdrivestemplates_amd.code_axes --checkpoint X.pth --out axes.npz [--axes 4] [--steps 7] [--lo 0.01 --hi 0.99] [--table KEY]
    python -m speechdrivestemplates_amd.code_axes --codes table.npy --out axes.npz

Everything is float64 on values converted exactly from the fp32 table, every operation rounded on its own; the ``model_*`` functions
restate the kernels in numpy with the same operation order.
"""
import argparse
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from .code_pca import MAX_DIM, MAX_SWEEPS, REL_TOL, _as_table, _eigh_decode, _eigh_launch, _moments, load_code_table

MAX_QUERIES = 65536
MAX_RANKS = 16
FILE_QUANTILES = (0.0, 0.01, 0.5, 0.99, 1.0)
NO_GPU = 'the template axes are computed on the GPU (csrc/code_axes.hip); there is no CPU fallback'


def _p(t):
    return C.c_void_p(t.data_ptr())


def _check(status):
    """as ``_lib.check``; the library's "unsupported size" status becomes a ValueError"""
    if status == -3:  # SDT_ERR_UNSUPPORTED
        raise ValueError('libsdt_hip: %s' % _lib.load().sdt_last_error().decode())
    _lib.check(status)


def fit_axes(codes, max_sweeps=MAX_SWEEPS):
    """All principal axes of the (N, D) / (N, F, D) fp32 device table ``codes`` and its projection on them.
    -> {'mean' (D,), 'components' (D, D), 'explained_variance' (D,), 'explained_variance_ratio' (D,), 'projections' (N, D),
    'covariance' (D, D): float64 device tensors; 'sweeps', 'offdiag', 'n_rows', 'dim'}.  Rows 0 and 1 of everything carry the bits of
    ``code_pca.fit_project``."""
    x = _as_table(codes)
    n, d = x.shape
    lib = _lib.load()
    dev = x.device
    with torch.cuda.device(dev):
        raw = torch.cuda.current_stream(dev).cuda_stream
        mean, cov = _moments(lib, x, raw)
        evals, comps, info, err = _eigh_launch(lib, 'axes', cov, d, max_sweeps, raw, check=_check)
        sweeps, offdiag, _, trace = _eigh_decode(max_sweeps, info, err)
        proj = torch.empty((n, d), dtype=torch.float64, device=dev)
        _check(lib.sdt_code_axes_project(_p(x), n, d, _p(mean), _p(comps), _p(proj), raw))
        ratio = torch.from_numpy(evals.cpu().numpy() / trace).to(dev)
    return {'mean': mean, 'components': comps, 'explained_variance': evals, 'explained_variance_ratio': ratio, 'projections': proj,
            'covariance': cov, 'sweeps': sweeps, 'offdiag': offdiag, 'n_rows': n, 'dim': d}


def quantile_ranks(q, n):
    """rank int(floor(q (N - 1))) of every q in [0, 1], in Python floats: ``np.quantile(..., method='lower')``"""
    ranks = []
    for v in np.atleast_1d(np.asarray(q, dtype=np.float64)).tolist():
        if not 0.0 <= v <= 1.0:
            raise ValueError('a quantile must lie in [0, 1], got %r' % (v,))
        ranks.append(int(math.floor(v * (n - 1))))
    return ranks


def _projection_table(projections):
    if not torch.is_tensor(projections) or not projections.is_cuda:
        raise RuntimeError(NO_GPU)
    if projections.dtype != torch.float64 or projections.ndim != 2:
        raise ValueError('projections must be (N, D) float64, got %s %s' % (tuple(projections.shape), projections.dtype))
    n, d = projections.shape
    if n < 2 or not 2 <= d <= MAX_DIM:
        raise ValueError('projections of shape (%d, %d): N must be at least 2 and D in [2, %d]' % (n, d, MAX_DIM))
    return projections.contiguous()


def order_statistics(projections, ranks):
    """(D, R) float64 device tensor: entry (k, r) = the element of column k that an ascending sort puts at position ranks[r]"""
    P = _projection_table(projections)
    n, d = P.shape
    ranks = [int(r) for r in ranks]
    if not 1 <= len(ranks) <= MAX_RANKS:
        raise ValueError('between 1 and %d ranks per call, got %d' % (MAX_RANKS, len(ranks)))
    if any(r < 0 or r >= n for r in ranks):
        raise ValueError('ranks must lie in [0, %d), got %r' % (n, ranks))
    lib = _lib.load()
    dev = P.device
    with torch.cuda.device(dev):
        raw = torch.cuda.current_stream(dev).cuda_stream
        ws_bytes = lib.sdt_code_axes_quantiles_workspace_bytes(n, d, len(ranks))
        if ws_bytes <= 0:
            raise ValueError('unsupported sizes: (%d, %d) with %d ranks' % (n, d, len(ranks)))
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
        ranks_d = torch.tensor(ranks, dtype=torch.int64, device=dev)
        out = torch.empty((d, len(ranks)), dtype=torch.float64, device=dev)
        _check(lib.sdt_code_axes_quantiles(_p(P), n, d, _p(ranks_d), len(ranks), _p(out), _p(ws), ws_bytes, raw))
    return out


def axis_quantiles(projections, q):
    """(D, len(q)) float64 device tensor: ``np.quantile(projections[:, k], q, method='lower')`` of every axis, exactly"""
    return order_statistics(projections, quantile_ranks(q, projections.shape[0]))


def traversal(fit, axes, steps, lo_q=0.01, hi_q=0.99):
    """``steps`` evenly spaced points on each chosen axis between its ``lo_q`` and ``hi_q`` order statistics.  ``axes``: a count (the
    leading ones) or a list of axis numbers.  -> {'axes' (A,) int64 numpy, 't' (A, M), 'points' (A, M, D) = mean + t components[k]:
    float64 device tensors}.  The A * M offsets are spaced on the host (np.linspace, float64)."""
    d = fit['dim']
    axes = list(range(int(axes))) if isinstance(axes, (int, np.integer)) else [int(a) for a in axes]
    if not axes or any(a < 0 or a >= d for a in axes):
        raise ValueError('axes must be numbers in [0, %d), got %r' % (d, axes))
    steps = int(steps)
    if steps < 1:
        raise ValueError('steps must be at least 1, got %d' % steps)
    if not 0.0 <= lo_q <= hi_q <= 1.0:
        raise ValueError('need 0 <= lo_q <= hi_q <= 1, got %r, %r' % (lo_q, hi_q))
    ends = axis_quantiles(fit['projections'], [lo_q, hi_q]).cpu().numpy()
    t = np.stack([np.linspace(ends[a, 0], ends[a, 1], steps) for a in axes])  # (A, M)
    mean, comps = fit['mean'].cpu().numpy(), fit['components'].cpu().numpy()
    points = mean[None, None, :] + t[:, :, None] * comps[axes][:, None, :]
    dev = fit['projections'].device
    return {'axes': np.asarray(axes, np.int64), 't': torch.from_numpy(t).to(dev), 'points': torch.from_numpy(points).to(dev)}


def nearest_codes(codes, queries):
    """the table row nearest to every query: ``queries`` (..., D) float64 device tensor -> (index (...) int64, dist2 (...) float64), device
    tensors; of equally near rows the lowest.  A non-finite table row or query raises, naming it."""
    x = _as_table(codes)
    n, d = x.shape
    if not torch.is_tensor(queries) or not queries.is_cuda:
        raise RuntimeError(NO_GPU)
    if queries.dtype != torch.float64 or queries.ndim < 1 or queries.shape[-1] != d:
        raise ValueError('queries must be (..., %d) float64, got %s %s' % (d, tuple(queries.shape), queries.dtype))
    shape = tuple(queries.shape[:-1])
    qs = queries.reshape(-1, d).contiguous()
    nq = qs.shape[0]
    if not 1 <= nq <= MAX_QUERIES:
        raise ValueError('between 1 and %d queries per call, got %d' % (MAX_QUERIES, nq))
    lib = _lib.load()
    dev = x.device
    with torch.cuda.device(dev):
        raw = torch.cuda.current_stream(dev).cuda_stream
        _moments(lib, x, raw)  # the bad-row word: a non-finite row is reported before the search runs
        ws_bytes = lib.sdt_code_axes_nearest_workspace_bytes(n, d, nq)
        if ws_bytes <= 0:
            raise ValueError('unsupported sizes: (%d, %d) with %d queries' % (n, d, nq))
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
        index = torch.empty(nq, dtype=torch.int64, device=dev)
        dist2 = torch.empty(nq, dtype=torch.float64, device=dev)
        bad = torch.empty(1, dtype=torch.int64, device=dev)
        _check(lib.sdt_code_axes_nearest(_p(x), n, d, _p(qs), nq, _p(index), _p(dist2), _p(bad), _p(ws), ws_bytes, raw))
        first = int(bad.item())
    if first >= 0:
        raise ValueError('query %d has a non-finite entry' % first)
    return index.reshape(shape), dist2.reshape(shape)


# -- the contract in numpy: the kernels' arithmetic in the kernels' order ----------------------------------------------------------
def _ordered_norm(A, skip_diagonal):
    """sqrt of the sum of squares, column by column (rows ascending), then over the columns ascending: csrc/jacobi.h"""
    sq = A * A
    if skip_diagonal:
        np.fill_diagonal(sq, 0.0)  # (adding +0.0 changes no partial sum)
    return math.sqrt(float(np.cumsum(np.cumsum(sq, axis=0)[-1])[-1]))


def model_components(cov, max_sweeps=MAX_SWEEPS, rel_tol=REL_TOL):
    """csrc/jacobi.h on the host: row-cyclic Jacobi of the (D, D) float64 ``cov`` with the kernel's rotations, sweep order, stopping rule
    and summation order, then the ranking (descending, ties to the lower column) and the sign rule (largest magnitude, first of equals,
    positive).  -> (eigenvalues (D,), components (D, D), sweeps, final off-diagonal norm); raises RuntimeError as ``fit_axes`` does."""
    A = np.array(cov, dtype=np.float64)
    D = A.shape[0]
    Vt = np.eye(D)
    frob = _ordered_norm(A, False)
    tol = rel_tol * frob
    sweeps = 0
    while True:
        off = _ordered_norm(A, True)
        if off <= tol:
            break
        if sweeps == max_sweeps:
            raise RuntimeError('Jacobi did not converge in %d sweeps: off-diagonal norm %.3e, ||C||_F %.3e' % (max_sweeps, off, frob))
        for p in range(D - 1):
            for q in range(p + 1, D):
                apq = float(A[p, q])
                if apq == 0.0:
                    continue
                app, aqq = float(A[p, p]), float(A[q, q])
                theta = (aqq - app) / (2.0 * apq)
                t = math.copysign(1.0, theta) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                rp, rq = A[p].copy(), A[q].copy()
                A[p] = A[:, p] = c * rp - s * rq
                A[q] = A[:, q] = s * rp + c * rq
                A[p, p], A[q, q] = app - t * apq, aqq + t * apq
                A[p, q] = A[q, p] = 0.0
                vp, vq = Vt[p].copy(), Vt[q].copy()
                Vt[p], Vt[q] = c * vp - s * vq, s * vp + c * vq
        sweeps += 1
    lam = np.diag(A).copy()
    order = sorted(range(D), key=lambda i: (-lam[i], i))
    comps = np.empty((D, D))
    for rank, i in enumerate(order):
        v = Vt[i]
        comps[rank] = -1.0 * v if v[int(np.argmax(np.abs(v)))] < 0 else 1.0 * v
    return lam[order], comps, sweeps, off


def model_project(table, mean, components):
    """P[n, k] = sum over d ascending of (x[n, d] - mean[d]) * components[k, d], every operation rounded on its own"""
    x = np.asarray(table)
    x = x.reshape(-1, x.shape[-1]).astype(np.float64)
    c = x - np.asarray(mean, np.float64)[None, :]
    comps = np.asarray(components, np.float64)
    P = np.zeros((x.shape[0], comps.shape[0]))
    for d in range(x.shape[1]):
        P = P + c[:, d:d + 1] * comps[None, :, d]
    return P


def model_quantiles(projections, ranks):
    """(D, R): entry (k, r) = sorted column k at position ranks[r]"""
    P = np.asarray(projections, np.float64)
    return np.sort(P, axis=0)[np.asarray(ranks, np.int64)].T.copy()


def model_nearest(table, queries):
    """(index, dist2) of the row with the least sum over d ascending of (q[d] - x[n, d])^2; of equals the first"""
    x = np.asarray(table)
    x = x.reshape(-1, x.shape[-1]).astype(np.float64)
    q = np.asarray(queries, np.float64).reshape(-1, x.shape[1])
    d2 = np.zeros((q.shape[0], x.shape[0]))
    for d in range(x.shape[1]):
        diff = q[:, d:d + 1] - x[None, :, d]
        d2 = d2 + diff * diff
    index = np.argmin(d2, axis=1)
    return index.astype(np.int64), d2[np.arange(q.shape[0]), index]


# -- the file ------------------------------------------------------------------------------------------------------------------------
def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def write_axes(path, fit, quantiles, trav, code_index, code_dist2):
    """one npz: v = components as float32 (D, D) (what ``np.load(DEMO.CODE_PATH)['v'][idx]`` indexes), mean, explained_variance,
    explained_variance_ratio, quantiles (D, 5) at FILE_QUANTILES, axes (A,), t (A, M), points (A, M, D), code_index (A, M) int64,
    code_dist2 (A, M)"""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, 'wb') as f:  # (np.savez would append '.npz' to a path without it; DEMO.CODE_PATH is opened as given)
        np.savez(f, v=_host(fit['components']).astype(np.float32), mean=_host(fit['mean']), explained_variance=_host(fit['explained_variance']),
                 explained_variance_ratio=_host(fit['explained_variance_ratio']), quantiles=_host(quantiles),
                 axes=np.asarray(trav['axes'], np.int64), t=_host(trav['t']), points=_host(trav['points']),
                 code_index=_host(code_index).astype(np.int64), code_dist2=_host(code_dist2))
    return path


def template_axes(codes, axes=4, steps=7, lo_q=0.01, hi_q=0.99):
    """fit, quantiles, traversal and nearest rows of a device table -> (fit, quantiles (D, 5), traversal, code_index, code_dist2)"""
    x = _as_table(codes)
    fit = fit_axes(x)
    quantiles = axis_quantiles(fit['projections'], FILE_QUANTILES)
    trav = traversal(fit, min(int(axes), fit['dim']), steps, lo_q, hi_q)
    index, dist2 = nearest_codes(x, trav['points'])
    return fit, quantiles, trav, index, dist2


def main(argv=None):
    ap = argparse.ArgumentParser(description='principal axes of a code table and the table rows along them, for the two demo modes')
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--checkpoint', help='a .pth of this engine or of the reference (same wire format)')
    src.add_argument('--codes', help='a bare (N, D) or (N, F, D) table as .npy (external codes)')
    ap.add_argument('--out', required=True, help='npz to write')
    ap.add_argument('--table', help='entry of model_state_dict; default: the first of module.clips_code, module.clip_code_mu that exists')
    ap.add_argument('--axes', type=int, default=4)
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--lo', type=float, default=0.01)
    ap.add_argument('--hi', type=float, default=0.99)
    a = ap.parse_args(argv)
    if a.codes:
        key, table = a.codes, torch.from_numpy(np.load(a.codes))
    else:
        key, table = load_code_table(a.checkpoint, a.table)
    if not torch.cuda.is_available():
        raise RuntimeError(NO_GPU)
    fit, quantiles, trav, index, dist2 = template_axes(table.float().cuda(), a.axes, a.steps, a.lo, a.hi)
    write_axes(a.out, fit, quantiles, trav, index, dist2)
    ratio, qs, idx, d2 = _host(fit['explained_variance_ratio']), _host(quantiles), _host(index), _host(dist2)
    print('%s %s (%d, %d): %d sweeps -> %s' % (a.checkpoint or a.codes, key, fit['n_rows'], fit['dim'], fit['sweeps'], a.out))
    for i, k in enumerate(trav['axes'].tolist()):
        print('axis %d: ratio %.6f quantiles(0, .01, .5, .99, 1)=(%s) rows %s' % (
            k, ratio[k], ', '.join('%.6g' % v for v in qs[k]), ' '.join('%d(%.4g)' % (n, v) for n, v in zip(idx[i], d2[i]))))
    print('DEMO.CODE_PATH %s' % a.out)
    print('DEMO.CODE_INDEX %d DEMO.CODE_INDEX_B %d' % (idx[0, 0], idx[0, -1]))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
