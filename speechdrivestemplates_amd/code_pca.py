"""The per-epoch clip-code figure, computed and drawn on the GPU (csrc/code_pca.hip): the reference's ``draw_figure_epoch``
(core/pipelines/voice2pose.py:479-510, pose2pose.py:314-345) fits ``sklearn.decomposition.PCA(n_components=2)`` to the clip-code
table on the host and scatter-plots the projection with matplotlib; here the table stays in HBM and neither library is needed.

Contract: float64 moments with ordered reductions, cyclic Jacobi on the D x D covariance, components signed
by their entry of largest magnitude (current scikit-learn's rule), projection, matplotlib's default 5 % axis margins, and a count
raster whose colours come from a host-built table (k markers of one colour composited over white do not depend on their order).
There is no text rendering: the explained-variance ratios and the axis limits go to the log line and into the PNG's text chunks.

    python -m speechdrivestemplates_amd.code_pca --checkpoint X.pth --out fig.png [--key module.clips_code] [--canvas 480x640]
"""
import argparse
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib

MAX_DIM = 64
MARGIN_PX = 12  # the plot rectangle is the canvas inset by this many pixels on every side (its black frame lies in the margin)
MAX_SWEEPS = 30  # cyclic Jacobi converges quadratically: a 64 x 64 covariance takes about ten sweeps
REL_TOL = 1e-15  # stop at off(A) <= REL_TOL * ||C||_F
DEFAULT_CANVAS = (480, 640)  # matplotlib's default figure (6.4 x 4.8 in at 100 dpi), as the reference draws it
DEFAULT_COLOUR = (31, 119, 180)  # matplotlib's first default colour, 'C0'
CODE_KEYS = ('module.clips_code', 'module.clip_code_mu')


def _p(t):
    return C.c_void_p(t.data_ptr())


def colour_table(alpha=0.2, colour=DEFAULT_COLOUR, max_len=1 << 16):
    """(L, 3) uint8: entry k = k markers of ``colour`` with opacity ``alpha`` composited over white,
    round_half_up(255 (1-a)^k + c (1 - (1-a)^k)) per channel in float64.  The last entry is the colour itself (the fixed point: no
    later k changes it), so counts past L - 1 are clamped to it."""
    a = float(alpha)
    if not 0.0 < a <= 1.0:
        raise ValueError('alpha must lie in (0, 1], got %r' % (alpha,))
    colour = tuple(int(c) for c in colour)
    if len(colour) != 3 or any(c < 0 or c > 255 for c in colour):
        raise ValueError('colour must be three integers in [0, 255], got %r' % (colour,))
    rows = []
    for k in range(max_len):
        q = (1.0 - a) ** k
        rows.append(tuple(int(math.floor(255.0 * q + c * (1.0 - q) + 0.5)) for c in colour))
        if rows[-1] == colour:
            return np.asarray(rows, np.uint8)
    raise ValueError('alpha=%r: the colour table has not reached %r after %d markers' % (alpha, colour, max_len))


def _as_table(codes):
    if not torch.is_tensor(codes) or not codes.is_cuda:
        raise RuntimeError('the clip-code figure is computed on the GPU (csrc/code_pca.hip); there is no CPU fallback')
    if codes.dtype != torch.float32:
        raise TypeError('the code table must be float32, got %s' % codes.dtype)
    if codes.ndim == 3:  # per-frame codes, as the reference reshapes them (voice2pose.py:496-497)
        codes = codes.reshape(-1, codes.shape[-1])
    if codes.ndim != 2:
        raise ValueError('the code table must be (N, D) or (N, F, D), got %s' % (tuple(codes.shape),))
    n, d = codes.shape
    if not 2 <= d <= MAX_DIM:
        raise ValueError('code dimension %d outside [2, %d]' % (d, MAX_DIM))
    if n < 2:
        raise ValueError('a PCA needs at least 2 rows, got %d' % n)
    return codes.detach().contiguous()


def _moments(lib, x, raw):
    """mean, covariance of the table by sdt_code_pca_moments; raises on a non-finite row BEFORE any other kernel sees the table"""
    n, d = x.shape
    ws_bytes = lib.sdt_code_pca_workspace_bytes(n, d)
    if ws_bytes <= 0:
        raise ValueError('unsupported table size (%d, %d)' % (n, d))
    f64 = dict(dtype=torch.float64, device=x.device)
    ws = torch.empty(ws_bytes // 8, **f64)
    mean, cov = torch.empty(d, **f64), torch.empty((d, d), **f64)
    bad = torch.empty(1, dtype=torch.int64, device=x.device)
    _lib.check(lib.sdt_code_pca_moments(_p(x), n, d, _p(ws), ws_bytes, _p(mean), _p(cov), _p(bad), raw))
    row = int(bad.item())
    if row:
        raise ValueError('the code table has a non-finite entry in row %d' % (row - 1))
    return mean, cov


def _eigh_launch(lib, which, cov, n_comps, max_sweeps, raw, check=_lib.check):
    """queues sdt_code_<which>_eigh ('pca' or 'axes') on the (D, D) device covariance -> (evals, comps, info, err), unread device tensors"""
    d = cov.shape[0]
    f64 = dict(dtype=torch.float64, device=cov.device)
    evals, comps, info = torch.empty(d, **f64), torch.empty((n_comps, d), **f64), torch.empty(4, **f64)
    err = torch.empty(1, dtype=torch.int32, device=cov.device)
    fn = getattr(lib, 'sdt_code_%s_eigh' % which)
    check(fn(_p(cov), d, int(max_sweeps), REL_TOL, _p(evals), _p(comps), _p(info), _p(err), raw))
    return evals, comps, info, err


def _eigh_decode(max_sweeps, info, err):
    """reads the error word and info of a queued ``_eigh_launch`` -> (sweeps, offdiag, frob, trace); raises what the word says"""
    word = int(err.item())
    sweeps, offdiag, frob, trace = info.cpu().tolist()
    if word & 1:
        raise RuntimeError('Jacobi did not converge in %d sweeps: off-diagonal norm %.3e, ||C||_F %.3e' % (max_sweeps, offdiag, frob))
    if word & 2:
        raise ValueError('the code table has no variance (trace of its covariance is %r): every row is the same' % trace)
    return int(sweeps), offdiag, frob, trace


def fit_project(codes, max_sweeps=MAX_SWEEPS):
    """2-component PCA of the (N, D) / (N, F, D) fp32 device table ``codes`` and its projection.
    -> {'mean' (D,), 'components' (2, D), 'explained_variance' (2,), 'explained_variance_ratio' (2,), 'eigenvalues' (D,): numpy
    float64; 'X' (N, 2) float64 device tensor; 'limits' (lo0, hi0, lo1, hi1) and 'minmax' (min0, max0, min1, max1): floats;
    'sweeps', 'offdiag' (final off-diagonal Frobenius norm), 'n_rows', 'dim'}"""
    x = _as_table(codes)
    n, d = x.shape
    lib = _lib.load()
    dev = x.device
    with torch.cuda.device(dev):
        raw = torch.cuda.current_stream(dev).cuda_stream
        mean, cov = _moments(lib, x, raw)
        evals, comps, info, err = _eigh_launch(lib, 'pca', cov, 2, max_sweeps, raw)
        f64 = dict(dtype=torch.float64, device=dev)
        ws_bytes = lib.sdt_code_pca_workspace_bytes(n, d)
        ws, X, limits = torch.empty(ws_bytes // 8, **f64), torch.empty((n, 2), **f64), torch.empty(8, **f64)
        _lib.check(lib.sdt_code_pca_project(_p(x), n, d, _p(mean), _p(comps), _p(X), _p(ws), ws_bytes, _p(limits), raw))  # queued before the error word is read
        sweeps, offdiag, frob, trace = _eigh_decode(max_sweeps, info, err)
    lam = evals.cpu().numpy()
    lim = limits.cpu().tolist()
    return {'mean': mean.cpu().numpy(), 'components': comps.cpu().numpy(), 'explained_variance': lam[:2].copy(),
            'explained_variance_ratio': lam[:2] / trace, 'eigenvalues': lam, 'X': X, 'limits': tuple(lim[4:]), 'minmax': tuple(lim[:4]),
            'sweeps': sweeps, 'offdiag': offdiag, 'n_rows': n, 'dim': d}


def plot_rectangle(canvas):
    """(Ph, Pw) of the plot rectangle of an (H, W) canvas"""
    h, w = (int(v) for v in canvas)
    if h - 2 * MARGIN_PX < 1 or w - 2 * MARGIN_PX < 1:
        raise ValueError('canvas %dx%d leaves no plot rectangle inside the %d-pixel margins' % (h, w, MARGIN_PX))
    return h - 2 * MARGIN_PX, w - 2 * MARGIN_PX


def render_scatter(X, limits, canvas=DEFAULT_CANVAS, marker_px=2, alpha=0.2, colour=DEFAULT_COLOUR, return_counts=False):
    """scatter plot of the (N, 2) float64 device tensor ``X`` inside the axis ``limits`` (lo0, hi0, lo1, hi1) -> (H, W, 3) uint8 RGB
    device tensor; with ``return_counts`` also the (Ph, Pw) uint32 marker counts of the plot rectangle (as int64)"""
    if not torch.is_tensor(X) or not X.is_cuda:
        raise RuntimeError('the clip-code figure is drawn on the GPU (csrc/code_pca.hip); there is no CPU fallback')
    if X.dtype != torch.float64 or X.ndim != 2 or X.shape[1] != 2 or X.shape[0] < 1:
        raise ValueError('X must be (N, 2) float64, got %s %s' % (tuple(X.shape), X.dtype))
    lim = [float(v) for v in limits]
    if len(lim) != 4 or not all(math.isfinite(v) for v in lim) or not (lim[1] > lim[0] and lim[3] > lim[2]):
        raise ValueError('limits must be finite (lo0, hi0, lo1, hi1) with hi > lo, got %r' % (limits,))
    h, w = (int(v) for v in canvas)
    ph, pw = plot_rectangle((h, w))
    table = colour_table(alpha, colour)
    lib = _lib.load()
    dev = X.device
    X = X.contiguous()
    with torch.cuda.device(dev):
        raw = torch.cuda.current_stream(dev).cuda_stream
        lim_d = torch.tensor(lim, dtype=torch.float64, device=dev)
        table_d = torch.from_numpy(table).to(dev)
        counts = torch.zeros((ph, pw), dtype=torch.int32, device=dev)  # the kernels expect zeroed counters (include/sdt_hip.h)
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        _lib.check(lib.sdt_code_pca_raster(_p(X), X.shape[0], _p(lim_d), _p(table_d), table.shape[0], h, w, MARGIN_PX, int(marker_px),
                                           _p(counts), counts.numel(), _p(out), out.numel(), raw))
    if return_counts:
        return out, counts.to(torch.int64) & 0xFFFFFFFF
    return out


def clip_code_figure(codes, canvas=DEFAULT_CANVAS, marker_px=2, alpha=0.2, colour=DEFAULT_COLOUR, return_meta=False):
    """``fit_project`` then ``render_scatter``: the figure of a code table -> (H, W, 3) uint8 RGB device tensor; with ``return_meta``
    also the numbers a figure with axes would show ({'explained_variance_ratio', 'limits', 'n_rows', 'dim', 'sweeps'})"""
    fit = fit_project(codes)
    image = render_scatter(fit['X'], fit['limits'], canvas, marker_px, alpha, colour)
    if not return_meta:
        return image
    return image, {'explained_variance_ratio': tuple(float(v) for v in fit['explained_variance_ratio']), 'limits': fit['limits'],
                   'n_rows': fit['n_rows'], 'dim': fit['dim'], 'sweeps': fit['sweeps']}


def describe(meta):
    """'evr=(a, b) limits=(lo0, hi0, lo1, hi1)' of a ``clip_code_figure`` meta dict (the epoch log line and the CLI print it)"""
    return 'evr=(%.6f, %.6f) limits=(%.6g, %.6g, %.6g, %.6g)' % (tuple(meta['explained_variance_ratio']) + tuple(meta['limits']))


def save_png(path, image, meta=None):
    """``image`` (H, W, 3) uint8 RGB (device tensor or numpy) -> PNG; ``meta`` items become tEXt chunks (repr of each value)"""
    from PIL import Image
    from PIL.PngImagePlugin import PngInfo
    from .video import to_host
    info = PngInfo()
    for k, v in (meta or {}).items():
        info.add_text(str(k), repr(v))
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    Image.fromarray(np.ascontiguousarray(to_host(image))).save(path, format='PNG', pnginfo=info)
    return path


def _canvas(text):
    try:
        h, w = (int(v) for v in text.lower().split('x'))
    except ValueError:
        raise argparse.ArgumentTypeError('canvas must be HxW, e.g. 480x640')
    return h, w


def load_code_table(checkpoint, key=None):
    """(key, table) of a checkpoint's code table: ``key`` of model_state_dict, or the first of CODE_KEYS that exists (host tensor)"""
    sd = torch.load(checkpoint, map_location='cpu')['model_state_dict']
    found = key or next((k for k in CODE_KEYS if k in sd), None)
    if found is None or found not in sd:
        raise KeyError('%s: no code table under %s' % (checkpoint, key or ' / '.join(CODE_KEYS)))
    return found, sd[found]


def main(argv=None):
    ap = argparse.ArgumentParser(description="the clip-code PCA figure of a checkpoint (the reference's train/clip_code), drawn on the GPU")
    ap.add_argument('--checkpoint', required=True, help='a .pth of this engine or of the reference (same wire format)')
    ap.add_argument('--out', required=True, help='PNG to write')
    ap.add_argument('--key', help='entry of model_state_dict; default: the first of %s that exists' % ', '.join(CODE_KEYS))
    ap.add_argument('--canvas', type=_canvas, default=DEFAULT_CANVAS, help='HxW, default 480x640')
    ap.add_argument('--marker-px', type=int, default=2)
    a = ap.parse_args(argv)
    key, table = load_code_table(a.checkpoint, a.key)
    if not torch.cuda.is_available():
        raise RuntimeError('the clip-code figure is computed on the GPU (csrc/code_pca.hip); there is no CPU fallback')
    image, meta = clip_code_figure(table.float().cuda(), canvas=a.canvas, marker_px=a.marker_px, return_meta=True)
    meta['key'] = key
    save_png(a.out, image, meta)
    print('%s %s (%d, %d): %s -> %s' % (a.checkpoint, key, meta['n_rows'], meta['dim'], describe(meta), a.out))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
