"""Clusters of the template-code table and the table row that stands for each, on the GPU (csrc/code_clusters.hip).

``code_axes`` answers "what does the extreme of direction 0 look like"; the demos ask something else: which handful of distinct templates
a speaker has, and which row of the table stands for each.  This tool runs k-means on the table (k-means++ or farthest-point seeding,
Lloyd's iteration), numbers the clusters by descending size and names each cluster's medoid.  Its npz is what both demos consume:
``v`` holds one code per cluster centre for ``np.load(DEMO.CODE_PATH)['v'][idx] * 10`` (pose2pose.py:50-56, DEMO.MULTIPLE k), and
``code_index`` the rows for DEMO.CODE_INDEX / DEMO.CODE_INDEX_B (voice2pose.py:107-117).

    python -m speechdrivestemplates_amd.code_clusters --checkpoint X.pth --out clusters.npz [--k 8] [--seed 0] [--init kmeans++|farthest]
                                                      [--max-iter 100] [--table KEY]
    python -m speechdrivestemplates_amd.code_clusters --codes table.npy --out clusters.npz

Everything is float64 on values converted exactly from the fp32 table, every operation rounded on its own, every sum over rows in chunks of
1024 rows (rows ascending from +0.0, then chunks ascending); the ``model_*`` functions restate the kernels in numpy with the same order.
"""
import argparse
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .code_axes import _check, nearest_codes
from .code_pca import _as_table, _moments, load_code_table

CHUNK = 1024
MAX_ROWS = 1 << 24
MAX_K = 64
INITS = ('kmeans++', 'farthest')
NO_GPU = 'the code clusters are computed on the GPU (csrc/code_clusters.hip); there is no CPU fallback'
RULES = ('walk', 'chunk-last', 'table-last', 'no-distance', 'farthest')  # what chose a seed (sdt_code_clusters_seed_pick's info[3])


def _p(t):
    return C.c_void_p(t.data_ptr())


def _check_args(n, k, init, max_iter):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError('k must be an integer, got %r' % (k,))
    if not 1 <= k <= MAX_K:
        raise ValueError('k must lie in [1, %d], got %d' % (MAX_K, k))
    if k > n:
        raise ValueError('k = %d exceeds the %d rows of the table' % (k, n))
    if n > MAX_ROWS:
        raise ValueError('the table has %d rows; at most 2^24 are supported' % n)
    if init not in INITS:
        raise ValueError('init must be one of %s, got %r' % (', '.join(INITS), init))
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError('max_iter must be an integer of at least 1, got %r' % (max_iter,))
    return int(k), int(max_iter)


def _table(table):
    if not torch.is_tensor(table) or not table.is_cuda:
        raise RuntimeError(NO_GPU)
    return _as_table(table)


def draw_uniforms(seed, k):
    """the k numbers in [0, 1) that k-means++ consumes, one per seed"""
    return np.random.Generator(np.random.PCG64(int(seed))).random(int(k))


def first_row(u0, n):
    """seed 0 of k-means++"""
    return min(int(u0 * n), n - 1)


def tenth_float32(centers):
    """the float32 nearest to centers / 10, ties to even.  The float64 quotient cast to float32 is rounded twice, yet equals the quotient
    rounded once: a float64 c whose tenth is not a float32 tie misses that tie by at least ulp(c) / 10 >= 0.8 float64 ulps of the tie
    (ulp(c) is 8 or 16 ulps of c / 10), so the float64 quotient never lands on a tie that the exact quotient is not on."""
    return (np.asarray(centers, np.float64) / 10.0).astype(np.float32)


# -- the stages on the device -----------------------------------------------------------------------------------------------------------
def choose_seeds(x, k, seed=0, init='kmeans++', history=None):
    """k seed rows of the (N, D) fp32 device table ``x`` -> (seeds (k,) int64, m (N,) float64 = every row's d2 to its nearest seed,
    rules: what chose each seed), device tensors.  ``history``: a list that receives {'stage': 'seed', 'j', 'm', 'info'} per seed."""
    x = _table(x)
    n, d = x.shape
    k, _ = _check_args(n, k, init, 1)
    lib = _lib.load()
    dev = x.device
    with torch.cuda.device(dev):
        raw = torch.cuda.current_stream(dev).cuda_stream
        u = draw_uniforms(seed, k)
        seeds = torch.zeros(k, dtype=torch.int64, device=dev)
        if init == 'kmeans++':
            seeds[0] = first_row(u[0], n)
        else:
            mean, _ = _moments(lib, x, raw)
            seeds[0:1] = nearest_codes(x, mean.reshape(1, d))[0]
        ws_bytes = lib.sdt_code_clusters_seed_workspace_bytes(n, d)
        if ws_bytes <= 0:
            raise ValueError('unsupported table size (%d, %d)' % (n, d))
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
        m = torch.empty(n, dtype=torch.float64, device=dev)
        info = torch.zeros((k, 4), dtype=torch.float64, device=dev)
        for j in range(k):
            if j:
                _check(lib.sdt_code_clusters_seed_pick(_p(m), n, INITS.index(init), float(u[j]), _p(seeds), j, _p(info[j]), _p(ws), ws_bytes, raw))
            _check(lib.sdt_code_clusters_seed_update(_p(x), n, d, _p(seeds), j, int(j == 0), _p(m), _p(ws), ws_bytes, raw))
            if history is not None:
                history.append({'stage': 'seed', 'j': j, 'seed': int(seeds[j].item()), 'm': m.cpu().numpy(), 'info': info[j].cpu().numpy()})
    return seeds, m, info


def assign(x, centers, labels, first):
    """labels[n] = the nearest of the (k, D) float64 ``centers`` (of equals the lowest), in place -> the number of labels that changed"""
    n, d = x.shape
    lib = _lib.load()
    with torch.cuda.device(x.device):
        raw = torch.cuda.current_stream(x.device).cuda_stream
        changed = torch.empty(1, dtype=torch.int64, device=x.device)
        _check(lib.sdt_code_clusters_assign(_p(x), n, d, _p(centers), centers.shape[0], _p(labels), int(bool(first)), _p(changed), raw))
        return int(changed.item())  # the one read-back of an iteration


def update(x, labels, centers, ws=None):
    """centers[c] = the ordered mean of the rows labelled c, in place (an empty cluster keeps its centre) -> counts (k,) int32"""
    n, d = x.shape
    k = centers.shape[0]
    lib = _lib.load()
    with torch.cuda.device(x.device):
        raw = torch.cuda.current_stream(x.device).cuda_stream
        ws_bytes = lib.sdt_code_clusters_update_workspace_bytes(n, d, k)
        if ws_bytes <= 0:
            raise ValueError('unsupported sizes: (%d, %d) with k = %d' % (n, d, k))
        if ws is None:
            ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=x.device)
        counts = torch.empty(k, dtype=torch.int32, device=x.device)
        _check(lib.sdt_code_clusters_update(_p(x), n, d, _p(labels), k, _p(centers), _p(counts), _p(ws), ws_bytes, raw))
    return counts


def final_pass(x, centers):
    """the last assignment against ``centers`` and everything the file holds, clusters numbered by descending count -> dict of device
    tensors: labels (N,) int32, centers (k, D), counts (k,) int32, within_ss (k,), inertia (), code_index (k,) int64, code_dist2 (k,),
    order (k,) int32 (the number each cluster had before)"""
    n, d = x.shape
    k = centers.shape[0]
    lib = _lib.load()
    dev = x.device
    with torch.cuda.device(dev):
        raw = torch.cuda.current_stream(dev).cuda_stream
        ws_bytes = lib.sdt_code_clusters_final_workspace_bytes(n, d, k)
        if ws_bytes <= 0:
            raise ValueError('unsupported sizes: (%d, %d) with k = %d' % (n, d, k))
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        out = {'labels': torch.empty(n, **i32), 'centers': torch.empty((k, d), **f64), 'counts': torch.empty(k, **i32),
               'within_ss': torch.empty(k, **f64), 'inertia': torch.empty(1, **f64), 'code_index': torch.empty(k, dtype=torch.int64, device=dev),
               'code_dist2': torch.empty(k, **f64), 'order': torch.empty(k, **i32)}
        _check(lib.sdt_code_clusters_final(_p(x), n, d, _p(centers), k, _p(out['labels']), _p(out['centers']), _p(out['counts']),
                                           _p(out['within_ss']), _p(out['inertia']), _p(out['code_index']), _p(out['code_dist2']),
                                           _p(out['order']), _p(ws), ws_bytes, raw))
    out['inertia'] = out['inertia'].reshape(())
    return out


def fit_clusters(table, k, seed=0, init='kmeans++', max_iter=100, history=None):
    """k-means of the (N, D) / (N, F, D) fp32 device ``table``.  -> {'centers' (k, D) float64, 'v' (k, D) float32 = centers / 10 rounded
    once, 'code_index' (k,) int64 (the member row nearest to its centre; -1: no member), 'code_dist2' (k,), 'counts' (k,) int32, 'labels'
    (N,) int32, 'within_ss' (k,), 'inertia' (), 'seeds' (k,) int64 in the order they were chosen, 'order' (k,) int32 (cluster i grew from
    seeds[order[i]]): device tensors; 'iterations', 'converged', 'empty_clusters', 'n_rows', 'dim'}.  Clusters are numbered by descending
    count (ties: the lower original number).  ``history``: a list that receives one record per seed and per iteration (host copies)."""
    x = _table(table)
    n, d = x.shape
    k, max_iter = _check_args(n, k, init, max_iter)
    lib = _lib.load()
    dev = x.device
    with torch.cuda.device(dev):
        raw = torch.cuda.current_stream(dev).cuda_stream
        _moments(lib, x, raw)  # the bad-row word: a non-finite row is reported before any other kernel sees the table
        seeds, _, _ = choose_seeds(x, k, seed, init, history)
        centers = x[seeds].double()  # (exact)
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        ws_bytes = lib.sdt_code_clusters_update_workspace_bytes(n, d, k)
        if ws_bytes <= 0:
            raise ValueError('unsupported sizes: (%d, %d) with k = %d' % (n, d, k))
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
        iterations, converged = 0, False
        while iterations < max_iter and not converged:
            iterations += 1
            changed = assign(x, centers, labels, iterations == 1)
            counts = update(x, labels, centers, ws)
            converged = changed == 0
            if history is not None:
                history.append({'stage': 'iteration', 'iteration': iterations, 'changed': changed, 'labels': labels.cpu().numpy(),
                                'centers': centers.cpu().numpy(), 'counts': counts.cpu().numpy()})
        out = final_pass(x, centers)
    out.update(v=torch.from_numpy(tenth_float32(out['centers'].cpu().numpy())).to(dev), seeds=seeds, iterations=iterations, converged=converged,
               empty_clusters=int((out['counts'] == 0).sum().item()), n_rows=n, dim=d)
    return out


# -- the contract in numpy: the kernels' arithmetic in the kernels' order ----------------------------------------------------------------
def _f64(table):
    x = np.asarray(table)
    return x.reshape(-1, x.shape[-1]).astype(np.float64)


def model_d2(x, b):
    """d2 of every row of the float64 (N, D) ``x`` to the point ``b``: sum over d ascending of (x[n, d] - b[d])^2"""
    acc = np.zeros(x.shape[0])
    for d in range(x.shape[1]):
        diff = x[:, d] - b[d]
        acc = acc + diff * diff
    return acc


def chunk_sums(v):
    """the ordered sum of every chunk of 1024 consecutive entries, from +0.0 (padding a non-negative sum with +0.0 changes no bit)"""
    chunks = -(-len(v) // CHUNK)
    padded = np.zeros(chunks * CHUNK)
    padded[:len(v)] = v
    return np.cumsum(padded.reshape(chunks, CHUNK), axis=1)[:, -1]


def _lowest_free_row(seeds):
    return next(c for c in range(len(seeds) + 1) if c not in seeds)


def model_seed_pick(m, init, u, seeds):
    """the next seed given ``m`` and the rows chosen so far -> (row, rule)"""
    m = np.asarray(m, np.float64)
    seeds = [int(s) for s in seeds]
    if init == 'farthest':
        row = int(np.argmax(m))  # (the first of equal maxima)
        return (row, 'farthest') if m[row] > 0.0 else (_lowest_free_row(seeds), 'no-distance')
    P = np.cumsum(chunk_sums(m))
    T = P[-1]
    if not T > 0.0:
        return _lowest_free_row(seeds), 'no-distance'
    r = float(u) * T
    passing = np.nonzero(P > r)[0]
    if len(passing) == 0:
        return int(np.nonzero(m > 0.0)[0][-1]), 'table-last'
    c = int(passing[0])
    part = m[c * CHUNK:(c + 1) * CHUNK]
    walk = np.cumsum(np.concatenate([[P[c - 1] if c else 0.0], part]))[1:]
    over = np.nonzero(walk > r)[0]
    if len(over):
        return c * CHUNK + int(over[0]), 'walk'
    return c * CHUNK + int(np.nonzero(part > 0.0)[0][-1]), 'chunk-last'


def model_seeds(table, k, seed=0, init='kmeans++', first_seed=None, history=None):
    """-> (seeds (k,) int64, m (N,), rules).  ``first_seed`` replaces seed 0 (farthest: the row nearest to the DEVICE's mean, whose
    summation order the models do not restate; without it the row nearest to numpy's mean)"""
    x = _f64(table)
    n = x.shape[0]
    u = draw_uniforms(seed, k)
    if first_seed is None:
        if init == 'kmeans++':
            first_seed = first_row(u[0], n)
        else:
            first_seed = int(np.argmin(model_d2(x, x.mean(axis=0))))
    seeds, rules = [int(first_seed)], ['first']
    m = np.full(n, np.inf)
    for j in range(k):
        if j:
            row, rule = model_seed_pick(m, init, u[j], seeds)
            seeds.append(row)
            rules.append(rule)
        m = np.minimum(m, model_d2(x, x[seeds[j]]))
        if history is not None:
            history.append({'stage': 'seed', 'j': j, 'seed': seeds[j], 'm': m.copy(), 'rule': rules[j]})
    return np.asarray(seeds, np.int64), m, rules


def model_assign(x, centers, block=1 << 15):
    """(labels int32, d2 to the chosen centre): the first of equally near centres"""
    k = centers.shape[0]
    labels, dist = np.empty(x.shape[0], np.int32), np.empty(x.shape[0])
    for a in range(0, x.shape[0], block):
        xb = x[a:a + block]
        d2 = np.zeros((xb.shape[0], k))
        for d in range(x.shape[1]):
            diff = xb[:, d:d + 1] - centers[None, :, d]
            d2 = d2 + diff * diff
        lab = np.argmin(d2, axis=1)
        labels[a:a + block] = lab
        dist[a:a + block] = d2[np.arange(xb.shape[0]), lab]
    return labels, dist


def _ordered_by_cluster(values, labels, k):
    """per cluster the sum of ``values`` ((N,) or (N, D)) over its members: rows ascending inside every chunk from +0.0, then chunks
    ascending.  The kernels add +0.0 for a row of another cluster; a sum that starts at +0.0 is never -0.0, so that changes no bit and
    the model leaves those additions out."""
    n = len(labels)
    chunks = -(-n // CHUNK)
    acc = np.zeros((chunks, k) + values.shape[1:])
    for i in range(min(CHUNK, n)):
        lab = labels[i::CHUNK]
        idx = np.arange(len(lab))
        acc[idx, lab] = acc[idx, lab] + values[i::CHUNK]
    return np.cumsum(acc, axis=0)[-1]


def model_update(x, labels, centers):
    """-> (new centres, counts int32)"""
    k = centers.shape[0]
    counts = np.bincount(labels, minlength=k).astype(np.int32)
    total = _ordered_by_cluster(x, labels, k)
    new = centers.copy()
    full = counts > 0
    new[full] = total[full] / counts[full, None].astype(np.float64)
    return new, counts


def model_final(x, centers):
    """the final pass -> dict of numpy arrays with ``final_pass``'s keys"""
    k = centers.shape[0]
    labels, dist = model_assign(x, centers)
    counts = np.bincount(labels, minlength=k).astype(np.int32)
    ss = _ordered_by_cluster(dist, labels, k)
    index, best = np.full(k, -1, np.int64), np.full(k, np.inf)
    for c in range(k):
        members = np.nonzero(labels == c)[0]
        if len(members):
            at = members[int(np.argmin(dist[members]))]  # (the first of equal distances: the lowest row)
            index[c], best[c] = at, dist[at]
    order = np.asarray(sorted(range(k), key=lambda c: (-int(counts[c]), c)), np.int32)
    rank = np.empty(k, np.int32)
    rank[order] = np.arange(k, dtype=np.int32)
    within = ss[order]
    return {'labels': rank[labels], 'centers': centers[order], 'counts': counts[order], 'within_ss': within,
            'inertia': np.cumsum(within)[-1], 'code_index': index[order], 'code_dist2': best[order], 'order': order}


def model_fit(table, k, seed=0, init='kmeans++', max_iter=100, first_seed=None, history=None):
    """``fit_clusters`` on the host, numpy arrays in place of device tensors"""
    x = _f64(table)
    n, d = x.shape
    k, max_iter = _check_args(n, k, init, max_iter)
    seeds, _, _ = model_seeds(table, k, seed, init, first_seed, history)
    centers = x[seeds].copy()
    labels = None
    iterations, converged = 0, False
    while iterations < max_iter and not converged:
        iterations += 1
        new_labels, _ = model_assign(x, centers)
        changed = n if labels is None else int((new_labels != labels).sum())
        labels = new_labels
        centers, counts = model_update(x, labels, centers)
        converged = changed == 0
        if history is not None:
            history.append({'stage': 'iteration', 'iteration': iterations, 'changed': changed, 'labels': labels.copy(), 'centers': centers.copy(),
                            'counts': counts})
    out = model_final(x, centers)
    out.update(v=tenth_float32(out['centers']), seeds=seeds, iterations=iterations, converged=converged,
               empty_clusters=int((out['counts'] == 0).sum()), n_rows=n, dim=d)
    return out


# -- the file ------------------------------------------------------------------------------------------------------------------------------
FILE_KEYS = ('centers', 'v', 'code_index', 'code_dist2', 'counts', 'labels', 'within_ss', 'inertia', 'seeds', 'order')


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def write_clusters(path, fit):
    """one npz: FILE_KEYS of ``fit`` (v float32 (k, D): what ``np.load(DEMO.CODE_PATH)['v'][idx] * 10`` indexes), iterations, converged,
    empty_clusters"""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, 'wb') as f:  # (np.savez would append '.npz' to a path without it; DEMO.CODE_PATH is opened as given)
        np.savez(f, iterations=np.int64(fit['iterations']), converged=np.bool_(fit['converged']), empty_clusters=np.int64(fit['empty_clusters']),
                 **{key: _host(fit[key]) for key in FILE_KEYS})
    return path


def main(argv=None):
    ap = argparse.ArgumentParser(description='k-means clusters of a code table and the row that stands for each, for the two demo modes')
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--checkpoint', help='a .pth of this engine or of the reference (same wire format)')
    src.add_argument('--codes', help='a bare (N, D) or (N, F, D) table as .npy (external codes)')
    ap.add_argument('--out', required=True, help='npz to write')
    ap.add_argument('--table', help='entry of model_state_dict; default: the first of module.clips_code, module.clip_code_mu that exists')
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--init', choices=INITS, default='kmeans++')
    ap.add_argument('--max-iter', type=int, default=100)
    a = ap.parse_args(argv)
    if a.codes:
        key, table = a.codes, torch.from_numpy(np.load(a.codes))
    else:
        key, table = load_code_table(a.checkpoint, a.table)
    if not torch.cuda.is_available():
        raise RuntimeError(NO_GPU)
    fit = fit_clusters(table.float().cuda(), a.k, a.seed, a.init, a.max_iter)
    write_clusters(a.out, fit)
    counts, index, dist2, within = (_host(fit[key_]) for key_ in ('counts', 'code_index', 'code_dist2', 'within_ss'))
    print('%s %s (%d, %d): k=%d init=%s seed=%d: %d iterations, %s, %d empty, inertia %.6g -> %s' % (
        a.checkpoint or a.codes, key, fit['n_rows'], fit['dim'], a.k, a.init, a.seed, fit['iterations'],
        'converged' if fit['converged'] else 'NOT converged', fit['empty_clusters'], float(fit['inertia']), a.out))
    for i in range(a.k):
        print('cluster %d: count %d code_index %d dist2 %.6g within_ss %.6g' % (i, counts[i], index[i], dist2[i], within[i]))
    second = index[1] if a.k > 1 and index[1] >= 0 else index[0]  # (one cluster, or a second one without rows: the first medoid twice)
    print('DEMO.CODE_PATH %s DEMO.MULTIPLE %d' % (a.out, a.k))
    print('DEMO.CODE_INDEX %d DEMO.CODE_INDEX_B %d' % (index[0], second))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
