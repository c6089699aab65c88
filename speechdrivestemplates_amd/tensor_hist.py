"""Per-tensor weight and gradient histograms on the GPU (csrc/tensor_hist.hip).

``FlatAdam`` keeps the parameters, gradients, moments and EMA of an optimiser in one contiguous fp32 buffer each, with per-tensor offsets.
One segmented pass over such a buffer gives, per tensor, the bucket counts over TensorBoard's default 1549 edges, the finite / NaN / inf
tallies and min, max, sum and sum of squares in float64 -- about 12 KB per tensor cross to the host instead of the buffer.  Counts and
tallies are integers (exact); the float64 sums have one fixed order, which ``model_histograms`` restates in numpy bit for bit.

    python -m speechdrivestemplates_amd.tensor_hist --checkpoint X.pth [--ema] [--out hist.npz]
        one line per floating-point tensor of the checkpoint's model_state_dict (--ema: model_ema_state_dict): name, numel, min, max, mean, std,
        zeros (|v| < 1e-12: the two buckets around 0), non-finite; --out writes the raw counts / tallies / stats arrays
"""
import math

import numpy as np

from .optim import _tree256

# launch constants of csrc/tensor_hist.hip (checked against the library by the tests)
HIST_THREADS, HIST_CHUNK, NUM_BUCKETS = 256, 16384, 1548
WHICH = ('param', 'grad', 'exp_avg', 'exp_avg_sq', 'ema')


def _bucket_edges():
    """the edges torch.utils.tensorboard uses by default: +-1e-12 * 1.1^k below 1e20 (774 per sign) around 0.0, in float64"""
    pos, v = [], 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    return np.array([-x for x in reversed(pos)] + [0.0] + pos, dtype=np.float64)


BUCKET_EDGES = _bucket_edges()
BUCKET_EDGES.setflags(write=False)


# -- the numpy contract model -----------------------------------------------------------------------------------------------------------
def _scaled(x, scale):
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        return np.ascontiguousarray(x, dtype=np.float32).reshape(-1) * np.float32(scale)  # one fp32 multiply


def _model_segment(v32):
    """(counts, tallies, stats) of one segment of scaled fp32 values, in the kernel's order"""
    n = v32.size
    finite = np.isfinite(v32)
    v = v32.astype(np.float64)
    tallies = np.array([int(finite.sum()), int(np.isnan(v32).sum()), int(np.isinf(v32).sum())], dtype=np.int64)
    idx = np.clip(np.searchsorted(BUCKET_EDGES, v[finite], 'right') - 1, 0, NUM_BUCKETS - 1)
    counts = np.bincount(idx, minlength=NUM_BUCKETS).astype(np.int64)
    stats = np.array([np.inf, -np.inf, 0.0, 0.0], dtype=np.float64)
    if tallies[0]:
        stats[0], stats[1] = v[finite].min(), v[finite].max()
    nch = -(-n // HIST_CHUNK)
    if nch == 0:
        return counts, tallies, stats
    # an absent or non-finite element adds nothing: adding +0 to an accumulator that started at +0 leaves its bits
    vals = np.zeros(nch * HIST_CHUNK, dtype=np.float64)
    vals[:n] = np.where(finite, v, 0.0)
    vals = vals.reshape(nch, HIST_CHUNK // (4 * HIST_THREADS), HIST_THREADS, 4)  # [chunk, trip, thread, element of the float4]
    out = []
    for x in (vals, vals * vals):
        acc = np.zeros((nch, HIST_THREADS), dtype=np.float64)
        for k in range(x.shape[1]):
            for e in range(4):
                acc = acc + x[:, k, :, e]
        part = _tree256(acc)  # one partial per chunk
        trips = -(-nch // HIST_THREADS)
        padded = np.zeros(trips * HIST_THREADS, dtype=np.float64)
        padded[:nch] = part
        facc = np.zeros(HIST_THREADS, dtype=np.float64)
        for k in range(trips):
            facc = facc + padded[k * HIST_THREADS:(k + 1) * HIST_THREADS]
        out.append(np.float64(_tree256(facc)))
    stats[2], stats[3] = out
    return counts, tallies, stats


def model_histograms(flat_np, offsets, sizes, scale=1.0):
    """Contract model of ``flat_histograms`` -> (counts (S, 1548) int64, tallies (S, 3) int64, stats (S, 4) float64).  Every element is
    v = fp32(x * scale) widened to float64; bucket = searchsorted(E, v, 'right') - 1 clipped to [0, 1547]; sums in the kernel's order: chunks
    of HIST_CHUNK elements; in a chunk thread t adds the float4s t, t + 256, ... (element 0 first) to an accumulator that starts at +0; a
    butterfly over each wave, (w0 + w1) + (w2 + w3) per chunk; then thread t adds the chunk partials t, t + 256, ... and the same tree."""
    flat_np = np.ascontiguousarray(flat_np, dtype=np.float32).reshape(-1)
    S = len(offsets)
    counts, tallies, stats = np.zeros((S, NUM_BUCKETS), np.int64), np.zeros((S, 3), np.int64), np.zeros((S, 4), np.float64)
    for s, (off, n) in enumerate(zip(offsets, sizes)):
        counts[s], tallies[s], stats[s] = _model_segment(_scaled(flat_np[off:off + n], scale))
    return counts, tallies, stats


def model_depth(n):
    """The largest number of float64 additions any one term passes through in ``model_histograms`` for a segment of ``n`` elements: a
    thread's serial run (HIST_CHUNK / 256), the 6 + 2 tree levels of its chunk, the final workgroup's serial run and its 6 + 2 levels."""
    nch = max(1, -(-n // HIST_CHUNK))
    return HIST_CHUNK // HIST_THREADS + 8 + (-(-nch // HIST_THREADS)) + 8


# -- the device path ----------------------------------------------------------------------------------------------------------------
_PLANS, _EDGES = {}, {}
NO_GPU = 'tensor_hist runs on the GPU only (no CPU fallback)'


def _plan(flat, offsets, sizes):
    key = (flat.device, flat.numel(), tuple(int(o) for o in offsets), tuple(int(s) for s in sizes))
    plan = _PLANS.get(key)
    if plan is None:
        from . import ops
        seg, chunks = ops.tensor_hist_plan(key[2], key[3], key[1])
        plan = _PLANS[key] = (seg.to(flat.device), chunks.to(flat.device))
    return plan


def _edges(dev):
    import torch
    if dev not in _EDGES:
        _EDGES[dev] = torch.from_numpy(np.array(BUCKET_EDGES)).to(dev)
    return _EDGES[dev]


def flat_histograms(flat, offsets, sizes, scale=1.0):
    """-> device tensors counts (S, 1548) int64, tallies (S, 3) int64 {finite, NaN, inf}, stats (S, 4) float64 {min, max, sum, sum of
    squares} of the segments ``flat[offsets[s] : offsets[s] + sizes[s]]`` scaled by ``scale`` in fp32.  Eager launches on the current
    stream, no host synchronisation (the tables of a new (device, offsets, sizes) are uploaded once)."""
    import torch
    from . import ops
    if not torch.is_tensor(flat) or not flat.is_cuda:
        raise RuntimeError(NO_GPU)
    if flat.dtype != torch.float32 or flat.dim() != 1 or not flat.is_contiguous():
        raise ValueError('flat must be a contiguous 1-D fp32 buffer, got %s %s' % (tuple(flat.shape), flat.dtype))
    scale = float(scale)
    if scale != scale:
        raise ValueError('scale is NaN')
    with torch.cuda.device(flat.device):
        seg, chunks = _plan(flat, offsets, sizes)
        S, dev = seg.shape[0], flat.device
        counts = torch.empty((S, NUM_BUCKETS), dtype=torch.int64, device=dev)
        tallies = torch.empty((S, 3), dtype=torch.int64, device=dev)
        stats = torch.empty((S, 4), dtype=torch.float64, device=dev)
        partials = torch.empty(4 * max(1, chunks.shape[0]), dtype=torch.float64, device=dev)
        ops.tensor_hist(flat.detach(), seg, chunks, _edges(dev), scale, counts, tallies, stats, partials)
    return counts, tallies, stats


def optimizer_histograms(opt, which):
    """``flat_histograms`` over one buffer of a ``FlatAdam``, one row per ``opt.params`` entry.  'grad' is scaled by ``opt.grad_scale``: the
    gradient Adam consumes, before clipping (as the logged grad_norm_*)."""
    if which not in WHICH:
        raise ValueError('which must be one of %s, got %r' % (', '.join(WHICH), which))
    buf = {'param': opt.flat_param, 'grad': opt.flat_grad, 'exp_avg': opt.exp_avg, 'exp_avg_sq': opt.exp_avg_sq, 'ema': opt.ema}[which]
    if buf is None:
        raise RuntimeError('this optimiser keeps no EMA (enable_ema)')
    return flat_histograms(buf, opt.offsets, [p.numel() for p in opt.params], opt.grad_scale if which == 'grad' else 1.0)


# -- TensorBoard's HistogramProto ---------------------------------------------------------------------------------------------------
def to_proto_fields(counts_row, tallies_row, stats_row):
    """-> (min, max, num, sum, sum_squares, bucket_limit, bucket) as torch's ``make_histogram`` trims them: the bins from the first to the
    last non-zero one plus one empty bin to the left (a zero count is prepended when the first non-zero bin is bin 0); ``bucket_limit`` =
    the left edge of the first kept bin, then the right edges of the kept bins (the first kept bin when one was prepended is the empty
    one, so the lists keep equal length).  ``num`` is the finite count.  None when the segment has no finite element."""
    counts = np.asarray(counts_row, dtype=np.int64).reshape(-1)
    if int(tallies_row[0]) == 0 or not counts.any():
        return None
    nz = np.flatnonzero(counts)
    first, last = int(nz[0]), int(nz[-1]) + 1  # counts[first:last] runs from the first to the last non-zero bin
    if first > 0:
        bucket = counts[first - 1:last]
    else:
        bucket = np.concatenate([[0], counts[:last]])
    limits = BUCKET_EDGES[first:last + 1]
    return (float(stats_row[0]), float(stats_row[1]), float(int(tallies_row[0])), float(stats_row[2]), float(stats_row[3]),
            [float(x) for x in limits], [float(x) for x in bucket])


# -- command line -------------------------------------------------------------------------------------------------------------------
def checkpoint_histograms(state_dict):
    """(names, numels, counts, tallies, stats) of every floating-point tensor of a state dict, computed on the GPU (numpy results)"""
    import torch
    items = [(k, v) for k, v in state_dict.items() if torch.is_tensor(v) and v.is_floating_point() and v.numel() > 0]
    if not items:
        raise ValueError('the state dict holds no floating-point tensor')
    offsets, total = [], 0
    for _, v in items:
        offsets.append(total)
        total += (v.numel() + 3) // 4 * 4
    flat = torch.zeros(total, dtype=torch.float32, device='cuda')
    sizes = [v.numel() for _, v in items]
    for (_, v), off in zip(items, offsets):
        flat[off:off + v.numel()].copy_(v.detach().reshape(-1))
    counts, tallies, stats = flat_histograms(flat, offsets, sizes)
    return [k for k, _ in items], sizes, counts.cpu().numpy(), tallies.cpu().numpy(), stats.cpu().numpy()


def describe(names, sizes, counts, tallies, stats):
    lines = []
    for i, name in enumerate(names):
        fin = int(tallies[i, 0])
        mean = stats[i, 2] / fin if fin else float('nan')
        std = math.sqrt(max(stats[i, 3] / fin - mean * mean, 0.0)) if fin else float('nan')
        lines.append('%s numel=%d min=%.6g max=%.6g mean=%.6g std=%.6g zeros=%d nonfinite=%d'
                     % (name, sizes[i], stats[i, 0], stats[i, 1], mean, std, int(counts[i, 773] + counts[i, 774]),
                        int(tallies[i, 1] + tallies[i, 2])))
    return lines


def main(argv=None):
    import argparse
    import torch
    ap = argparse.ArgumentParser(description='per-tensor statistics and histograms of a checkpoint, computed on the GPU')
    ap.add_argument('--checkpoint', required=True)
    ap.add_argument('--ema', action='store_true', help="read 'model_ema_state_dict' instead of 'model_state_dict'")
    ap.add_argument('--out', metavar='NPZ', help='write names, numel, counts, tallies, stats and the bucket edges')
    a = ap.parse_args(argv)
    ckpt = torch.load(a.checkpoint, map_location='cpu')
    key = 'model_ema_state_dict' if a.ema else 'model_state_dict'
    if key not in ckpt:
        raise SystemExit('%s carries no %r' % (a.checkpoint, key))
    names, sizes, counts, tallies, stats = checkpoint_histograms(ckpt[key])
    print('\n'.join(describe(names, sizes, counts, tallies, stats)))
    if a.out:
        np.savez(a.out, names=np.array(names), numel=np.array(sizes, dtype=np.int64), counts=counts, tallies=tallies, stats=stats,
                 bucket_edges=BUCKET_EDGES)


if __name__ == '__main__':
    main()
