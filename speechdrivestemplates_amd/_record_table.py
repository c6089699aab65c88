"""The record-table protocol of the per-clip validation metrics, shared by clip_metrics, sync_metrics and motion_dist (DESIGN.md section 22 states it;
csrc/record_table.h is the device side).

A table is a (num_clips + 1, cols) int64 tensor: one record per clip of the validation set, then a header row whose word 0 counts the clip
indices outside the table.  Under data parallelism there is one table per rank; per clip the lowest rank whose record has its seen word set
gives the record.  The epoch sum runs over chunks of 64 clips in index order, then over the chunk partials in order.  The word layouts, what
each word adds up and the final divisions belong to the families.  prdc.FeatureSetAccumulator keeps its feature table under the same protocol
(its epoch stage compares sets of clips instead of summing over them)."""
import numpy as np

from ._exact_model import MAX_COPIES, MAX_K, MAX_TABLES

CHUNK = 64  # clips per chunk of the epoch sum


# ---- the numpy contract model ------------------------------------------------------------------------------------------------------------------
def merge_tables(tables, seen):
    """(N, cols) record arrays, one per rank -> the records the epoch stage reads: per clip the lowest rank that has seen it"""
    tables = [np.asarray(t, dtype=np.int64) for t in tables]
    out = np.zeros_like(tables[0])
    for t in tables:
        take = (out[:, seen] == 0) & (t[:, seen] != 0)
        out[take] = t[take]
    return out


def chunked_records(tables, seen):
    """chunk by chunk in index order, the list of the chunk's records: per clip the one of the lowest rank that has seen it, none if no rank has"""
    tables = [np.asarray(t, dtype=np.int64) for t in tables]
    N = tables[0].shape[0]
    for n0 in range(0, N, CHUNK):
        recs = (next((t[n] for t in tables if t[n, seen] != 0), None) for n in range(n0, min(N, n0 + CHUNK)))
        yield [rec for rec in recs if rec is not None]


def check_num_clips(num_clips):
    num_clips = int(num_clips)
    if num_clips < 1:
        raise ValueError('the table needs at least one clip, got %d' % num_clips)
    return num_clips


# ---- the argument front end of the device routes -----------------------------------------------------------------------------------------------
# ``noun`` names the family in a message ('the clip metrics'), ``no_gpu`` is its own "there is no CPU fallback" sentence.
def check_keypoints(K):
    K = int(K)
    if not 1 <= K <= MAX_K:
        raise ValueError('K = %d keypoints outside [1, %d]' % (K, MAX_K))
    return K


def cuda_device(device, no_gpu):
    """a device argument -> the torch.device of a CUDA device with its index; RuntimeError(``no_gpu``) for any other"""
    import torch
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError(no_gpu)
    return torch.device('cuda', torch.cuda.current_device()) if device.index is None else device


def stream(device):
    """the raw handle of the current stream of ``device``"""
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t):
    import ctypes as C
    return None if t is None else C.c_void_p(t.data_ptr())


def check_poses(x, K, device, noun, no_gpu):
    """a (rows, frames, 2, K) float64 tensor on ``device`` -> detached and contiguous"""
    import torch
    if not torch.is_tensor(x) or x.device != device:
        raise RuntimeError('%s take tensors on %s; %s' % (noun, device, no_gpu))
    if x.dtype != torch.float64 or x.ndim != 4 or x.shape[2] != 2 or x.shape[3] != K or x.shape[0] < 1 or x.shape[1] < 1:
        raise TypeError('poses must be (rows, frames, 2, %d) float64, got %s %s' % (K, tuple(x.shape), x.dtype))
    return x.detach().contiguous()


def check_step(pred, gt, clip_index, multiple, K, device, noun, no_gpu, gt_optional=False):
    """the arguments of one validation step -> (pred, gt, idx, B, R, T, m): the checked pose tensors of R = m * B rows (``gt`` may be None
    only with ``gt_optional``), the first B entries of the int64 ``clip_index`` (of B or R entries) on ``device``, and the sizes"""
    import torch
    m = int(multiple)
    if not 1 <= m <= MAX_COPIES:
        raise ValueError('%d copies outside [1, %d]' % (m, MAX_COPIES))
    pred = check_poses(pred, K, device, noun, no_gpu)
    gt = None if gt is None and gt_optional else check_poses(gt, K, device, noun, no_gpu)
    R, T = pred.shape[:2]
    if (gt is not None and pred.shape != gt.shape) or R % m:
        raise ValueError('prediction %s and ground truth %s must be %d copies of one batch' % (
            tuple(pred.shape), None if gt is None else tuple(gt.shape), m))
    B = R // m
    if not torch.is_tensor(clip_index) or clip_index.dtype != torch.int64 or clip_index.ndim != 1 or clip_index.numel() not in (B, R):
        raise TypeError('clip_index must be an int64 tensor of %d (or %d) entries' % (B, R))
    return pred, gt, clip_index[:B].to(device, non_blocking=True).contiguous(), B, R, T, m


# ---- the device route --------------------------------------------------------------------------------------------------------------------------
class RecordTable:
    """The state of an accumulator: a table of ``num_clips`` records of ``cols`` words on ``device`` (any CUDA device argument), the
    workspace of the epoch stage and its output vector.  A subclass sets ``NOUN`` / ``NO_GPU`` (its name in a message, its "no CPU fallback"
    sentence) and ``self.K``, keeps its ``add``, launches its epoch stage in ``_launch_epoch(ptrs, ranks, stream)`` (-> the status of the C
    call) and names the words of the epoch vector in ``epoch_values(words)``."""
    NOUN = NO_GPU = None
    _p = staticmethod(ptr)

    def __init__(self, num_clips, device, cols, chunk_words, out_words):
        import torch
        self.num_clips, self.device = num_clips, cuda_device(device, self.NO_GPU)
        device = self.device
        self._state = torch.zeros((num_clips + 1, cols), dtype=torch.int64, device=device)
        self._epoch_work = torch.empty((-(-num_clips // CHUNK), chunk_words), dtype=torch.int64, device=device)
        self._out = torch.empty(out_words, dtype=torch.int64, device=device)

    def state(self):
        """the (num_clips + 1, cols) int64 tensor (records, then the header row), for a collective"""
        return self._state

    def table(self):
        """the (num_clips, cols) records, a view of the state"""
        return self._state[:self.num_clips]

    def reset(self):
        self._state.zero_()

    def _stream(self):
        return stream(self.device)

    def _poses(self, x):
        return check_poses(x, self.K, self.device, self.NOUN, self.NO_GPU)

    def _step(self, pred, gt, clip_index, multiple, gt_optional=False):
        return check_step(pred, gt, clip_index, multiple, self.K, self.device, self.NOUN, self.NO_GPU, gt_optional)

    def result(self, gathered=None):
        """-> the named epoch values (``epoch_values``) over this accumulator's table, or over ``gathered``: a (ranks, num_clips + 1, cols)
        int64 tensor (or a list of such states / accumulators), one entry per rank; the lowest rank that has seen a clip gives its record"""
        return self.epoch_values(self.result_words(gathered))

    def table_pointers(self, gathered=None):
        """-> (a host array of table pointers, their number, the tensors that own them): this accumulator's state, or the checked ``gathered``"""
        import ctypes as C
        import torch
        if gathered is None:
            blocks = [self._state]
        elif torch.is_tensor(gathered):
            blocks = list(gathered.unbind(0)) if gathered.ndim == 3 else [gathered]
        else:
            blocks = [g.state() if isinstance(g, RecordTable) else g for g in gathered]
        if not 1 <= len(blocks) <= MAX_TABLES:
            raise ValueError('%d tables; the epoch stage takes 1 to %d' % (len(blocks), MAX_TABLES))
        for b in blocks:
            if b.dtype != torch.int64 or tuple(b.shape) != tuple(self._state.shape) or b.device != self.device or not b.is_contiguous():
                raise ValueError('a gathered state must be a contiguous %s int64 tensor on %s' % (tuple(self._state.shape), self.device))
        return (C.c_void_p * len(blocks))(*[b.data_ptr() for b in blocks]), len(blocks), blocks

    def result_words(self, gathered=None):
        """the words of the epoch vector as a numpy int64 array (float64 words viewed as int64)"""
        import torch
        from . import _lib
        ptrs, ranks, _keep = self.table_pointers(gathered)
        with torch.cuda.device(self.device):
            _lib.check(self._launch_epoch(ptrs, ranks, self._stream()))
            return self._out.cpu().numpy()  # (same stream: ordered after the kernels, and the one wait of an accumulator)
