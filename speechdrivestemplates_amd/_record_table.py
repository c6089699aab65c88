"""The record-table protocol of the per-clip validation metrics, shared by clip_metrics, sync_metrics and motion_dist (DESIGN.md section 22 states it;
csrc/record_table.h is the device side).

A table is a (num_clips + 1, cols) int64 tensor: one record per clip of the validation set, then a header row whose word 0 counts the clip
indices outside the table.  Under data parallelism there is one table per rank; per clip the lowest rank whose record has its seen word set
gives the record.  The epoch sum runs over chunks of 64 clips in index order, then over the chunk partials in order.  The word layouts, what
each word adds up and the final divisions belong to the families."""
import numpy as np

from ._exact_model import MAX_TABLES

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


# ---- the device route --------------------------------------------------------------------------------------------------------------------------
class RecordTable:
    """The state of an accumulator: a table of ``num_clips`` records of ``cols`` words on ``device`` (a torch.device with an index), the
    workspace of the epoch stage and its output vector.  A subclass keeps its ``add``, launches its epoch stage in ``_launch_epoch(ptrs,
    ranks, stream)`` (-> the status of the C call) and names the words of the epoch vector in ``epoch_values(words)``."""

    def __init__(self, num_clips, device, cols, chunk_words, out_words):
        import torch
        self.num_clips, self.device = num_clips, device
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

    def result(self, gathered=None):
        """-> the named epoch values (``epoch_values``) over this accumulator's table, or over ``gathered``: a (ranks, num_clips + 1, cols)
        int64 tensor (or a list of such states / accumulators), one entry per rank; the lowest rank that has seen a clip gives its record"""
        return self.epoch_values(self.result_words(gathered))

    def result_words(self, gathered=None):
        """the words of the epoch vector as a numpy int64 array (float64 words viewed as int64)"""
        import ctypes as C
        import torch
        from . import _lib
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
        ptrs = (C.c_void_p * len(blocks))(*[b.data_ptr() for b in blocks])
        with torch.cuda.device(self.device):
            _lib.check(self._launch_epoch(ptrs, len(blocks), torch.cuda.current_stream(self.device).cuda_stream))
            return self._out.cpu().numpy()  # (same stream: ordered after the kernels, and the one wait of an accumulator)
