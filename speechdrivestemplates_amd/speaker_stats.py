"""A custom speaker's normalisation statistics, computed on the GPU from its clips (csrc/speaker_stats.hip): the reference's
data_preprocess/4_1_calculate_mean_std.py (-m parted and -m global) followed by 4_2_parse_mean_std_npz.py, written in the
npz layout ``load_speaker_stats`` reads instead of being pasted into core/datasets/speakers_stat.py.

Contract: the ``dataset == 'train'`` rows of ``<root>/<speaker>/<csv>`` in csv order, frames
[0, NUM_FRAMES) of each clip's ``pose``, split into ``num_chunks`` chunks of N // num_chunks rows (the remainder is dropped,
like cal_mean_std's ``stride``).  parted mean / std and global std are the reference's bits; the reference's global mean
raises on its first clip (4_1:26-27 compares a 2-vector), so it is computed with the component-wise test of cal_std_global.

    python -m speechdrivestemplates_amd.speaker_stats --root DIR --speaker NAME (--scale-factor F | --scale-like NAME)
"""
import argparse
import ctypes as C
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib

KP = 137
DELETE_137 = [1] + list(range(8, 15)) + list(range(17, 25))  # 4_2_parse_mean_std_npz.py:16
KEPT_137 = [k for k in range(KP) if k not in DELETE_137]
MAX_READ_THREADS = 16  # npz decoding threads: a fixed cap, not os.cpu_count(), which counts every CPU of a shared host
DEFAULT_WINDOW = 64
DEFAULT_DEVICE_BUDGET = 8 << 30


def plan_speaker_stats(root_dir, speaker, csv='processed_137.csv', num_chunks=10):
    """-> dict(paths of the training clips in csv order, stride, clips used / dropped, csv path); raises on too few clips"""
    import pandas as pd
    csv_path = os.path.join(root_dir, speaker, csv)
    if not os.path.exists(csv_path):
        raise FileNotFoundError('No csv file: %s' % csv_path)
    if int(num_chunks) < 1:
        raise ValueError('num_chunks must be at least 1, got %r' % (num_chunks,))
    df = pd.read_csv(csv_path)
    fns = list(df[df['dataset'] == 'train']['pose_fn'])
    n = len(fns)
    if n < num_chunks:
        raise ValueError('%s has %d training clips, fewer than num_chunks=%d: every chunk would be empty and the reference would '
                         'write all-zero statistics' % (csv_path, n, num_chunks))
    stride = n // num_chunks
    return {'paths': [os.path.join(root_dir, speaker, fn) for fn in fns], 'stride': stride, 'num_chunks': int(num_chunks),
            'clips_used': stride * num_chunks, 'clips_dropped': n - stride * num_chunks, 'csv': csv_path}


def read_clip_poses(path, num_frames):
    """x / y of frames [0, num_frames) of a clip npz, (num_frames, 2, 137) in the file's dtype (float32 or float64)"""
    with np.load(path) as z:
        pose = z['pose']
    if pose.ndim != 3 or pose.shape[1] < 2 or pose.shape[2] != KP:
        raise ValueError('%s: pose has shape %s, expected (frames, 3, 137)' % (path, pose.shape))
    if pose.shape[0] < num_frames:
        raise ValueError('%s: %d frames, fewer than the %d the statistics use' % (path, pose.shape[0], num_frames))
    if pose.dtype not in (np.float32, np.float64):
        raise ValueError('%s: pose dtype %s (float32 or float64 expected)' % (path, pose.dtype))
    return pose[:num_frames, :2, :]


def _scale_factors(scale_factor, scale_like):
    if (scale_factor is None) == (scale_like is None):
        raise ValueError('give exactly one of scale_factor (a number) or scale_like (a built-in speaker whose factors to copy): '
                         'the factor is not derivable from the clips')
    if scale_factor is not None:
        return float(scale_factor), float(scale_factor)
    from .core.datasets import gesture_dataset as gd
    gd.load_builtin_speaker_stats()
    out = []
    for table in (gd.SPEAKERS_STAT_121_parted, gd.SPEAKERS_STAT_121):
        if scale_like not in table:
            raise KeyError('scale_like=%r: no built-in %s statistics for that speaker'
                           % (scale_like, 'parted' if table is gd.SPEAKERS_STAT_121_parted else 'global'))
        out.append(float(table[scale_like]['scale_factor']))
    return tuple(out)


def _p(t):
    return C.c_void_p(t.data_ptr())


class _Reader:
    """decodes the windows of clips [j0, j0 + w) of every chunk into pinned staging buffers on a thread pool (two buffers, so
    the host fills one while the GPU copies / reads the other)"""

    def __init__(self, plan, num_frames, dtype, window):
        self.plan, self.F, self.dtype = plan, num_frames, dtype
        shape = (plan['num_chunks'], window, num_frames, 2, KP)
        self.bufs = [torch.empty(shape, dtype=dtype).pin_memory() for _ in range(2)]
        self.done = [None, None]  # the event after the last copy out of each buffer
        self.pool = ThreadPoolExecutor(max_workers=min(MAX_READ_THREADS, plan['num_chunks'] * window))
        self.np_dtype = np.float32 if dtype == torch.float32 else np.float64

    def fill(self, slot, j0, w):
        if self.done[slot] is not None:
            self.done[slot].synchronize()
        dst = self.bufs[slot].numpy()
        stride, paths = self.plan['stride'], self.plan['paths']

        def one(cj):
            c, j = divmod(cj, w)
            path = paths[c * stride + j0 + j]
            p = read_clip_poses(path, self.F)
            if p.dtype != self.np_dtype:
                raise ValueError('%s: pose dtype %s, but the first training clip is %s (one dtype per speaker)'
                                 % (path, p.dtype, self.np_dtype.__name__))
            dst[c, j] = p
        for f in [self.pool.submit(one, cj) for cj in range(self.plan['num_chunks'] * w)]:
            f.result()
        return self.bufs[slot]

    def close(self):
        self.pool.shutdown()


def compute_speaker_stats(root_dir, speaker, cfg=None, csv='processed_137.csv', num_chunks=10, scale_factor=None, scale_like=None,
                          allow_zero_std=False, device='cuda', window=DEFAULT_WINDOW, device_budget_bytes=DEFAULT_DEVICE_BUDGET):
    """-> {'parted': {'mean' (242,), 'std' (242,), 'scale_factor'}, 'global': {...}, 'mean137' / 'std137' (2 modes, 2, 137),
    'counts' (2 modes, 137) int64, 'clips_used', 'clips_dropped', 'num_chunks', 'num_frames', 'csv', 'timing'}.
    Modes are ordered parted, global.  Decoded clips stay on the device up to ``device_budget_bytes``; past it, pass 2 reads the
    files again (the reference's way); both give the same bits."""
    F = int(cfg.DATASET.NUM_FRAMES) if cfg is not None else 64
    scales = _scale_factors(scale_factor, scale_like)
    plan = plan_speaker_stats(root_dir, speaker, csv, num_chunks)
    Cn, stride = plan['num_chunks'], plan['stride']
    first = read_clip_poses(plan['paths'][0], F)  # the speaker's dtype (and a short / malformed first clip fails before any GPU work)
    dtype = torch.float32 if first.dtype == np.float32 else torch.float64
    w_max = max(1, min(int(window), stride))
    lib = _lib.load()
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('speaker statistics are computed on the GPU (csrc/speaker_stats.hip); there is no CPU fallback')
    t_start = time.perf_counter()
    clip_elems = F * 2 * KP
    esize = 4 if dtype == torch.float32 else 8
    resident = Cn * stride * clip_elems * esize <= device_budget_bytes
    state_bytes = lib.sdt_speaker_stats_state_bytes(Cn, F)
    if state_bytes <= 0:
        raise ValueError('unsupported chunk / frame count (%d, %d)' % (Cn, F))
    state = torch.empty(state_bytes // 8, dtype=torch.float64, device=dev)
    out137 = torch.empty((2, 2, 2, KP), dtype=torch.float64, device=dev)  # [pass][mode][coord][k]
    out242 = torch.empty((2, 2, 242), dtype=torch.float64, device=dev)
    counts = torch.empty((2, 2, KP), dtype=torch.float64, device=dev)
    first_bad = torch.empty((2, KP), dtype=torch.int64, device=dev)
    flags = torch.empty((2, 2, KP), dtype=torch.int32, device=dev)
    store = torch.empty((Cn, stride, F, 2, KP), dtype=dtype, device=dev) if resident else None
    wbuf = None if resident else torch.empty((Cn, w_max, F, 2, KP), dtype=dtype, device=dev)
    st = torch.cuda.current_stream(dev)
    raw = st.cuda_stream
    reader = _Reader(plan, F, dtype, w_max)
    t_read = [0.0]
    kernel_ms = [0.0, 0.0]

    def accumulate(pss, buf, offset, pitch, w, j0):
        """clips [j0, j0 + w) of every chunk, the first of chunk 0 at element ``offset`` of ``buf``"""
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(st)
        ptr = C.c_void_p(buf.data_ptr() + offset * esize)
        _lib.check(lib.sdt_speaker_stats_accumulate(pss, esize, ptr, buf.numel() - offset, pitch, Cn, F, w, j0, stride,
                                                    _p(out137[0]) if pss == 2 else None, _p(state), state_bytes, raw))
        ev1.record(st)
        return ev0, ev1

    def stream_pass(pss):
        timings = []
        for slot, j0 in enumerate(range(0, stride, w_max)):
            w = min(w_max, stride - j0)
            t0 = time.perf_counter()
            host = reader.fill(slot % 2, j0, w)
            t_read[0] += time.perf_counter() - t0
            with torch.cuda.stream(st):
                if resident:
                    for c in range(Cn):
                        store[c, j0:j0 + w].copy_(host[c, :w], non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(st)
                    reader.done[slot % 2] = ev
                    timings.append(accumulate(pss, store, j0 * clip_elems, stride * clip_elems, w, j0))
                else:
                    wbuf[:, :w].copy_(host[:, :w], non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(st)
                    reader.done[slot % 2] = ev
                    timings.append(accumulate(pss, wbuf, 0, w_max * clip_elems, w, j0))
        return timings

    def finalize(pss):
        _lib.check(lib.sdt_speaker_stats_finalize(pss, _p(state), state_bytes, Cn, F, _p(out137[pss - 1]), _p(out242[pss - 1]),
                                                  _p(counts[pss - 1]), _p(first_bad[pss - 1]), _p(flags[pss - 1]), raw))

    try:
        tm = stream_pass(1)
        finalize(1)
        torch.cuda.synchronize(dev)
        kernel_ms[0] = sum(a.elapsed_time(b) for a, b in tm)
        bad = first_bad[0].cpu().numpy()
        if (bad > 0).any():
            row = int(bad[bad > 0].min()) - 1  # c * stride + j: the csv position among the training rows
            raise ValueError('%s: non-finite pose coordinates in frames [0, %d)' % (plan['paths'][row], F))
        if resident:
            tm = [accumulate(2, store, 0, stride * clip_elems, stride, 0)]  # the whole chunk in one launch
        else:
            tm = stream_pass(2)
        finalize(2)
        torch.cuda.synchronize(dev)
        kernel_ms[1] = sum(a.elapsed_time(b) for a, b in tm)
    finally:
        reader.close()
    fl = flags[1].cpu().numpy()
    cnt = counts[1].cpu().numpy().astype(np.int64)
    if (fl & 1).any():
        m, k = np.argwhere(fl & 1)[0]
        raise ValueError('non-finite %s statistics at keypoint %d' % (('parted', 'global')[m], k))
    zero = [(('parted', 'global')[m], int(k)) for m, k in np.argwhere(fl & 2)]
    if zero and not allow_zero_std:
        raise ValueError('zero std at %d kept keypoint(s), normalisation would divide by zero: %s (allow_zero_std=True keeps the '
                         "reference's zeros)" % (len(zero), ', '.join('%s keypoint %d of 137 (%d of 121), %d detections'
                                                                      % (m, k, KEPT_137.index(k), cnt[('parted', 'global').index(m), k])
                                                                      for m, k in zero)))
    t242 = out242.cpu().numpy()
    t137 = out137.cpu().numpy()
    return {'parted': {'mean': t242[0, 0].copy(), 'std': t242[1, 0].copy(), 'scale_factor': scales[0]},
            'global': {'mean': t242[0, 1].copy(), 'std': t242[1, 1].copy(), 'scale_factor': scales[1]},
            'mean137': t137[0], 'std137': t137[1], 'counts': cnt, 'clips_used': plan['clips_used'],
            'clips_dropped': plan['clips_dropped'], 'num_chunks': Cn, 'num_frames': F, 'csv': plan['csv'], 'dtype': str(first.dtype),
            'timing': {'kernel_ms': kernel_ms, 'read_s': t_read[0], 'total_s': time.perf_counter() - t_start, 'resident': resident}}


def save_speaker_stats(path, stats):
    """the keys load_speaker_stats reads ({parted,global}_{mean,std,scale}) plus informational extras"""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    np.savez(path, parted_mean=np.asarray(stats['parted']['mean'], np.float64), parted_std=np.asarray(stats['parted']['std'], np.float64),
             parted_scale=np.float64(stats['parted']['scale_factor']), global_mean=np.asarray(stats['global']['mean'], np.float64),
             global_std=np.asarray(stats['global']['std'], np.float64), global_scale=np.float64(stats['global']['scale_factor']),
             parted_count=np.asarray(stats['counts'][0], np.int64), global_count=np.asarray(stats['counts'][1], np.int64),
             num_chunks=np.int64(stats['num_chunks']), num_frames=np.int64(stats['num_frames']),
             clips_used=np.int64(stats['clips_used']), clips_dropped=np.int64(stats['clips_dropped']), source_csv=np.array(stats['csv']))
    return path


def main(argv=None):
    ap = argparse.ArgumentParser(description="a speaker's pose statistics on the GPU (the reference's 4_1 + 4_2) -> npz for "
                                             "DATASET.SPEAKER_STAT_FILE")
    ap.add_argument('--root', required=True, help='dataset root (DATASET.ROOT_DIR)')
    ap.add_argument('--speaker', required=True)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument('--scale-factor', type=float, help='scale_factor of both tables')
    g.add_argument('--scale-like', help="copy each table's scale_factor from this built-in speaker")
    ap.add_argument('--csv', default='processed_137.csv', help='clip list under <root>/<speaker>/ (4_1 itself reads clips.csv)')
    ap.add_argument('--chunks', type=int, default=10, help="number of chunks (4_1's -np)")
    ap.add_argument('--frames', type=int, default=64, help='frames per clip (DATASET.NUM_FRAMES)')
    ap.add_argument('--out', help='default <root>/<speaker>/speaker_stat_121.npz')
    ap.add_argument('--allow-zero-std', action='store_true', help="keep the reference's zero std of never-detected keypoints")
    a = ap.parse_args(argv)
    from .config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_list(['DATASET.NUM_FRAMES', a.frames])
    stats = compute_speaker_stats(a.root, a.speaker, cfg=cfg, csv=a.csv, num_chunks=a.chunks, scale_factor=a.scale_factor,
                                  scale_like=a.scale_like, allow_zero_std=a.allow_zero_std)
    out = a.out or os.path.join(a.root, a.speaker, 'speaker_stat_121.npz')
    save_speaker_stats(out, stats)
    t = stats['timing']
    print('speaker %s: %d clips used, %d dropped, %d chunks, %s -> %s (%.2f s, %.2f s reading, kernels %.3f / %.3f ms)'
          % (a.speaker, stats['clips_used'], stats['clips_dropped'], stats['num_chunks'], stats['dtype'], out, t['total_s'], t['read_s'],
             t['kernel_ms'][0], t['kernel_ms'][1]))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
