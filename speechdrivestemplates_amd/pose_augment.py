"""Pose augmentation inside the train step: a left/right mirror, a uniform scale and an in-plane rotation about the neck
(TRAIN.POSE_AUGMENT).  The audio half is augment.py (TRAIN.AUGMENT; section 25); this module shares its generator.

Everything random is ONE block of Philox4x32-10 (``augment.philox4x32``) per clip, with the key (SEED low 32 bits, SEED high 32 bits) and
the counter (0, purpose 2, clip index low 32 bits, step low 32 bits -- 0 with PER_CLIP), so what a clip looks like depends on
(seed, step, clip) only -- not on the rank, the clip's row in the batch or the batch size.  Purposes 0 and 1 belong to the audio augmenter.

    mirror    on iff (w0 >> 8) < floor(MIRROR_PROB 2^24)
    scale     is = w1 >> 24, s = 1 + (-P + 2 P (is + 0.5) / 256) / 100 from a 256-entry float64 table (P = SCALE_PCT)
    rotation  ir = w2 >> 24, a = -R + 2 R (ir + 0.5) / 256 degrees, (c, sn) = (cos a, sin a) from a 256-entry float64 table (R = ROT_DEG)
    w3        unused

For keypoint k with the mirror partner m = perm[k] (m = k without the mirror), per frame, in float64 on values converted exactly from
float32, every operation rounded on its own:

    dx = n_x[m] std_x[m] + mean_x[m],  dy likewise;  dx = -dx under mirror
    (rx, ry) = (s dx, s dy) when c == 1 and sn == 0 (no rotation is formed: a NaN in one coordinate stays in it), else
    (rx, ry) = (s (c dx - sn dy), s (sn dx + c dy))
    out_x[k] = float32((rx - mean_x[k]) / std_x[k]),  out_y[k] likewise

A clip whose transformation is the identity (no mirror, s == 1, c == 1, sn == 0 -- every clip when MIRROR_PROB, SCALE_PCT and ROT_DEG are 0)
gets its input's bits: signed zeros, subnormals and NaN payloads included.  The confidences travel with their keypoints:
score_out[k] = score[m], as bits.  The effective clip index is clip + N mirror: a mirrored clip is another motion and trains its own row of
the (2 N)-row code tables.

The formula is the same on hierarchical offsets and on neck-relative global poses: the transformation x -> s R M x is linear, and perm maps
every part root to a part root (6 <-> 3, 39 to itself), so the offset of k from its root maps to the offset of perm[k] from ITS root.

Two routes that run the same operations in the same order: ``params_model`` / ``pose_model`` are the contract in numpy; ``augment_poses``
runs csrc/pose_augment.hip on CUDA tensors.  There is no CPU fallback.  ``PoseAugmenter`` is what the pipelines' forward passes use.

    python -m speechdrivestemplates_amd.pose_augment CLIP.npz OUT.npz --speaker NAME --step N --clip I [--seed ..] [--mirror-prob ..]
                                                                      [--scale-pct ..] [--rot-deg ..] [--per-clip] [--n-clips ..]
                                                                      [--stat-file ..] [--global]

writes the poses the model would be trained on for CLIP.npz as clip I at step N (on the GPU) and prints the record.
"""
import math

import numpy as np

from .augment import _dev_tensor, _index_tensors, _key, _ptr, philox4x32

REC_COLS = 8  # words of a clip's record (SDT_POSE_AUGMENT_REC_COLS)
MIRROR, IS, IR, S, C, SN, EFF, IDENTITY = range(8)
PURPOSE = 2
MAX_K, MAX_B, MAX_T, MAX_CLIPS = 128, 65535, 1 << 24, 1 << 40
_NO_GPU = 'the pose augmentation is computed on the GPU (csrc/pose_augment.hip); there is no CPU fallback (pose_model is the numpy contract)'
NEUTRAL = {'seed': 0, 'mirror_prob': 0.0, 'scale_pct': 0.0, 'rot_deg': 0.0, 'per_clip': False}


def options(**kw):
    """the options dict ``config.check_pose_augment`` returns, from keywords (the rest neutral)"""
    unknown = set(kw) - set(NEUTRAL)
    if unknown:
        raise ValueError('unknown pose augmentation option(s): %s' % ', '.join(sorted(unknown)))
    out = dict(NEUTRAL, **kw)
    out['seed'], out['per_clip'] = int(out['seed']), bool(out['per_clip'])
    for name, hi in (('mirror_prob', 1.0), ('scale_pct', 50.0), ('rot_deg', 45.0)):
        out[name] = float(out[name])
        if not 0.0 <= out[name] <= hi:
            raise ValueError('%s must lie in [0, %g], got %r' % (name, hi, out[name]))
    if not 0 <= out['seed'] < 1 << 64:
        raise ValueError('the seed must lie in [0, 2^64), got %r' % (out['seed'],))
    return out


def mirrors(opts):
    """does any draw mirror a clip: the per-clip code tables then have 2 N rows"""
    return opts is not None and mirror_prob24(opts) > 0


def table_rows(opts, n_clips):
    """rows of a per-clip code table over ``n_clips`` training clips"""
    return 2 * int(n_clips) if mirrors(opts) else int(n_clips)


def check_table_rows(what, rows, opts, n_clips):
    """a loaded per-clip table against the training set: raises with both counts"""
    want = table_rows(opts, n_clips)
    if int(rows) != want:
        raise RuntimeError('%s has %d rows but %s' % (what, rows, (
            'TRAIN.POSE_AUGMENT.MIRROR_PROB > 0 needs %d (2 x %d clips: a mirrored clip i trains row %d + i)' % (want, n_clips, n_clips)
            if mirrors(opts) else 'the training set has %d clips (a table of %d rows comes from a run with TRAIN.POSE_AUGMENT.MIRROR_PROB > 0)'
            % (want, 2 * want))))


# ---- the numpy contract models ---------------------------------------------------------------------------------------------------------------
def scale_table(scale_pct):
    """256 float64 factors: level i is 1 + (-P + 2 P (i + 0.5) / 256) / 100 (ones at P = 0)"""
    P = float(scale_pct)
    return np.array([1.0 + (-P + 2.0 * P * (i + 0.5) / 256.0) / 100.0 for i in range(256)], dtype=np.float64)


def rot_table(rot_deg):
    """(256, 2) float64 (cos, sin): level i is -R + 2 R (i + 0.5) / 256 degrees ((1, 0) at R = 0)"""
    R = float(rot_deg)
    a = [math.radians(-R + 2.0 * R * (i + 0.5) / 256.0) for i in range(256)]
    return np.array([[math.cos(v), math.sin(v) + 0.0] for v in a], dtype=np.float64)


def mirror_prob24(opts):
    """the mirror is on iff (w0 >> 8) < this"""
    return int(math.floor(float(opts['mirror_prob']) * (1 << 24)))


def default_perm(K):
    """the mirror table of the 121-keypoint skeleton (the only one there is)"""
    if K != 121:
        raise ValueError('the mirror table is that of the 121-keypoint skeleton; give perm for K = %d' % K)
    from .core.datasets.gesture_dataset import PoseTransforms
    return PoseTransforms.mirror_table()


def check_perm(perm, K):
    perm = [int(v) for v in perm]
    if len(perm) != K or sorted(perm) != list(range(K)):
        raise ValueError('perm must be a permutation of 0 .. %d' % (K - 1))
    return perm


def params_model(opts, clip, step, n_clips=1, words=None):
    """one clip's parameters: {'mirror', 'is', 'ir', 's', 'c', 'sn', 'eff', 'identity'}.  ``words``: the four words of the block in place
    of the Philox draw (the tests' extremes)"""
    if words is None:
        counter = [0, PURPOSE, int(clip) & 0xffffffff, 0 if opts['per_clip'] else int(step) & 0xffffffff]
        words = philox4x32(counter, _key(opts['seed']))
    w = [int(v) & 0xffffffff for v in words]
    mirror = int((w[0] >> 8) < mirror_prob24(opts))
    i_s, i_r = w[1] >> 24, w[2] >> 24
    s = scale_table(opts['scale_pct'])[i_s]
    c, sn = rot_table(opts['rot_deg'])[i_r]
    return {'mirror': mirror, 'is': i_s, 'ir': i_r, 's': s, 'c': c, 'sn': sn, 'eff': int(clip) + int(n_clips) * mirror,
            'identity': int(not mirror and s == 1.0 and c == 1.0 and sn == 0.0)}


def _record(p):
    r = np.zeros(REC_COLS, dtype=np.int64)
    r[MIRROR], r[IS], r[IR], r[EFF], r[IDENTITY] = p['mirror'], p['is'], p['ir'], p['eff'], p['identity']
    r[S], r[C], r[SN] = (np.float64(p[k]).view(np.int64) for k in ('s', 'c', 'sn'))
    return r


def coords_model(d, p, perm):
    """the transformation on de-normalised coordinates d (..., 2, K) float64 (hierarchical offsets or neck-relative global positions alike):
    keypoint k takes its partner's, mirrored, rotated and scaled"""
    d = np.asarray(d, dtype=np.float64)
    m = np.asarray(perm, dtype=np.int64) if p['mirror'] else np.arange(d.shape[-1])
    with np.errstate(all='ignore'):
        dx, dy = d[..., 0, :][..., m], d[..., 1, :][..., m]
        if p['mirror']:
            dx = -dx
        s, c, sn = np.float64(p['s']), np.float64(p['c']), np.float64(p['sn'])
        if c == 1.0 and sn == 0.0:
            rx, ry = s * dx, s * dy
        else:
            rx, ry = s * (c * dx - sn * dy), s * (sn * dx + c * dy)
        return np.stack([rx, ry], axis=-2)


def transform_model(n, mean, std, p, perm):
    """one clip: n (T, 2, K) float32, mean / std (2 K,) float64, p from ``params_model`` -> (T, 2, K) float32"""
    n = np.asarray(n, dtype=np.float32)
    if p['identity']:
        return n.copy()
    K = n.shape[-1]
    mean, std = np.asarray(mean, dtype=np.float64).reshape(2, K), np.asarray(std, dtype=np.float64).reshape(2, K)
    with np.errstate(all='ignore'):
        return ((coords_model(n.astype(np.float64) * std + mean, p, perm) - mean) / std).astype(np.float32)


def pose_model(poses, score, mean, std, clip_index, step, opts, n_clips, perm=None):
    """(B, T, 2, K) float32 poses, ``score`` the same shape or None, mean / std (B, 2 K) float64 -> (poses_out, score_out or None,
    eff_index (B,) int64, records (B, 8) int64): sdt_pose_augment_f32"""
    poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float32))
    B, T, _, K = poses.shape
    perm = check_perm(default_perm(K) if perm is None else perm, K)
    clip_index = np.asarray(clip_index, dtype=np.int64).reshape(B)
    mean, std = np.asarray(mean, dtype=np.float64).reshape(B, 2 * K), np.asarray(std, dtype=np.float64).reshape(B, 2 * K)
    out, rec = np.empty_like(poses), np.zeros((B, REC_COLS), dtype=np.int64)
    score_out = None if score is None else np.array(score, dtype=np.float32, copy=True)
    for b in range(B):
        p = params_model(opts, clip_index[b], step, n_clips)
        rec[b] = _record(p)
        out[b] = transform_model(poses[b], mean[b], std[b], p, perm)
        if score is not None and p['mirror']:
            score_out[b] = np.asarray(score, dtype=np.float32)[b][:, :, perm]
    return out, score_out, rec[:, EFF].copy(), rec


def record_values(rec):
    """one clip's 8 words -> a dict with names"""
    rec = np.ascontiguousarray(np.asarray(rec, dtype=np.int64).reshape(REC_COLS))
    f = rec.view(np.float64)
    return {'mirror': int(rec[MIRROR]), 'is': int(rec[IS]), 'ir': int(rec[IR]), 's': float(f[S]), 'c': float(f[C]), 'sn': float(f[SN]),
            'eff': int(rec[EFF]), 'identity': int(rec[IDENTITY])}


def describe(rec):
    """one line for the log"""
    v = record_values(rec)
    if v['identity']:
        return 'unchanged, code row %d' % v['eff']
    return '%s, scale %.6f (level %d), rotation %+.4f degrees (level %d), code row %d' % (
        'mirrored' if v['mirror'] else 'not mirrored', v['s'], v['is'], math.degrees(math.atan2(v['sn'], v['c'])), v['ir'], v['eff'])


# ---- the device route (csrc/pose_augment.hip) --------------------------------------------------------------------------------------------------
def device_tables(opts, device):
    """(scale table (256,), rotation table (256, 2)) float64 on ``device``: uploaded once by whoever holds them"""
    import torch
    return torch.from_numpy(scale_table(opts['scale_pct'])).to(device), torch.from_numpy(rot_table(opts['rot_deg'])).to(device)


def perm_array(perm):
    """the host array of K int32 the C entry point takes"""
    import ctypes as C
    return (C.c_int32 * len(perm))(*perm)


def _stat_tensor(x, B, K, what, device):
    import torch
    x = _dev_tensor(x, torch.float64, what)
    if tuple(x.shape) != (B, 2 * K) or x.device != device:
        raise ValueError('%s must be (%d, %d) float64 on %s, got %s' % (what, B, 2 * K, device, tuple(x.shape)))
    return x


def augment_poses(poses, score, mean, std, clip_index, step, opts, n_clips, perm=None, tables=None, rec=None, out=None, score_out=None):
    """(B, T, 2, K) float32 poses on the GPU, ``score`` the same shape or None, mean / std (B, 2 K) float64, clip_index (B,) and step (1,)
    int64 on the GPU -> (a new poses tensor, a new score tensor or None, eff_index (B,) int64, the records (B, 8) int64).  ``tables``:
    ``device_tables`` kept by the caller; ``perm``: the mirror table (a list, or a ``perm_array``; default: the 121-keypoint skeleton's);
    ``rec`` / ``out`` / ``score_out``: buffers to write into (contiguous, not the inputs)"""
    import torch
    from . import _lib
    poses = _dev_tensor(poses, torch.float32, 'the poses')
    if poses.ndim != 4 or poses.shape[2] != 2 or not 1 <= poses.shape[0] <= MAX_B or not 1 <= poses.shape[1] <= MAX_T \
            or not 1 <= poses.shape[3] <= MAX_K:
        raise ValueError('the poses must be (B, T, 2, K) with B in [1, %d], T in [1, 2^24] and K in [1, %d], got %s'
                         % (MAX_B, MAX_K, tuple(poses.shape)))
    B, T, _, K = (int(v) for v in poses.shape)
    if not 1 <= int(n_clips) <= MAX_CLIPS:
        raise ValueError('n_clips must lie in [1, 2^40], got %r' % (n_clips,))
    dev = poses.device
    if score is not None:
        score = _dev_tensor(score, torch.float32, 'the score')
        if score.shape != poses.shape or score.device != dev:
            raise ValueError('the score must have the shape of the poses %s on %s, got %s' % (tuple(poses.shape), dev, tuple(score.shape)))
    mean, std = _stat_tensor(mean, B, K, 'mean', dev), _stat_tensor(std, B, K, 'std', dev)
    clip_index, step = _index_tensors(clip_index, step, B, dev)
    if perm is None or isinstance(perm, (list, tuple)):
        perm = perm_array(check_perm(default_perm(K) if perm is None else perm, K))
    if len(perm) != K:
        raise ValueError('perm has %d entries for K = %d' % (len(perm), K))
    scale, rot = device_tables(opts, dev) if tables is None else tables
    if rec is None:
        rec = torch.empty((B, REC_COLS), dtype=torch.int64, device=dev)
    out = torch.empty_like(poses) if out is None else out
    if score is not None and score_out is None:
        score_out = torch.empty_like(score)
    for t, what in ((out, 'out'), (score_out, 'score_out')):
        if t is not None and (t.shape != poses.shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev):
            raise ValueError('%s must be a contiguous float32 tensor of shape %s on %s' % (what, tuple(poses.shape), dev))
    eff = torch.empty(B, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().sdt_pose_augment_f32(
            _ptr(poses), None if score is None else _ptr(score), _ptr(mean), _ptr(std), B, T, K, _ptr(clip_index), _ptr(step), int(n_clips),
            int(opts['seed']), mirror_prob24(opts), int(bool(opts['per_clip'])), perm, _ptr(scale), _ptr(rot), _ptr(out),
            None if score is None else _ptr(score_out), _ptr(eff), _ptr(rec), torch.cuda.current_stream(dev).cuda_stream))
    return out, (score_out if score is not None else None), eff, rec


class PoseAugmenter:
    """the tables (uploaded once), the mirror table and the record buffers of one device.  A record buffer is allocated at the first call of
    a (B, T) -- in the eager steps that precede a graph capture; the outputs are new tensors of every call, as the audio augmenter's are.
    ``record`` is the (B, 8) int64 record of the last call, on the device."""

    def __init__(self, opts, device, n_clips, perm=None):
        import torch
        self.opts, self.device, self.n_clips = opts, torch.device(device), int(n_clips)
        self.tables = device_tables(opts, self.device)
        self._perm = None if perm is None else perm_array(check_perm(perm, len(perm)))
        self._bufs = {}
        self.record = None

    def __call__(self, poses, score, mean, std, clip_index, step):
        """-> (poses, score or None, eff_index)"""
        import torch
        B, T, K = int(poses.shape[0]), int(poses.shape[1]), int(poses.shape[3])
        if self._perm is None:
            self._perm = perm_array(check_perm(default_perm(K), K))
        if (B, T) not in self._bufs:
            self._bufs[(B, T)] = torch.zeros((B, REC_COLS), dtype=torch.int64, device=self.device)
        out, score_out, eff, self.record = augment_poses(poses, score, mean, std, clip_index, step, self.opts, self.n_clips, self._perm,
                                                         self.tables, self._bufs[(B, T)])
        return out, score_out, eff


def batch_poses(aug, batch, dev, want_score):
    """what both pipelines' training forward passes do with a batch: -> (poses, score or None, eff_index) on ``dev``"""
    import torch
    if 'aug_step' not in batch:
        raise KeyError("TRAIN.POSE_AUGMENT.ENABLE is set but the batch has no 'aug_step' (an int64 tensor of shape (1,) with the global "
                       "step; train_step adds it): the augmentation depends on (seed, step, clip)")
    stat = batch['speaker_stat']
    mean, std = (torch.as_tensor(stat[k]).to(dev, non_blocking=True).double() for k in ('mean', 'std'))
    poses = batch['poses'].to(dev, non_blocking=True).float()
    score = batch['poses_score'].to(dev, non_blocking=True).float() if want_score else None
    B = poses.shape[0]
    if mean.dim() == 1:  # one table for the whole batch
        mean, std = mean.expand(B, -1), std.expand(B, -1)
    return aug(poses, score, mean.reshape(B, -1), std.reshape(B, -1), batch['clip_index'].to(dev, non_blocking=True).long().reshape(-1),
               batch['aug_step'].to(dev, non_blocking=True))


# ---- command line ------------------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='write the poses the model would be trained on for a clip npz as clip I at train step N, and '
                                             'print the record')
    ap.add_argument('inp', metavar='CLIP.npz', help="a clip file with 'pose' (frames, 3, 137): x, y, confidence in pixels")
    ap.add_argument('out', metavar='OUT.npz')
    ap.add_argument('--speaker', required=True, metavar='NAME', help='whose statistics normalise the poses')
    ap.add_argument('--step', type=int, required=True, metavar='N', help='the global train step')
    ap.add_argument('--clip', type=int, required=True, metavar='I', help='the clip index')
    ap.add_argument('--seed', type=int, default=0, help='TRAIN.POSE_AUGMENT.SEED')
    ap.add_argument('--mirror-prob', type=float, default=0.0, help='TRAIN.POSE_AUGMENT.MIRROR_PROB, 0 .. 1')
    ap.add_argument('--scale-pct', type=float, default=0.0, help='TRAIN.POSE_AUGMENT.SCALE_PCT, 0 .. 50')
    ap.add_argument('--rot-deg', type=float, default=0.0, help='TRAIN.POSE_AUGMENT.ROT_DEG, 0 .. 45')
    ap.add_argument('--per-clip', action='store_true', help='TRAIN.POSE_AUGMENT.PER_CLIP')
    ap.add_argument('--n-clips', type=int, default=None, metavar='N', help='clips of the training set (default: I + 1)')
    ap.add_argument('--stat-file', default=None, help="DATASET.SPEAKER_STAT_FILE: an npz of the speaker's statistics")
    ap.add_argument('--global', dest='hierarchical', action='store_false', help='DATASET.HIERARCHICAL_POSE False')
    a = ap.parse_args(argv)
    if a.step < 0 or a.clip < 0 or not 0 <= a.seed < 1 << 64:
        ap.error('--step and --clip must be >= 0 and --seed in [0, 2^64)')
    if not 0 <= a.mirror_prob <= 1 or not 0 <= a.scale_pct <= 50 or not 0 <= a.rot_deg <= 45:
        ap.error('--mirror-prob takes 0 .. 1, --scale-pct 0 .. 50, --rot-deg 0 .. 45')
    if a.n_clips is None:
        a.n_clips = a.clip + 1
    if not a.clip < a.n_clips <= MAX_CLIPS:
        ap.error('--n-clips must lie in (--clip, 2^40]')
    return a


def main(argv=None):
    a = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    from .config import get_cfg_defaults
    from .core.datasets import gesture_dataset as gd
    cfg = get_cfg_defaults()
    cfg.merge_from_list(['DATASET.HIERARCHICAL_POSE', a.hierarchical, 'DATASET.SPEAKER', a.speaker, 'DATASET.SPEAKER_STAT_FILE', a.stat_file])
    gd.register_configured_speaker_stats(cfg)
    ds = gd.GestureDataset(cfg=cfg, speaker=a.speaker)
    p = torch.Tensor(np.load(a.inp)['pose'][:cfg.DATASET.NUM_FRAMES, ...])  # GestureDataset.__getitem__
    p = ds.absolute_to_relative(ds.remove_unuesd_kp(p))
    if a.hierarchical:
        p = ds.global_to_parted(p)
    stat = ds.get_speaker_stat(a.speaker, 121, parted=a.hierarchical)
    poses, score = ds.normalize_poses(p[:, :2, :], stat), p[:, 2:, :].repeat(1, 2, 1)
    opts = options(seed=a.seed, mirror_prob=a.mirror_prob, scale_pct=a.scale_pct, rot_deg=a.rot_deg, per_clip=a.per_clip)
    dev = torch.device('cuda', torch.cuda.current_device())
    to64 = lambda v: torch.tensor(np.asarray(v, dtype=np.float64)[None]).to(dev)  # noqa: E731
    out, score_out, eff, rec = augment_poses(poses[None].contiguous().to(dev), score[None].contiguous().to(dev), to64(stat['mean']),
                                             to64(stat['std']), torch.tensor([a.clip], dtype=torch.int64, device=dev),
                                             torch.tensor([a.step], dtype=torch.int64, device=dev), opts, a.n_clips)
    rec = rec.cpu().numpy()[0]
    print('clip %d at step %d: %s' % (a.clip, a.step, describe(rec)))
    np.savez(a.out, poses=out.cpu().numpy()[0], poses_score=score_out.cpu().numpy()[0], eff_index=eff.cpu().numpy()[0], record=rec)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
