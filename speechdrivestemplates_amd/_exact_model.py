"""The numpy model helpers of the bit-exact metric contracts (DESIGN.md sections 22-25), shared by clip_metrics, sync_metrics, long_demo and
augment: the same operations in the same order as the lane helpers of csrc/exact_lanes.h, and the limits and the part table they share."""
import numpy as np

PARTS = ('all', 'body', 'face', 'hands')
MAX_K, MAX_COPIES, MAX_TABLES = 128, 16, 64
WAVE, LANES = 64, 128  # lanes of one wave; of the two waves that hold a frame's keypoints, one lane per keypoint
assert LANES == MAX_K


def check_parts(parts, K):
    """-> (K,) uint8 array; the default for K = 121 is PoseTransforms.part_table()"""
    if parts is None:
        if K != 121:
            raise ValueError('a part table is needed for K = %d keypoints (the default is the 121-keypoint layout)' % K)
        from .core.datasets.gesture_dataset import PoseTransforms
        parts = PoseTransforms.part_table()
    parts = np.asarray(parts)
    if parts.shape != (K,) or not np.isin(parts, (0, 1, 2)).all():
        raise ValueError('the part table must hold K = %d values in {0, 1, 2}' % K)
    return parts.astype(np.uint8)


def part_sizes(parts):
    """(K, body, face, hands) keypoint counts"""
    parts = np.asarray(parts)
    return (int(parts.size),) + tuple(int((parts == p).sum()) for p in range(3))


def _butterfly_wave(v):
    """the xor butterfly 32, 16, 8, 4, 2, 1 along the last axis of 64 lanes -> lane 0's value (every lane holds the same bits)"""
    idx = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def _butterfly(v):
    """(..., 128) lane values -> what every lane of the kernel ends with: the butterfly inside each 64-lane wave, then wave 0 + wave 1"""
    waves = _butterfly_wave(v.reshape(v.shape[:-1] + (2, WAVE)))
    return waves[..., 0] + waves[..., 1]


def _part_sums(term, parts):
    """(..., K) per-keypoint terms -> (..., 4): per part the lanes' values (+0.0 outside the part and for k >= K) through the butterfly"""
    K = term.shape[-1]
    lanes = np.zeros(term.shape[:-1] + (4, LANES))
    for p in range(4):
        lanes[..., p, :K] = term if p == 0 else np.where(parts == p - 1, term, 0.0)
    return _butterfly(lanes)


def _norm2(x, y):
    return x * x + y * y  # (numpy rounds each operation on its own)


def _ordered_sum(x, axis):
    """serial sum along ``axis`` starting from +0.0"""
    x = np.moveaxis(x, axis, 0)
    s = np.zeros(x.shape[1:])
    for i in range(x.shape[0]):
        s = s + x[i]
    return s


def _quotient(x, n):
    return np.float64(0.0) if n == 0 else np.float64(x) / np.float64(n)
