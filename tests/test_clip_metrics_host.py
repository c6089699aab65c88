"""The per-clip validation metrics (speechdrivestemplates_amd/clip_metrics.py) without a GPU: the numpy contract model
against plain formulas, the ties of the PCK comparison, NaN handling, the epoch stage's choice of rank, the config check and the command line.

Bars.  Hit counts are integers and must be equal.  A sum of n non-negative float64 terms computed in any order differs from any other order
by at most (n - 1) 2^-52 relative; the two formulations of one term (sqrt(dx^2 + dy^2) by separately rounded operations here, torch.norm
there) differ by at most 2 ulp: together (n + 2) 2^-52 relative.
"""
import numpy as np
import pytest
import torch

from speechdrivestemplates_amd import clip_metrics as cm
from speechdrivestemplates_amd.config import check_clip_metrics, get_cfg_defaults
from speechdrivestemplates_amd.core.datasets.gesture_dataset import PoseTransforms

SHAPES = [(1, 1, 1), (1, 2, 1), (2, 3, 5), (3, 2, 63), (2, 2, 64), (2, 2, 65), (2, 3, 128), (3, 64, 121), (5, 64, 121)]  # (R, T, K)
ULP = 2.0 ** -52


def part_table(K):
    return PoseTransforms.part_table() if K == 121 else [k % 3 for k in range(K)]


def poses(R, T, K, seed=0):
    """ground truth spread over a few hundred pixels, prediction a few pixels to a few tens of pixels off: PCK lands strictly inside (0, 1)"""
    rng = np.random.Generator(np.random.PCG64(1000 * seed + 7 * R + 3 * T + K))
    gt = rng.uniform(0.0, 400.0, (R, T, 2, K))
    pred = gt + rng.standard_normal((R, T, 2, K)) * rng.uniform(2.0, 60.0, (R, 1, 1, K))
    return pred, gt


def alphas_for(n):
    return [0.1, 0.2, 0.05, 0.5][:n]


def copies_for(R):
    return [m for m in (1, 2, 3, 16) if R % m == 0]


def plain_formulas(pred, gt, parts, alphas, m):
    """the quantities of the issue per clip, straightforwardly: torch.norm, boolean masks, np.sum -> (floats {name: (B, 4)}, hits (B, A, 4),
    terms {name: n per part (4,)})"""
    p, g = torch.from_numpy(pred), torch.from_numpy(gt)
    R, T, _, K = pred.shape
    B = R // m
    parts = np.asarray(parts)
    masks = [np.ones(K, dtype=bool)] + [parts == i for i in range(3)]
    dist = torch.norm(p - g, p=2, dim=2).numpy()  # (R, T, K)
    vp, vg = p[:, 1:] - p[:, :-1], g[:, 1:] - g[:, :-1]
    per_row = {'l2_sum': dist, 'speed_pred': torch.norm(vp, p=2, dim=2).numpy(), 'speed_gt': torch.norm(vg, p=2, dim=2).numpy(),
               'vel_l2': torch.norm(vp - vg, p=2, dim=2).numpy()}
    floats = {k: np.stack([np.sum(v[:, :, mk].reshape(m, B, -1), axis=(0, 2)) for mk in masks], axis=1) for k, v in per_row.items()}
    c = p.reshape(m, B, T, 2, K)
    div = sum((torch.norm(c[i] - c[j], p=2, dim=2).numpy() for i in range(m) for j in range(i + 1, m)), np.zeros((B, T, K)))
    floats['div_sum'] = np.stack([np.sum(div[:, :, mk].reshape(B, -1), axis=1) for mk in masks], axis=1)
    d2 = ((p - g) ** 2).sum(2).numpy()
    s = torch.maximum(g[:, :, 0].max(-1).values - g[:, :, 0].min(-1).values, g[:, :, 1].max(-1).values - g[:, :, 1].min(-1).values).numpy()
    hits = np.stack([np.stack([np.sum((d2 <= ((a * s) ** 2)[..., None])[:, :, mk].reshape(m, B, -1), axis=(0, 2)) for mk in masks], axis=1)
                     for a in alphas], axis=1)
    sizes = np.array([mk.sum() for mk in masks])
    terms = {'l2_sum': m * T * sizes, 'speed_pred': m * (T - 1) * sizes, 'speed_gt': m * (T - 1) * sizes, 'vel_l2': m * (T - 1) * sizes,
             'div_sum': m * (m - 1) // 2 * T * sizes}
    return floats, hits, terms


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_model_against_plain_formulas(shape):
    R, T, K = shape
    pred, gt = poses(R, T, K)
    parts = part_table(K)
    for i, m in enumerate(copies_for(R)):
        alphas = alphas_for(1 + (i + K) % 4)
        u = cm.unpack(cm.clip_metrics_model(pred, gt, parts, alphas, m))
        floats, hits, terms = plain_formulas(pred, gt, parts, alphas, m)
        assert np.array_equal(u['pck_hit'][:, :len(alphas)], hits) and not u['pck_hit'][:, len(alphas):].any()
        assert (u['seen'] == 1).all() and (u['copies'] == m).all() and (u['frames'] == T).all() and not u['nonfinite'].any()
        for name, want in floats.items():
            bar = (terms[name] + 2) * ULP * np.abs(want)
            err = np.abs(u[name] - want)
            assert (err <= bar).all(), "%s m=%d: error %s bar %s" % (name, m, err.max(), bar.max())
            assert (u[name][:, terms[name] == 0] == 0).all()
    if K > 1 and R * T * K > 50:
        frac = u['pck_hit'][:, 0, 0].sum() / (R * T * K)
        assert 0 < frac < 1, "the inputs leave PCK at %s: the comparison is not exercised" % frac


def tie_case():
    """gt: three keypoints whose bounding box is 8 x 2; with alpha = 0.25 the threshold is exactly 2.  Keypoint 0 is displaced by (2, 0): a hit
    (<=); keypoint 1 by (nextafter(2, 3), 0): a miss; keypoint 2 by nothing: a hit.  The displaced keypoints sit at x = 0, so pred - gt is exact."""
    gt = np.zeros((1, 1, 2, 3))
    gt[0, 0, 0] = [0.0, 0.0, 8.0]
    gt[0, 0, 1] = [0.0, 1.0, 2.0]
    pred = gt.copy()
    pred[0, 0, 0, 0] = 2.0
    pred[0, 0, 0, 1] = np.nextafter(2.0, 3.0)
    return pred, gt, [0, 1, 2], [0.25]


def single_keypoint_case():
    """K = 1: the box has side 0, a hit is exact equality.  Row 0: pred == gt; row 1: one ulp off."""
    gt = np.full((2, 1, 2, 1), 1.0)
    pred = gt.copy()
    pred[1, 0, 0, 0] = np.nextafter(1.0, 2.0)
    return pred, gt, [0], [0.1, 0.2]


def test_ties():
    pred, gt, parts, alphas = tie_case()
    u = cm.unpack(cm.clip_metrics_model(pred, gt, parts, alphas))
    assert u['pck_hit'][0, 0].tolist() == [2, 1, 0, 1]  # all, body (keypoint 0), face (keypoint 1), hands (keypoint 2)
    pred, gt, parts, alphas = single_keypoint_case()
    u = cm.unpack(cm.clip_metrics_model(pred, gt, parts, alphas))
    assert u['pck_hit'][0, :2, :2].tolist() == [[1, 1], [1, 1]] and not u['pck_hit'][1].any()
    assert u['l2_sum'][0, 0] == 0.0 and u['l2_sum'][1, 0] == 2.0 ** -52


def nan_case():
    pred, gt = poses(3, 4, 5, seed=3)
    pred[1, 2, 0, 3] = np.nan
    return pred, gt, part_table(5), [0.1, 0.2]


def test_nan_flags_one_clip_and_the_epoch_leaves_it_out():
    pred, gt, parts, alphas = nan_case()
    rec = cm.clip_metrics_model(pred, gt, parts, alphas)
    assert rec[:, cm.NONFINITE].tolist() == [0, 1, 0]
    clean = cm.clip_metrics_model(np.nan_to_num(pred), gt, parts, alphas)
    assert np.array_equal(rec[[0, 2]], clean[[0, 2]])  # no bit of another clip's record changes
    sizes = cm.part_sizes(parts)
    words = cm.epoch_model([rec], sizes, 2)
    assert words[cm.OUT_SEEN] == 3 and words[cm.OUT_NONFINITE] == 1
    without = clean.copy()
    without[1] = 0  # never seen
    ref = cm.epoch_model([without], sizes, 2)
    assert np.array_equal(words[:36], ref[:36]) and np.isfinite(words[:36].view(np.float64)).all()
    vals = cm.epoch_values(words, alphas)
    assert vals['clips_nonfinite'] == 1 and vals['clips_seen'] == 3 and 'diversity' not in vals
    assert vals['PCK'] == (vals['PCK_0.1'] + vals['PCK_0.2']) / 2


def test_lowest_rank_wins_and_unseen_clips_do_not_count():
    parts, alphas = part_table(5), [0.1, 0.2]
    sizes = cm.part_sizes(parts)
    a = cm.clip_metrics_model(*poses(6, 3, 5, seed=1), parts, alphas)
    b = cm.clip_metrics_model(*poses(6, 3, 5, seed=2), parts, alphas)
    t0, t1 = np.zeros((7, cm.COLS), dtype=np.int64), np.zeros((7, cm.COLS), dtype=np.int64)
    t0[[0, 1, 2]] = a[[0, 1, 2]]
    t1[[1, 2, 3, 4]] = b[[1, 2, 3, 4]]  # clips 1 and 2 on both ranks with other records; clips 5 and 6 on none
    want = np.zeros((7, cm.COLS), dtype=np.int64)
    want[[0, 1, 2]] = a[[0, 1, 2]]
    want[[3, 4]] = b[[3, 4]]
    assert np.array_equal(cm.merge_tables([t0, t1]), want)
    words = cm.epoch_model([t0, t1], sizes, 2, index_errors=3)
    assert np.array_equal(words, cm.epoch_model([want], sizes, 2, index_errors=3))
    assert words[cm.OUT_SEEN] == 5 and words[cm.OUT_INDEX_ERRORS] == 3
    assert not np.array_equal(words, cm.epoch_model([t1, t0], sizes, 2, index_errors=3))
    # the means divide by the terms of the five clips that count
    u = cm.unpack(want)
    l2 = cm.epoch_values(words, alphas)['L2_hands']
    assert abs(l2 - u['l2_sum'][:, 3].sum() / (5 * 3 * sizes[3])) <= 20 * ULP * l2
    # no clip at all, and T = 1: every mean is 0.0
    empty = cm.epoch_values(cm.epoch_model([np.zeros((4, cm.COLS), dtype=np.int64)], sizes, 2), alphas)
    assert empty['clips_seen'] == 0 and all(v == 0 for v in empty.values())
    one = cm.epoch_values(cm.epoch_model([cm.clip_metrics_model(*poses(2, 1, 5), parts, alphas)], sizes, 2), alphas)
    assert one['speed_ratio'] == 0.0 and one['vel_L2'] == 0.0 and one['L2_hands'] > 0


def _cfg(pipeline="Voice2Pose", **test_keys):
    cfg = get_cfg_defaults()
    cfg.PIPELINE_TYPE = pipeline
    for k, v in test_keys.items():
        cfg.TEST[k] = v
    return cfg


def test_check_clip_metrics():
    cfg = get_cfg_defaults()
    assert cfg.TEST.CLIP_METRICS is False and cfg.TEST.PCK_ALPHAS == [0.1, 0.2]
    assert check_clip_metrics(_cfg()) is None
    assert check_clip_metrics(_cfg(CLIP_METRICS=True)) == (0.1, 0.2)
    assert check_clip_metrics(_cfg(CLIP_METRICS=True, PCK_ALPHAS=[1, 0.5, 0.25, 2.0], MULTIPLE=16)) == (1.0, 0.5, 0.25, 2.0)
    for on in (False, True):  # the alphas are checked whether or not the key is on
        for bad in ([], [0.1] * 5, [0.1, 0], [0.1, -0.2], [float('nan')], [float('inf')], [True], 0.1, None, ['0.1']):
            with pytest.raises(ValueError, match="PCK_ALPHAS"):
                check_clip_metrics(_cfg(CLIP_METRICS=on, PCK_ALPHAS=bad))
    with pytest.raises(ValueError, match="CLIP_METRICS must be"):
        check_clip_metrics(_cfg(CLIP_METRICS=1))
    with pytest.raises(ValueError, match="MULTIPLE"):
        check_clip_metrics(_cfg(CLIP_METRICS=True, MULTIPLE=17))
    assert check_clip_metrics(_cfg(MULTIPLE=17)) is None  # the parent's loop takes any number of copies
    with pytest.raises(ValueError, match="Voice2Pose"):
        check_clip_metrics(_cfg("Pose2Pose", CLIP_METRICS=True))
    assert check_clip_metrics(_cfg("Pose2Pose")) is None


def test_size_checks_of_the_model():
    pred, gt = poses(4, 2, 5)
    with pytest.raises(ValueError):
        cm.clip_metrics_model(pred, gt, part_table(5), [0.1] * 5)
    with pytest.raises(ValueError):
        cm.clip_metrics_model(pred, gt, part_table(5), [0.1], multiple=3)
    with pytest.raises(ValueError):
        cm.clip_metrics_model(pred, gt, [0, 1, 2, 3, 0], [0.1])
    with pytest.raises(ValueError):
        cm.clip_metrics_model(pred, gt, None, [0.1])  # no default part table but for 121 keypoints


def test_command_line_arguments_and_npz_keys(tmp_path):
    a = cm.parse_args(["x.npz", "y.npz"])
    assert a.files == ["x.npz", "y.npz"] and a.alphas == [0.1, 0.2] and a.multiple == 1 and a.worst == 5 and a.out is None
    a = cm.parse_args(["x.npz", "--alphas", "0.05", "0.3", "0.5", "--worst", "2", "--out", "t.npz", "--multiple", "4"])
    assert a.alphas == [0.05, 0.3, 0.5] and a.worst == 2 and a.out == "t.npz" and a.multiple == 4
    with pytest.raises(ValueError):
        cm.parse_args(["x.npz", "--alphas", "0.1", "0.2", "0.3", "0.4", "0.5"])
    with pytest.raises(ValueError):
        cm.parse_args(["x.npz", "--alphas", "-1"])
    for bad in (["x.npz", "--multiple", "17"], ["x.npz", "--worst", "-1"], []):
        with pytest.raises(SystemExit):
            cm.parse_args(bad)
    pred, gt = poses(2, 3, 5)
    good, bad = str(tmp_path / "good.npz"), str(tmp_path / "bad.npz")
    np.savez(good, poses_pred_batch=pred.astype(np.float32), poses_gt_batch=gt, mu_pred=np.zeros((2, 4)))
    np.savez(bad, poses_pred_batch=pred, mu_pred=np.zeros((2, 4)))
    p, g = cm.load_poses(good)
    assert p.dtype == np.float64 and np.array_equal(p, pred.astype(np.float32).astype(np.float64)) and np.array_equal(g, gt)
    with pytest.raises(KeyError, match="poses_gt_batch"):
        cm.load_poses(bad)
    np.savez(bad, poses_pred_batch=pred, poses_gt_batch=gt[:1])
    with pytest.raises(ValueError, match="one shape"):
        cm.load_poses(bad)
    rec = cm.clip_metrics_model(pred, gt, part_table(5), [0.1])
    cm.save_table(str(tmp_path / "t.npz"), rec, [0.1])
    with np.load(str(tmp_path / "t.npz")) as z:
        assert np.array_equal(z["table"], rec) and tuple(z["columns"]) == cm.COLUMN_NAMES and len(cm.COLUMN_NAMES) == cm.COLS
        assert z["alphas"].tolist() == [0.1]
    err = cm.hand_errors(rec, cm.part_sizes(part_table(5)))
    u = cm.unpack(rec)
    assert np.array_equal(err, u['l2_sum'][:, 3] / (3.0 * 1))  # keypoint 2 is the one hand keypoint of five
