"""The pose augmentation's host side (speechdrivestemplates_amd/pose_augment.py, TRAIN.POSE_AUGMENT): the mirror table
against the skeleton's own tables, the parameter maps, the numpy contract model's properties, the config node, the table sizes, the C entry
point's refusals and the command line.  No GPU."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

from conftest import REPO
from speechdrivestemplates_amd import pose_augment as PA
from speechdrivestemplates_amd.config import check_pose_augment, get_cfg_defaults
from speechdrivestemplates_amd.core.datasets.gesture_dataset import HAND_ROOT_L, HAND_ROOT_R, HEAD_ROOT, PoseTransforms

PERM = PoseTransforms.mirror_table()
ALL_ON = PA.options(seed=0x1234567890abcdef, mirror_prob=0.5, scale_pct=10.0, rot_deg=15.0)
MIRROR_ONLY = PA.options(seed=7, mirror_prob=1.0)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def clip_poses(B, T, K=121, seed=3):
    """-> (poses (B, T, 2, K) float32, score, mean (B, 2 K), std (B, 2 K)) as the synthetic data set makes them"""
    rng = np.random.Generator(np.random.PCG64([seed, B, T, K]))
    return (rng.standard_normal((B, T, 2, K)).astype(np.float32), rng.uniform(0, 1, (B, T, 2, K)).astype(np.float32),
            rng.standard_normal((B, 2 * K)) * 20.0, rng.uniform(2.0, 30.0, (B, 2 * K)))


# -- the mirror table ----------------------------------------------------------------------------------------------------------------------------
def test_the_mirror_table_is_an_involution_that_keeps_the_parts():
    assert sorted(PERM) == list(range(121))
    assert all(PERM[PERM[k]] == k for k in range(121))
    parts = PoseTransforms.part_table()
    assert all(parts[PERM[k]] == parts[k] for k in range(121))
    fixed = [k for k in range(121) if PERM[k] == k]
    # the nose, the jaw's tip, the bridge, the nostrils' middle and the lips' four midline points
    assert fixed == [0, 9 + 8, 9 + 27, 9 + 28, 9 + 29, 9 + 30, 9 + 33, 9 + 51, 9 + 57, 9 + 62, 9 + 66]
    assert (PERM[1], PERM[2], PERM[3], PERM[7]) == (4, 5, 6, 8) and PERM[9 + 68] == 9 + 69
    assert all(PERM[79 + j] == 100 + j for j in range(21))


def test_the_mirror_table_maps_part_roots_to_part_roots():
    root = PoseTransforms.part_roots(True)
    pi = lambda k: -1 if k < 0 else PERM[k]  # noqa: E731
    assert all(root[PERM[k]] == pi(root[k]) for k in range(121))
    assert PERM[HAND_ROOT_L] == HAND_ROOT_R and PERM[HAND_ROOT_R] == HAND_ROOT_L and PERM[HEAD_ROOT] == HEAD_ROOT
    assert all(r == -1 for r in PoseTransforms.part_roots(False))


def test_the_mirror_table_maps_the_skeleton_onto_itself():
    """the check that catches a wrong face index: every limb's image is a limb"""
    edges = {frozenset(e) for e in PoseTransforms.skeleton_edges()}
    assert len(edges) == 108
    image = {frozenset((PERM[a], PERM[b])) for a, b in PoseTransforms.skeleton_edges()}
    assert image == edges
    wrong = list(PERM)
    wrong[9 + 36], wrong[9 + 37], wrong[9 + 45], wrong[9 + 44] = 9 + 44, 9 + 45, 9 + 37, 9 + 36  # an eye's corner and lid swapped
    assert {frozenset((wrong[a], wrong[b])) for a, b in PoseTransforms.skeleton_edges()} != edges


# -- the parameter maps --------------------------------------------------------------------------------------------------------------------------
def test_tables_sit_at_the_centres_of_256_levels():
    s, r = PA.scale_table(10.0), PA.rot_table(15.0)
    assert s.shape == (256,) and r.shape == (256, 2) and s.dtype == r.dtype == np.float64
    assert s[0] == 1.0 + (-10.0 + 20.0 * 0.5 / 256.0) / 100.0 and s[255] == 1.0 + (-10.0 + 20.0 * 255.5 / 256.0) / 100.0
    assert 0.9 < s[0] < s[255] < 1.1 and abs((s[0] + s[255]) / 2 - 1.0) < 1e-15
    a = np.degrees(np.arctan2(r[:, 1], r[:, 0]))
    assert np.allclose(a, -15.0 + 30.0 * (np.arange(256) + 0.5) / 256.0, atol=1e-12) and np.allclose((r ** 2).sum(1), 1.0, atol=1e-15)
    assert np.array_equal(PA.scale_table(0.0), np.ones(256)) and np.array_equal(PA.rot_table(0.0), np.tile([1.0, 0.0], (256, 1)))
    assert not np.signbit(PA.rot_table(0.0)).any()


def test_parameter_maps_at_the_extremes_of_each_word():
    lo = PA.params_model(ALL_ON, 5, 0, n_clips=100, words=[0, 0, 0, 0])
    hi = PA.params_model(ALL_ON, 5, 0, n_clips=100, words=[0xffffffff] * 4)
    assert (lo['mirror'], lo['is'], lo['ir'], lo['eff'], lo['identity']) == (1, 0, 0, 105, 0)
    assert (hi['mirror'], hi['is'], hi['ir'], hi['eff'], hi['identity']) == (0, 255, 255, 5, 0)
    assert lo['s'] == PA.scale_table(10.0)[0] and hi['s'] == PA.scale_table(10.0)[255]
    assert (lo['c'], lo['sn']) == tuple(PA.rot_table(15.0)[0]) and (hi['c'], hi['sn']) == tuple(PA.rot_table(15.0)[255])
    assert lo['sn'] < 0 < hi['sn']
    # the mirror's threshold is floor(p 2^24) on the word's upper 24 bits
    assert PA.mirror_prob24(ALL_ON) == 1 << 23
    at = lambda w0: PA.params_model(ALL_ON, 0, 0, words=[w0, 0, 0, 0])['mirror']  # noqa: E731
    assert at(((1 << 23) - 1) << 8 | 0xff) == 1 and at((1 << 23) << 8) == 0
    # w3 is unused
    assert PA.params_model(ALL_ON, 0, 0, words=[1, 2, 3, 0]) == PA.params_model(ALL_ON, 0, 0, words=[1, 2, 3, 0xffffffff])
    rec = PA._record(lo)
    assert rec.shape == (PA.REC_COLS,) and PA.record_values(rec) == {k: (float(v) if k in ('s', 'c', 'sn') else int(v)) for k, v in lo.items()}
    assert 'mirrored' in PA.describe(rec) and 'code row 105' in PA.describe(rec)


def test_the_draw_uses_purpose_2_of_the_audio_augmenters_generator():
    from speechdrivestemplates_amd import augment as A
    w = A.philox4x32([0, 2, 9, 4], A._key(ALL_ON['seed']))
    assert PA.params_model(ALL_ON, 9, 4) == PA.params_model(ALL_ON, 9, 4, words=w)
    assert PA.params_model(ALL_ON, 9 + (1 << 32), 4 + (1 << 32), n_clips=1)['is'] == PA.params_model(ALL_ON, 9, 4)['is']  # the low 32 bits count
    other = [A.philox4x32([0, p, 9, 4], A._key(ALL_ON['seed'])) for p in (0, 1)]
    assert not any(np.array_equal(w, o) for o in other)


def test_mirror_probability_0_half_and_1():
    clips = range(4096)
    share = {}
    for prob in (0.0, 0.5, 1.0):
        opts = PA.options(seed=11, mirror_prob=prob)
        share[prob] = sum(PA.params_model(opts, c, 3)['mirror'] for c in clips) / 4096.0
    print("  mirrored share at 0, 0.5, 1: %s" % share)
    assert share[0.0] == 0.0 and share[1.0] == 1.0
    assert abs(share[0.5] - 0.5) <= 6 * np.sqrt(0.25 / 4096)  # six binomial standard deviations: 0.047


def test_per_clip_ignores_the_step():
    fixed, moving = PA.options(**dict(ALL_ON, per_clip=True)), ALL_ON
    draws = [PA.params_model(fixed, 17, s) for s in (0, 1, 99, (1 << 32) - 1)]
    assert all(d == draws[0] for d in draws)
    from speechdrivestemplates_amd import augment as A
    assert draws[0] == PA.params_model(fixed, 17, 5, words=A.philox4x32([0, 2, 17, 0], A._key(fixed['seed'])))
    assert len({(d['is'], d['ir']) for d in (PA.params_model(moving, 17, s) for s in range(8))}) > 1
    assert len({(PA.params_model(fixed, c, 0)['is']) for c in range(8)}) > 1  # ... but not the clip


# -- the model -----------------------------------------------------------------------------------------------------------------------------------
def test_identity_options_return_the_input_bits():
    poses, score, mean, std = clip_poses(2, 3)
    poses[0, 0, 0, :4] = [0.0, -0.0, np.float32(1e-40), -np.float32(1e-40)]
    bits = bits32(poses)
    bits[1, 2, 1, 7] = 0x7fc12345  # a NaN with a payload
    bits[1, 2, 0, 7] = 0xff800000  # -inf
    poses = bits.view(np.float32)
    out, score_out, eff, rec = PA.pose_model(poses, score, mean, std, [3, 4], 5, PA.options(seed=9), 10)
    assert np.array_equal(bits32(out), bits) and np.array_equal(bits32(score_out), bits32(score))
    assert list(eff) == [3, 4] and np.all(rec[:, PA.IDENTITY] == 1) and np.all(rec[:, PA.MIRROR] == 0)
    assert PA.pose_model(poses, None, mean, std, [3, 4], 5, PA.options(seed=9), 10)[1] is None
    # with an augmentation on no clip is the identity: a scale level is never exactly 1, an angle never exactly 0
    assert not np.any(PA.scale_table(10.0) == 1.0) and not np.any(PA.rot_table(15.0)[:, 1] == 0.0)


def test_the_model_is_the_stated_formula():
    poses, score, mean, std = clip_poses(2, 2)
    out, score_out, eff, rec = PA.pose_model(poses, score, mean, std, [1, 2], 3, ALL_ON, 50)
    for b, clip in enumerate((1, 2)):
        p = PA.params_model(ALL_ON, clip, 3, 50)
        assert eff[b] == clip + 50 * p['mirror'] == rec[b, PA.EFF]
        for k in (0, 3, 39, 45, 80, 120):
            m = PERM[k] if p['mirror'] else k
            dx = np.float64(poses[b, 1, 0, m]) * std[b, m] + mean[b, m]
            dy = np.float64(poses[b, 1, 1, m]) * std[b, 121 + m] + mean[b, 121 + m]
            dx = -dx if p['mirror'] else dx
            rx, ry = p['s'] * (p['c'] * dx - p['sn'] * dy), p['s'] * (p['sn'] * dx + p['c'] * dy)
            assert out[b, 1, 0, k] == np.float32((rx - mean[b, k]) / std[b, k])
            assert out[b, 1, 1, k] == np.float32((ry - mean[b, 121 + k]) / std[b, 121 + k])
            assert bits32(score_out[b, 1, :, k]).tolist() == bits32(score[b, 1, :, m]).tolist()


def test_mirror_twice_returns_the_coordinates():
    """Each pass rounds a normalised value to float32 once -- half an ulp of it, std in de-normalised units -- and the float64 operations
    around it add a few 2^-53 of the magnitudes involved.  So after two passes keypoint k's coordinate is within
    ulp32(out1[perm k]) std[perm k] / 2 + ulp32(out2[k]) std[k] / 2 (+ 1e-12 for the float64 part) of where it started: at most two ulp of the
    larger normalised value, scaled by the larger std."""
    poses, score, mean, std = clip_poses(3, 4)
    one, s1, e1, _ = PA.pose_model(poses, score, mean, std, [0, 1, 2], 0, MIRROR_ONLY, 3)
    two, s2, e2, _ = PA.pose_model(one, s1, mean, std, [0, 1, 2], 0, MIRROR_ONLY, 3)
    assert list(e1) == [3, 4, 5] and np.array_equal(bits32(s2), bits32(score)) and not np.array_equal(one, poses)
    m3, s3 = mean.reshape(3, 1, 2, 121), std.reshape(3, 1, 2, 121)
    d0, d2 = poses.astype(np.float64) * s3 + m3, two.astype(np.float64) * s3 + m3
    ulp = lambda a: np.spacing(np.abs(a)).astype(np.float64)  # noqa: E731
    bound = 0.5 * (ulp(one) * s3)[..., PERM] + 0.5 * ulp(two) * s3 + 1e-12
    err = np.abs(d2 - d0)
    print("  mirror twice: largest error %.3e, smallest margin to the bound %.3e" % (err.max(), (bound - err).min()))
    assert np.all(err <= bound)
    loose = 2.0 * np.maximum(ulp(one)[..., PERM], ulp(two)) * np.maximum(s3[..., PERM], s3)
    assert np.all(bound <= loose + 1e-12)


def _parted_to_global(d):
    root = np.array(PoseTransforms.part_roots(True))
    g = d.copy()
    sel = root >= 0
    g[..., sel] += d[..., root[sel]]
    return g


def test_mirror_in_hierarchical_space_is_mirror_in_global_space():
    rng = np.random.Generator(np.random.PCG64(5))
    o = rng.uniform(-1e3, 1e3, (6, 2, 121))  # de-normalised hierarchical offsets
    p = PA.params_model(MIRROR_ONLY, 0, 0)
    assert p['mirror'] == 1 and p['s'] == 1.0 and p['c'] == 1.0
    a = _parted_to_global(PA.coords_model(o, p, PERM))
    b = PA.coords_model(_parted_to_global(o), p, PERM)
    print("  mirror, hierarchical against global: largest difference %.3e" % np.abs(a - b).max())
    assert np.abs(a - b).max() <= 1e-12
    # with a scale and a rotation too: six rounded operations on magnitudes up to 2 * 1.5 * sqrt(2) * 1e3 -> 6 * 4.3e3 * 2^-53 = 3e-12
    p = PA.params_model(PA.options(seed=1, mirror_prob=1.0, scale_pct=50.0, rot_deg=45.0), 0, 0, words=[0, 0xffffffff, 0, 0])
    a, b = _parted_to_global(PA.coords_model(o, p, PERM)), PA.coords_model(_parted_to_global(o), p, PERM)
    print("  mirror + scale + rotation: largest difference %.3e" % np.abs(a - b).max())
    assert np.abs(a - b).max() <= 1e-11


def test_permuted_and_sliced_batches():
    poses, score, mean, std = clip_poses(5, 3)
    clips = [4, 9, 2, 7, 0]
    out, so, eff, rec = PA.pose_model(poses, score, mean, std, clips, 6, ALL_ON, 20)
    assert len(set(rec[:, PA.MIRROR])) == 2  # both branches
    order = [3, 0, 4, 2, 1]
    o2, s2, e2, r2 = PA.pose_model(poses[order], score[order], mean[order], std[order], [clips[i] for i in order], 6, ALL_ON, 20)
    assert np.array_equal(bits32(o2), bits32(out[order])) and np.array_equal(bits32(s2), bits32(so[order]))
    assert np.array_equal(e2, eff[order]) and np.array_equal(r2, rec[order])
    o3, s3, e3, r3 = PA.pose_model(poses[1:3], score[1:3], mean[1:3], std[1:3], clips[1:3], 6, ALL_ON, 20)
    assert np.array_equal(bits32(o3), bits32(out[1:3])) and np.array_equal(r3, rec[1:3])
    o4 = PA.pose_model(poses[:, :2], score[:, :2], mean, std, clips, 6, ALL_ON, 20)[0]  # fewer frames: the others' values
    assert np.array_equal(bits32(o4), bits32(out[:, :2]))


def test_a_non_finite_element_reaches_only_its_partners_outputs():
    poses, score, mean, std = clip_poses(1, 3)
    k_src = 79 + 4
    for opts, both in ((MIRROR_ONLY, False), (PA.options(seed=7, mirror_prob=1.0, scale_pct=10.0), False),
                       (PA.options(seed=7, mirror_prob=1.0, rot_deg=15.0), True)):
        clean = PA.pose_model(poses, None, mean, std, [0], 0, opts, 1)[0]
        bad = poses.copy()
        bad[0, 1, 0, k_src] = np.nan
        got = PA.pose_model(bad, None, mean, std, [0], 0, opts, 1)[0]
        hit = np.argwhere(bits32(got) != bits32(clean)).tolist()
        want = [[0, 1, 0, PERM[k_src]]] + ([[0, 1, 1, PERM[k_src]]] if both else [])
        assert hit == want and np.isnan(got[0, 1, 0, PERM[k_src]])


def test_a_hand_made_permutation_and_its_checks():
    poses, score, mean, std = clip_poses(2, 5, K=5)
    perm = [0, 2, 1, 4, 3]
    out, so, eff, rec = PA.pose_model(poses, score, mean, std, [0, 1], 0, MIRROR_ONLY, 2, perm)
    assert np.array_equal(bits32(so), bits32(score[..., perm])) and list(eff) == [2, 3]
    for bad in ([0, 1, 2, 3], [0, 1, 2, 3, 3], [0, 1, 2, 3, 5], [-1, 1, 2, 3, 4]):
        with pytest.raises(ValueError, match="permutation"):
            PA.pose_model(poses, score, mean, std, [0, 1], 0, MIRROR_ONLY, 2, bad)
    with pytest.raises(ValueError, match="121"):
        PA.pose_model(poses, score, mean, std, [0, 1], 0, MIRROR_ONLY, 2)
    with pytest.raises(ValueError, match="unknown"):
        PA.options(mirror=1.0)
    for kw in ({'mirror_prob': 1.5}, {'scale_pct': 51}, {'rot_deg': -1}, {'seed': -1}):
        with pytest.raises(ValueError):
            PA.options(**kw)


def test_the_device_function_has_no_cpu_fallback():
    poses, score, mean, std = clip_poses(1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PA.augment_poses(torch.from_numpy(poses), None, torch.from_numpy(mean), torch.from_numpy(std), torch.tensor([0]), torch.tensor([0]),
                         ALL_ON, 1)


# -- config --------------------------------------------------------------------------------------------------------------------------------------
P = "TRAIN.POSE_AUGMENT."


def _cfg(*pairs, pipeline="Voice2Pose"):
    cfg = get_cfg_defaults()
    cfg.merge_from_list(["PIPELINE_TYPE", pipeline] + list(pairs))
    return cfg


def test_defaults_return_none_and_leave_the_audio_node_alone():
    from speechdrivestemplates_amd import augment as A
    from speechdrivestemplates_amd.config import check_augment
    cfg = get_cfg_defaults()
    assert check_pose_augment(cfg) is None and check_augment(cfg) is None
    assert dict(cfg.TRAIN.POSE_AUGMENT) == {"ENABLE": False, "SEED": 0, "MIRROR_PROB": 0.0, "SCALE_PCT": 0.0, "ROT_DEG": 0.0, "PER_CLIP": False}
    assert "MIRROR_PROB" not in cfg.TRAIN.AUGMENT and "mirror_prob" not in A.NEUTRAL
    assert check_pose_augment(_cfg(P + "MIRROR_PROB", 0.5)) is None  # the other keys mean nothing with ENABLE off
    assert check_pose_augment(_cfg(P + "ROT_DEG", 99.0)) is None  # ... and are checked for their type only


def test_validated_values():
    got = check_pose_augment(_cfg(P + "ENABLE", True, P + "SEED", (1 << 64) - 1, P + "MIRROR_PROB", 1, P + "SCALE_PCT", 50, P + "ROT_DEG", 45,
                                  P + "PER_CLIP", True))
    assert got == {'seed': (1 << 64) - 1, 'mirror_prob': 1.0, 'scale_pct': 50.0, 'rot_deg': 45.0, 'per_clip': True}
    assert PA.options(**got) == got
    for pipeline in ("Voice2Pose", "Pose2Pose"):
        assert check_pose_augment(_cfg(P + "ENABLE", True, P + "ROT_DEG", 5.0, pipeline=pipeline))['rot_deg'] == 5.0


BAD_TYPES = [("ENABLE", 1), ("ENABLE", "yes"), ("SEED", 1.5), ("SEED", True), ("MIRROR_PROB", "half"), ("MIRROR_PROB", float("nan")),
             ("MIRROR_PROB", None), ("SCALE_PCT", [10]), ("SCALE_PCT", float("inf")), ("ROT_DEG", "steep"), ("ROT_DEG", None), ("PER_CLIP", 0),
             ("PER_CLIP", "no")]
BAD_RANGES = [("SEED", -1), ("SEED", 1 << 64), ("MIRROR_PROB", -0.1), ("MIRROR_PROB", 1.5), ("SCALE_PCT", -1), ("SCALE_PCT", 50.5),
              ("ROT_DEG", -0.5), ("ROT_DEG", 46)]


@pytest.mark.parametrize("key, value", BAD_TYPES, ids=lambda v: str(v)[:12])
def test_a_bad_type_raises_whether_enabled_or_not(key, value):
    for on in (False, True):
        cfg = _cfg(P + "ENABLE", value) if key == "ENABLE" else _cfg(P + "ENABLE", on, P + "MIRROR_PROB", 0.5, P + key, value)
        with pytest.raises(ValueError, match=r"TRAIN\.POSE_AUGMENT\." + key):
            check_pose_augment(cfg)


@pytest.mark.parametrize("key, value", BAD_RANGES, ids=lambda v: str(v)[:12])
def test_a_value_outside_its_range_raises_when_enabled(key, value):
    with pytest.raises(ValueError, match=r"TRAIN\.POSE_AUGMENT\." + key):
        check_pose_augment(_cfg(P + "ENABLE", True, P + "SCALE_PCT", 5.0, P + key, value))
    assert check_pose_augment(_cfg(P + "SCALE_PCT", 5.0, P + key, value)) is None


def test_enable_needs_121_keypoints_and_something_to_do():
    with pytest.raises(ValueError, match=r"TRAIN\.POSE_AUGMENT\.ENABLE.*NUM_LANDMARKS.*137"):
        check_pose_augment(_cfg(P + "ENABLE", True, P + "MIRROR_PROB", 0.5, "DATASET.NUM_LANDMARKS", 137))
    with pytest.raises(ValueError, match=r"TRAIN\.POSE_AUGMENT\.ENABLE.*neutral"):
        check_pose_augment(_cfg(P + "ENABLE", True))
    with pytest.raises(ValueError, match=r"TRAIN\.POSE_AUGMENT\.ENABLE.*PIPELINE_TYPE"):
        check_pose_augment(_cfg(P + "ENABLE", True, P + "MIRROR_PROB", 0.5, pipeline="Other"))


def test_every_shipped_yaml_validates():
    paths = sorted(glob.glob(os.path.join(REPO, "configs", "*.yaml")))
    assert len(paths) >= 4
    for path in paths:
        cfg = get_cfg_defaults()
        cfg.merge_from_file(path)
        assert check_pose_augment(cfg) is None, path
        cfg.merge_from_list([P + "ENABLE", True, P + "MIRROR_PROB", 0.5])
        assert check_pose_augment(cfg)['mirror_prob'] == 0.5, path


# -- table sizes ---------------------------------------------------------------------------------------------------------------------------------
def _yaml(name, *pairs):
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(REPO, "configs", name + ".yaml"))
    cfg.merge_from_list(list(pairs))
    cfg.freeze()
    return cfg


MIRROR_KEYS = (P + "ENABLE", True, P + "MIRROR_PROB", 0.5)
SCALE_KEYS = (P + "ENABLE", True, P + "SCALE_PCT", 5.0)


def test_rows_of_the_code_tables():
    assert PA.table_rows(None, 7) == 7 and PA.table_rows(PA.options(scale_pct=5.0), 7) == 7 and PA.table_rows(MIRROR_ONLY, 7) == 14
    assert PA.table_rows(PA.options(mirror_prob=2.0 ** -25), 7) == 7  # floor(p 2^24) == 0: no draw mirrors
    PA.check_table_rows("t", 14, MIRROR_ONLY, 7)
    PA.check_table_rows("t", 7, None, 7)
    with pytest.raises(RuntimeError, match=r"t has 7 rows but .*MIRROR_PROB > 0 needs 14 \(2 x 7 clips"):
        PA.check_table_rows("t", 7, MIRROR_ONLY, 7)
    with pytest.raises(RuntimeError, match=r"t has 14 rows but the training set has 7 clips \(a table of 14 rows"):
        PA.check_table_rows("t", 14, None, 7)


def test_voice2pose_table_sizes_and_checkpoint_mismatches():
    from speechdrivestemplates_amd.core.pipelines.voice2pose import Voice2PoseModel
    N, D = 6, 32
    assert Voice2PoseModel(_yaml("voice2pose_sdt_bp"), num_train_samples=N).clips_code.shape == (N, D)
    assert Voice2PoseModel(_yaml("voice2pose_sdt_bp", *SCALE_KEYS), num_train_samples=N).clips_code.shape == (N, D)
    on = Voice2PoseModel(_yaml("voice2pose_sdt_bp", *MIRROR_KEYS), num_train_samples=N)
    assert on.clips_code.shape == (2 * N, D) and on.num_clips == N and on.pose_aug_opts['mirror_prob'] == 0.5 and on._pose_augmenters == {}
    sd = lambda rows: {"module.clips_code": torch.zeros(rows, D)}  # noqa: E731
    with pytest.raises(RuntimeError, match=r"clips_code has 6 rows but .*needs 12 \(2 x 6 clips"):
        Voice2PoseModel(_yaml("voice2pose_sdt_bp", *MIRROR_KEYS), sd(N), N)
    with pytest.raises(RuntimeError, match=r"clips_code has 12 rows but the training set has 6 clips"):
        Voice2PoseModel(_yaml("voice2pose_sdt_bp"), sd(2 * N), N)
    assert Voice2PoseModel(_yaml("voice2pose_sdt_bp", *MIRROR_KEYS), sd(2 * N), N).clips_code.shape == (2 * N, D)
    late = Voice2PoseModel(_yaml("voice2pose_sdt_bp", *MIRROR_KEYS), sd(2 * N), None)  # no data set: the checkpoint's rows, half of them clips
    assert late.clips_code.shape == (2 * N, D) and late.num_clips == N
    # outside training the random rows are those of the clips as they are
    on.eval()
    torch.manual_seed(0)
    with torch.no_grad():
        on.clips_code.copy_(torch.arange(2 * N, dtype=torch.float32)[:, None].expand(2 * N, D))
    rows = on._eval_code(None, 4096, torch.device("cpu"), None, None, None, None, True)[:, 0]
    assert rows.min() == 0 and rows.max() == N - 1


def test_external_codes_are_checked_against_two_n_rows():
    from speechdrivestemplates_amd.core.pipelines.voice2pose import Voice2PoseModel
    N = 6
    assert Voice2PoseModel(_yaml("voice2pose_sdt_vae"), num_train_samples=N, external_codes=torch.zeros(N, 32)).clips_code.shape[0] == N
    with pytest.raises(RuntimeError, match=r"external clip codes have 5 rows but the training set has 6 clips$"):
        Voice2PoseModel(_yaml("voice2pose_sdt_vae"), num_train_samples=N, external_codes=torch.zeros(5, 32))
    with pytest.raises(RuntimeError, match=r"external clip codes have 6 rows but the training set has 6 clips and .*MIRROR_PROB > 0 needs 12"):
        Voice2PoseModel(_yaml("voice2pose_sdt_vae", *MIRROR_KEYS), num_train_samples=N, external_codes=torch.zeros(N, 32))
    ok = Voice2PoseModel(_yaml("voice2pose_sdt_vae", *MIRROR_KEYS), num_train_samples=N, external_codes=torch.zeros(2 * N, 32))
    assert ok.clips_code.shape[0] == 2 * N and ok.num_clips == N


def test_pose2pose_buffer_sizes_and_checkpoint_mismatches():
    from speechdrivestemplates_amd.core.pipelines.pose2pose import Pose2PoseModel
    N = 6
    off, on = Pose2PoseModel(_yaml("pose2pose"), None, N), Pose2PoseModel(_yaml("pose2pose", *MIRROR_KEYS), None, N)
    assert off.clip_code_mu.shape[0] == off.clip_code_logvar.shape[0] == N and off.pose_aug_opts is None
    assert on.clip_code_mu.shape[0] == on.clip_code_logvar.shape[0] == 2 * N and on.num_clips == N
    d = off.clip_code_mu.shape[1]
    with pytest.raises(RuntimeError, match=r"clip_code_mu has 6 rows but .*needs 12"):
        Pose2PoseModel(_yaml("pose2pose", *MIRROR_KEYS), {"module.clip_code_mu": torch.zeros(N, d)}, N)
    with pytest.raises(RuntimeError, match=r"clip_code_mu has 12 rows but the training set has 6 clips"):
        Pose2PoseModel(_yaml("pose2pose"), {"module.clip_code_mu": torch.zeros(2 * N, d)}, N)
    assert Pose2PoseModel(_yaml("pose2pose", *MIRROR_KEYS), {"module.clip_code_mu": torch.zeros(2 * N, d)}, None).num_clips == N


# -- the C entry point ---------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_unsupported_sizes_before_any_launch():
    """outside K in [1, 128], B in [1, 65535], T in [1, 2^24], n_clips in [1, 2^40] the entry point returns SDT_ERR_UNSUPPORTED; a perm that
    is no permutation, a null pointer or an in-place call is an argument error -- all before any launch (there is no GPU here)"""
    from speechdrivestemplates_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    q = C.c_void_p(C.addressof(buf) + 32)
    perm = PA.perm_array([0, 2, 1])

    def call(B=1, T=1, K=3, n_clips=1, prob=0, per_clip=0, perm=perm, out=q, poses=p):
        return lib.sdt_pose_augment_f32(poses, None, p, p, B, T, K, p, p, n_clips, 0, prob, per_clip, perm, p, p, out, None, p, p, None)

    for kw in ({'K': 0}, {'K': 129}, {'B': 0}, {'B': 65536}, {'T': 0}, {'T': (1 << 24) + 1}, {'n_clips': 0}, {'n_clips': (1 << 40) + 1}):
        assert call(**kw) == -3, kw  # SDT_ERR_UNSUPPORTED
        assert b"sdt_pose_augment_f32" in lib.sdt_last_error()
    for kw in ({'perm': PA.perm_array([0, 1, 1])}, {'perm': PA.perm_array([0, 1, 3])}, {'perm': PA.perm_array([-1, 1, 2])}, {'prob': -1},
               {'prob': (1 << 24) + 1}, {'per_clip': 2}, {'out': p}, {'poses': None}, {'perm': None}):
        assert call(**kw) == -1, kw  # SDT_ERR_ARG
    assert call(perm=PA.perm_array([2, 2, 0])) == -1 and b"permutation" in lib.sdt_last_error()


# -- command line --------------------------------------------------------------------------------------------------------------------------------
def test_command_line_arguments():
    a = PA.parse_args(["clip.npz", "out.npz", "--speaker", "oliver", "--step", "3", "--clip", "9", "--mirror-prob", "0.5", "--per-clip"])
    assert (a.inp, a.out, a.speaker, a.step, a.clip, a.seed, a.mirror_prob, a.scale_pct, a.rot_deg, a.per_clip, a.n_clips, a.hierarchical) == \
        ("clip.npz", "out.npz", "oliver", 3, 9, 0, 0.5, 0.0, 0.0, True, 10, True)
    a = PA.parse_args(["c.npz", "o.npz", "--speaker", "x", "--step", "0", "--clip", "0", "--n-clips", "100", "--global", "--rot-deg", "45"])
    assert a.n_clips == 100 and a.hierarchical is False and a.rot_deg == 45.0
    base = ["c.npz", "o.npz", "--speaker", "x", "--step", "0", "--clip", "4"]
    for bad in (["--mirror-prob", "1.5"], ["--scale-pct", "51"], ["--rot-deg", "-1"], ["--seed", "-2"], ["--n-clips", "4"]):
        with pytest.raises(SystemExit):
            PA.parse_args(base + bad)
    with pytest.raises(SystemExit):
        PA.parse_args(["c.npz", "o.npz", "--step", "0", "--clip", "0"])  # no speaker
