"""The pose augmentation on the GPU (csrc/pose_augment.hip, speechdrivestemplates_amd/pose_augment.py, TRAIN.POSE_AUGMENT; DESIGN.md section
30) against the numpy contract model.

Bars.  The kernel runs the model's float64 operations in the model's order, each rounded on its own, and calls no transcendental function
(the scale factors and the (cos, sin) pairs are host-made tables): poses, confidences, effective indices and records are bit-identical.
Every comparison prints how many values were bit-identical before it asserts.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import REPO
from speechdrivestemplates_amd import pose_augment as PA
from test_pose_augment_host import ALL_ON, MIRROR_ONLY, PERM, bits32, clip_poses

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1, 1), (1, 1, 121), (2, 3, 121), (3, 64, 121), (33, 2, 121), (2, 5, 5)]
HAND_PERM = [0, 2, 1, 4, 3]
CLIPS = [0, 1 << 31, (1 << 32) + 5]  # (the low 32 bits count for the draw, all 64 for the effective index)
STEPS = [0, 1, (1 << 32) - 1]
N_CLIPS = [1, 1 << 33]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def dev(x):
    return torch.from_numpy(np.array(x, copy=True)).to(DEV)  # (a copy: the shared inputs are read-only arrays)


def i64(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64, device=DEV)


def case_of(shape):
    """-> (clip indices, step, n_clips, perm) of a shape: the indices, the steps and the two table sizes take turns"""
    k = SHAPES.index(shape)
    return [CLIPS[(k + b) % 3] for b in range(shape[0])], STEPS[k % 3], N_CLIPS[k % 2], (PERM if shape[2] == 121 else HAND_PERM if shape[2] == 5 else [0])


@functools.lru_cache(maxsize=None)
def inputs_of(shape):
    arrays = clip_poses(*shape)
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def model_of(shape):
    """pose_model with every augmentation on, computed once per shape"""
    clips, step, n_clips, perm = case_of(shape)
    out = PA.pose_model(*inputs_of(shape), clips, step, ALL_ON, n_clips, perm)
    for a in out:
        a.setflags(write=False)
    return out


def run(poses, score, mean, std, clips, step, opts, n_clips, perm=None, **kw):
    out, so, eff, rec = PA.augment_poses(dev(poses), None if score is None else dev(score), dev(mean), dev(std), i64(clips), i64([step]), opts,
                                         n_clips, perm, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if so is None else so.cpu().numpy(), eff.cpu().numpy(), rec.cpu().numpy()


def same(name, got, want):
    """all four outputs bit-identical"""
    for what, g, w in zip(("poses", "score"), got[:2], want[:2]):
        if w is None:
            assert g is None
            continue
        assert g.shape == w.shape and g.dtype == np.float32
        n = int((bits32(g) == bits32(w)).sum())
        print("  %-52s %d of %d %s values bit-identical" % (name, n, g.size, what))
        assert n == g.size, "%s: %d of %d %s values differ in bits" % (name, g.size - n, g.size, what)
    assert got[2].dtype == np.int64 and np.array_equal(got[2], want[2]), "%s: effective indices %s, want %s" % (name, got[2], want[2])
    assert got[3].dtype == np.int64 and np.array_equal(got[3], want[3]), "%s: records differ\n%s\n%s" % (name, got[3], want[3])


# -- the kernel against the model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_outputs_and_records_equal_the_model(shape):
    clips, step, n_clips, perm = case_of(shape)
    want = model_of(shape)
    same("%dx%dx%d clips %s step %d N %d" % (shape + (clips, step, n_clips)), run(*inputs_of(shape), clips, step, ALL_ON, n_clips, perm), want)
    assert np.array_equal(want[2], np.array(clips) + n_clips * want[3][:, PA.MIRROR]) and np.isfinite(want[0]).all()


def test_every_branch_is_taken_and_the_score_may_be_null():
    """over a few steps of the (3, 64, 121) case: mirrored and not -- and still the model's bits; then the same without a score"""
    shape = (3, 64, 121)
    poses, score, mean, std = inputs_of(shape)
    seen = set()
    for step in (2, 3, 4):
        want = PA.pose_model(poses, score, mean, std, CLIPS, step, ALL_ON, 1 << 33)
        same("step %d" % step, run(poses, score, mean, std, CLIPS, step, ALL_ON, 1 << 33), want)
        seen.update(int(v) for v in want[3][:, PA.MIRROR])
    assert seen == {0, 1}
    want = PA.pose_model(poses, None, mean, std, CLIPS, 2, ALL_ON, 1)
    got = run(poses, None, mean, std, CLIPS, 2, ALL_ON, 1)
    assert got[1] is None
    same("no score", got, want)
    # mirror alone, scale alone, rotation alone, PER_CLIP: each its own path through the kernel
    for name, opts in (("mirror alone", MIRROR_ONLY), ("scale alone", PA.options(seed=5, scale_pct=50.0)),
                       ("rotation alone", PA.options(seed=5, rot_deg=45.0)), ("per clip", PA.options(**dict(ALL_ON, per_clip=True)))):
        same(name, run(poses, score, mean, std, CLIPS, 1, opts, 7), PA.pose_model(poses, score, mean, std, CLIPS, 1, opts, 7))
    a, b = (run(poses, score, mean, std, CLIPS, s, PA.options(**dict(ALL_ON, per_clip=True)), 7) for s in (1, 2))
    assert np.array_equal(a[3], b[3]) and np.array_equal(bits32(a[0]), bits32(b[0]))


def test_a_nan_and_an_inf_reach_only_their_partners_outputs():
    shape = (2, 3, 121)
    poses, score, mean, std = inputs_of(shape)
    k_src = 79 + 4
    for name, opts, both in (("mirror", MIRROR_ONLY, False), ("mirror + rotation", PA.options(seed=7, mirror_prob=1.0, rot_deg=15.0), True)):
        clean = run(poses, score, mean, std, [0, 1], 0, opts, 2)
        bad = poses.copy()
        bad[1, 1, 0, k_src], bad[1, 2, 1, k_src] = np.nan, np.inf
        got = run(bad, score, mean, std, [0, 1], 0, opts, 2)
        same(name + " with a NaN and an inf", got, PA.pose_model(bad, score, mean, std, [0, 1], 0, opts, 2))
        hit = np.argwhere(bits32(got[0]) != bits32(clean[0])).tolist()
        k = PERM[k_src]
        want = sorted([[1, 1, 0, k], [1, 2, 1, k]] + ([[1, 1, 1, k], [1, 2, 0, k]] if both else []))
        print("  %-52s outputs that changed: %s" % (name, hit))
        assert hit == want and np.isnan(got[0][1, 1, 0, k]) and not np.isfinite(got[0][1, 2, 1, k])
        assert np.array_equal(bits32(got[1]), bits32(clean[1])) and np.array_equal(got[3], clean[3])


@pytest.mark.parametrize("offset", [0, 1, 3], ids=lambda o: "offset%d" % o)
def test_guard_bands_around_the_outputs_stay_untouched(offset):
    """poses_out and score_out start ``offset`` floats past a 16-byte boundary, between bands of NaN"""
    shape = (2, 3, 121)
    clips, step, n_clips, perm = case_of(shape)
    guard, n = 64, int(np.prod(shape)) * 2
    bufs = [torch.full((guard + offset + n + guard,), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2)]
    views = [b[guard + offset:guard + offset + n].view(shape[0], shape[1], 2, shape[2]) for b in bufs]
    rec = torch.full((shape[0] + 2, PA.REC_COLS), -1, dtype=torch.int64, device=DEV)
    poses, score, mean, std = inputs_of(shape)
    out, so, eff, r = PA.augment_poses(dev(poses), dev(score), dev(mean), dev(std), i64(clips), i64([step]), ALL_ON, n_clips, perm,
                                       out=views[0], score_out=views[1], rec=rec[1:-1])
    torch.cuda.synchronize()
    assert out.data_ptr() == views[0].data_ptr() and so.data_ptr() == views[1].data_ptr()
    for b in bufs:
        host = b.cpu().numpy()
        assert np.isnan(host[:guard + offset]).all() and np.isnan(host[guard + offset + n:]).all()
    assert torch.all(rec[0] == -1) and torch.all(rec[-1] == -1)
    same("into views at offset %d" % offset, (out.cpu().numpy(), so.cpu().numpy(), eff.cpu().numpy(), r.cpu().numpy()), model_of(shape))
    with pytest.raises(RuntimeError, match="never runs in place"):
        x = dev(poses)
        PA.augment_poses(x, None, dev(mean), dev(std), i64(clips), i64([step]), ALL_ON, n_clips, perm, out=x)


def test_identity_options_return_the_input_bits():
    poses, score, mean, std = (a.copy() for a in inputs_of((2, 3, 121)))
    poses[0, 0, 0, :4] = [0.0, -0.0, np.float32(1e-40), -np.float32(1e-40)]
    bits = bits32(poses)
    bits[1, 2, 1, 7], bits[1, 2, 0, 7] = 0x7fc12345, 0xff800000  # a NaN with a payload, -inf
    poses = bits.view(np.float32)
    got = run(poses, score, mean, std, [3, 4], 5, PA.options(seed=9), 10)
    n = int((bits32(got[0]) == bits).sum())
    print("  %-52s %d of %d values bit-identical" % ("identity options", n, bits.size))
    assert n == bits.size and np.array_equal(bits32(got[1]), bits32(score)) and list(got[2]) == [3, 4] and np.all(got[3][:, PA.IDENTITY] == 1)
    same("identity options against the model", got, PA.pose_model(poses, score, mean, std, [3, 4], 5, PA.options(seed=9), 10))


def test_refusals_on_the_device_route():
    poses, score, mean, std = inputs_of((2, 5, 5))
    with pytest.raises(ValueError, match="permutation"):
        run(poses, score, mean, std, [0, 1], 0, ALL_ON, 2, [0, 1, 2, 3, 3])
    with pytest.raises(ValueError, match="121"):
        run(poses, score, mean, std, [0, 1], 0, ALL_ON, 2)
    with pytest.raises(ValueError, match="n_clips"):
        run(poses, score, mean, std, [0, 1], 0, ALL_ON, 0, HAND_PERM)
    with pytest.raises(ValueError, match="mean"):
        run(poses, score, mean[:, :9], std, [0, 1], 0, ALL_ON, 2, HAND_PERM)
    with pytest.raises(TypeError, match="mean"):
        run(poses, score, mean.astype(np.float32), std, [0, 1], 0, ALL_ON, 2, HAND_PERM)


# -- graph ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_call_follows_the_step_tensor():
    shape = (3, 64, 121)
    poses, score, mean, std = (dev(a) for a in inputs_of(shape))
    clips = i64(CLIPS)
    aug = PA.PoseAugmenter(ALL_ON, DEV, 1 << 33)
    steps = [3, (1 << 32) - 1, 77]
    eager = []
    for s in steps:  # (these eager calls also allocate the augmenter's record buffer: the capture and the replays allocate none)
        out, so, eff = aug(poses, score, mean, std, clips, i64([s]))
        eager.append(tuple(t.cpu().numpy() for t in (out, so, eff, aug.record)))
    assert not np.array_equal(eager[0][3], eager[1][3]) and not np.array_equal(eager[0][3], eager[2][3])
    ptrs = {k: t.data_ptr() for k, t in aug._bufs.items()}
    step_t = i64([0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = aug(poses, score, mean, std, clips, step_t)
    assert {k: t.data_ptr() for k, t in aug._bufs.items()} == ptrs
    for s, want in zip(steps, eager):
        step_t.copy_(i64([s]))
        g.replay()
        torch.cuda.synchronize()
        same("replay at step %d" % s, tuple(t.cpu().numpy() for t in static + (aug.record,)), want)


# -- pipelines -----------------------------------------------------------------------------------------------------------------------------------
P = "TRAIN.POSE_AUGMENT."
KEYS = [P + "SEED", 1234, P + "MIRROR_PROB", 0.5, P + "SCALE_PCT", 10.0, P + "ROT_DEG", 15.0]
ON, OFF = [P + "ENABLE", True] + KEYS, [P + "ENABLE", False] + KEYS
GLOBAL_STEPS = (1, 2)
N = 4


def _bits(t):
    return t.detach().float().cpu().numpy().view(np.int32)


def _build(name, extra, state):
    """pipeline on the oracle's seeded initial state (as __graft_entry__.make_pipeline builds it)"""
    from speechdrivestemplates_amd.config import get_cfg_defaults
    from speechdrivestemplates_amd.core.datasets import gesture_dataset as gd
    from speechdrivestemplates_amd.core.pipelines import get_pipeline
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(REPO, "configs", name + ".yaml"))
    cfg.merge_from_list(["DATASET.NAME", "SyntheticGestureDataset", "DATASET.SYNTHETIC_CLIPS", N, "SYS.LOG_INTERVAL", 10 ** 9,
                         "TRAIN.BATCH_SIZE", 4, "TEST.BATCH_SIZE", 4, "SYS.NUM_WORKERS", 0, "TRAIN.LR_SCHEDULER", False,
                         "TRAIN.SAVE_VIDEO", False, "TEST.SAVE_VIDEO", False, "TEST.SAVE_NPZ", False] + list(extra))
    cfg.freeze()
    pipe = get_pipeline(cfg.PIPELINE_TYPE)(cfg)
    pipe.num_train_samples = N
    pipe.train_dataset = gd.SyntheticGestureDataset(cfg=cfg, num_clips=N)
    pipe.setup_model(cfg, state_dict={"module." + k: v for k, v in state.items()})
    pipe.setup_optimizer()
    pipe.model.train()
    return pipe


def _v2p(extra=(), mirror_rows=False):
    from oracle import sdt_oracle as O
    state = O.make_voice2pose_state(O.cfg_named("voice2pose_sdt_bp"), N, seed=0, code_std=0.5)
    if mirror_rows:  # rows N .. 2 N - 1 for the mirrored clips, the rest of the state as it is
        state["clips_code"] = torch.cat([state["clips_code"], state["clips_code"].flip(0) * 0.5])
    return _build("voice2pose_sdt_bp", extra, state)


def _p2p(extra=(), mirror_rows=False):
    from oracle import sdt_oracle as O
    state = O.make_pose2pose_state(O.cfg_named("pose2pose"), N, seed=0)
    state["mel_transfm.spectrogram.window"], state["mel_transfm.mel_scale.fb"] = O.mel_window(), O.mel_filterbank()
    if mirror_rows:
        for k in ("clip_code_mu", "clip_code_logvar"):
            state[k] = torch.cat([state[k], state[k]])
    return _build("pose2pose", extra, state)


def _batch(step, b=2):
    from oracle import sdt_oracle as O
    return O.make_batch(b, N, step=step, seed=1)


def _manual_steps(pipe, with_step, loss_key):
    out = []
    for gs in GLOBAL_STEPS:
        batch = _batch(gs)
        if with_step:
            batch['aug_step'] = torch.tensor([gs], dtype=torch.int64)
        torch.manual_seed(gs)  # (pose2pose draws its reparameterisation noise from torch's generator)
        losses, results = pipe.forward_backward(batch)
        pipe.optimizer_updates(losses)
        torch.cuda.synchronize()
        out.append((_bits(losses[loss_key]), _bits(results['poses_gt_batch']), batch))
    return out


def _expected_gt(batch, gs, opts):
    stat = batch['speaker_stat']
    return PA.pose_model(batch['poses'].numpy(), None, stat['mean'].numpy(), stat['std'].numpy(), batch['clip_index'].numpy(), gs, opts, N)


@pytest.mark.parametrize("kind", ["voice2pose", "pose2pose"])
def test_pipeline_with_the_key_on_off_and_in_eval(kind):
    make, loss_key = (_v2p, 'G_loss') if kind == "voice2pose" else (_p2p, 'loss')
    on, off, plain = make(ON, mirror_rows=True), make(OFF), make()
    opts = on.model.pose_aug_opts
    assert opts == PA.options(seed=1234, mirror_prob=0.5, scale_pct=10.0, rot_deg=15.0) and off.model.pose_aug_opts is None
    table = on.model.clips_code if kind == "voice2pose" else on.model.clip_code_mu
    assert table.shape[0] == 2 * N and (off.model.clips_code if kind == "voice2pose" else off.model.clip_code_mu).shape[0] == N
    # evaluation sees untouched poses, and no PoseAugmenter is built for it
    probe = _batch(0)
    on.model.eval()
    with torch.no_grad():
        torch.manual_seed(0)
        res = (on.model(probe, on.train_dataset) if kind == "voice2pose" else on.model(probe))[1]
    on.model.train()
    assert np.array_equal(_bits(res['poses_gt_batch']), _bits(probe['poses'])) and on.model._pose_augmenters == {}
    with pytest.raises(KeyError, match="aug_step"):
        on.model(_batch(0), on.train_dataset) if kind == "voice2pose" else on.model(_batch(0))
    r_on, r_off, r_plain = _manual_steps(on, True, loss_key), _manual_steps(off, False, loss_key), _manual_steps(plain, False, loss_key)
    print("  %s on %s off %s" % (loss_key, [x[0].view(np.float32) for x in r_on], [x[0].view(np.float32) for x in r_off]))
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(r_off, r_plain)), "the key off is not the step as it was"
    assert all(np.array_equal(a[1], _bits(a[2]['poses'])) for a in r_off)
    assert all(not np.array_equal(a[0], b[0]) for a, b in zip(r_on, r_off)), "the augmentation did not reach the loss"
    for (_, gt, batch), gs in zip(r_on, GLOBAL_STEPS):  # poses_gt_batch, which the per-step metrics read, is the model's output
        want = _expected_gt(batch, gs, opts)
        n = int((gt.view(np.uint32) == bits32(want[0])).sum())
        print("  %-52s %d of %d values bit-identical" % ("%s poses_gt_batch at step %d" % (kind, gs), n, gt.size))
        assert n == gt.size
    assert off.model._pose_augmenters == {} and plain.model._pose_augmenters == {} and len(on.model._pose_augmenters) == 1
    rec = next(iter(on.model._pose_augmenters.values())).record.cpu().numpy()
    assert rec.shape == (2, PA.REC_COLS) and np.array_equal(rec, _expected_gt(r_on[-1][2], GLOBAL_STEPS[-1], opts)[3])
    for p in (on, off, plain):
        p.close()


def test_a_mirrored_clip_trains_its_own_code_row():
    """one train_step of voice2pose_sdt_bp with MIRROR_PROB 1: the batch's clips are 2 and 3, their gradient sits in rows N + 2 and N + 3"""
    pipe = _v2p([P + "ENABLE", True, P + "MIRROR_PROB", 1.0], mirror_rows=True)
    batch = _batch(1)
    clips = batch['clip_index'].tolist()
    assert clips == [2, 3]
    pipe.train_step(batch, 1, 1, 1)
    torch.cuda.synchronize()
    assert 'aug_step' not in batch
    grad = pipe.model.clips_code.grad.detach().cpu().numpy()
    rows = sorted(set(np.nonzero(np.abs(grad).sum(1))[0].tolist()))
    print("  rows of clips_code with a gradient: %s (batch clips %s, N = %d)" % (rows, clips, N))
    assert grad.shape[0] == 2 * N and rows == [N + c for c in clips]
    rec = next(iter(pipe.model._pose_augmenters.values())).record.cpu().numpy()
    assert np.all(rec[:, PA.MIRROR] == 1) and list(rec[:, PA.EFF]) == rows
    pipe.close()


def test_pose2pose_writes_its_codes_to_the_effective_rows():
    pipe = _p2p([P + "ENABLE", True, P + "MIRROR_PROB", 0.5, P + "SEED", 3], mirror_rows=True)
    opts = pipe.model.pose_aug_opts
    written = set()
    for gs in (1, 2, 3, 4):
        batch = _batch(gs)
        pipe.train_step(batch, 1, gs, 1)
        torch.cuda.synchronize()
        eff = [c + N * PA.params_model(opts, c, gs)['mirror'] for c in batch['clip_index'].tolist()]
        assert pipe.model.code_rows.tolist() == eff
        written.update(eff)
        mu = pipe.model.clip_code_mu.detach().cpu().numpy()
        assert sorted(set(np.nonzero(np.abs(mu).sum(1))[0].tolist())) == sorted(written), (gs, eff)
    print("  rows of clip_code_mu written after four steps: %s" % sorted(written))
    assert any(r >= N for r in written) and any(r < N for r in written)
    pipe.close()
