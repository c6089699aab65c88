"""The repair stage of the clip builder on the GPU (csrc/clip_builder.hip, clip_builder.py): device_repair against
the numpy contract models bit for bit on every video and parameter set synth_repair_videos.check() asserts, determinism, the untouched
input, the refused sizes, build_clips with and without the stage, one written clip through GestureDataset, and the command line."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import synth_repair_videos as R  # noqa: E402

from speechdrivestemplates_amd import clip_builder as cb  # noqa: E402

pytestmark = pytest.mark.gpu

RECORDS = ('valid', 'spike', 'filled', 'present_r', 'repaired_per_frame')
SPEAKER_PARAMS = [('rp_f32', 1, None), ('rp_f64', 4, (2, 3.0, 10.0))]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    r = str(tmp_path_factory.mktemp("repair_videos"))
    for sp in R.SPEAKERS:
        R.write_speaker(r, sp)
    return r


def on_device(video, dtype):
    a, present = R.video_frames(video, dtype)
    return a, present, torch.from_numpy(a).cuda(), torch.from_numpy(present.astype(np.uint8)).cuda()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("video,max_gap,despike", R.PARAMS)
def test_device_repair_equals_the_models_bit_for_bit(video, max_gap, despike, dtype):
    a, present, src, pres = on_device(video, dtype)
    before = src.clone()
    want = cb.model_repair(a, present, max_gap, despike)
    o = cb.device_repair(src, pres, max_gap, despike)
    again = cb.device_repair(src, pres, max_gap, despike)
    torch.cuda.synchronize()
    assert o['src_r'].dtype == src.dtype and o['src_r'].data_ptr() != src.data_ptr()
    assert o['src_r'].cpu().numpy().tobytes() == want['src_r'].tobytes(), int((o['src_r'].cpu().numpy() != want['src_r']).sum())
    for k in RECORDS:
        got = o[k].cpu().numpy()
        assert got.dtype == (np.int32 if k == 'repaired_per_frame' else np.uint8)
        assert np.array_equal(got, want[k].astype(got.dtype)), k
    for k in ('src_r',) + RECORDS:
        assert o[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), k
    assert before.cpu().numpy().tobytes() == src.cpu().numpy().tobytes() == a.tobytes()  # the input is read only
    # the stages behind it, on the repaired tracks, and the per-clip counts
    start = R.VIDEOS[video]['start']
    keep, _ = cb.model_frame_flags(want['src_r'], want['present_r'])
    starts = cb.model_clip_starts(keep, start, R.FRAMES)
    st = cb.device_frame_stages(o['src_r'], o['present_r'], start, R.FRAMES, 1)
    n_clips = int(st['n_clips'].item())
    assert np.array_equal(st['keep'].cpu().numpy().astype(bool), keep) and list(st['starts'][:n_clips].cpu().numpy()) == starts
    per_clip = cb.device_repaired_per_clip(o['repaired_per_frame'], st['starts'], n_clips, R.FRAMES)
    assert per_clip.dtype == torch.int32
    assert np.array_equal(per_clip.cpu().numpy(), cb.model_repaired_per_clip(want['repaired_per_frame'], starts, R.FRAMES))


def test_unsupported_sizes_raise_value_error():
    _, _, src, pres = on_device('r3', 'float32')
    for gap in (0, 65, -1):
        with pytest.raises(ValueError, match="max_gap"):
            cb.device_repair(src, pres, gap)
    for h in (4, -1):
        with pytest.raises(ValueError, match="half window"):
            cb.device_repair(src, pres, 4, (h, 3.0, 0.0))
    with pytest.raises(ValueError, match="frame count"):
        cb.device_repair(src[:0], pres[:0], 4)
    with pytest.raises(ValueError, match="kappa"):
        cb.device_repair(src, pres, 4, (2, -1.0, 0.0))
    from speechdrivestemplates_amd import _lib
    assert _lib.load().sdt_clip_repair_workspace_bytes((1 << 30) + 1) < 0 and _lib.load().sdt_clip_repair_workspace_bytes(3) == 32
    torch.cuda.synchronize()


def model_speaker(sp, max_gap, despike):
    """per video of the speaker: dict(starts, starts0, poses, per_clip, summary) from the models"""
    dtype, videos, start = R.SPEAKERS[sp]
    out = {}
    for video in videos:
        a, present = R.video_frames(video, dtype)
        keep0, _ = cb.model_frame_flags(a, present)
        starts0 = cb.model_clip_starts(keep0, start, R.FRAMES)
        rep = cb.model_repair(a, present, max_gap, despike)
        keep, dist = cb.model_frame_flags(rep['src_r'], rep['present_r'])
        means, _ = cb.model_shoulder_means(dist[keep], 1)
        scalar = cb.model_scalar(means)
        starts = cb.model_clip_starts(keep, start, R.FRAMES)
        scaled = cb.model_scale(rep['src_r'], scalar, True)
        per_clip = cb.model_repaired_per_clip(rep['repaired_per_frame'], starts, R.FRAMES)
        out[video] = dict(starts=starts, starts0=starts0, rep=rep, per_clip=per_clip, scalar=scalar, keep=keep,
                          poses=np.stack([scaled[s:s + R.FRAMES] for s in starts]) if starts else np.zeros((0, R.FRAMES, 3, 137), a.dtype),
                          summary=cb.model_repair_summary(present, keep0, keep, rep, starts0, starts, per_clip, R.FRAMES))
    return out


@pytest.mark.parametrize("sp,max_gap,despike", SPEAKER_PARAMS)
def test_build_clips_with_repair_equals_the_models(root, sp, max_gap, despike):
    start = R.SPEAKERS[sp][2]
    res = cb.build_clips(root, sp, start_frame=start, num_frames=R.FRAMES, write=False, repair_max_gap=max_gap, despike=despike)
    want = model_speaker(sp, max_gap, despike)
    assert want['r70']['starts0'] == [] and len(want['r70']['starts']) > 0  # (synth_repair_videos.check() asserts the same by its loop)
    row = 0
    for video in R.SPEAKERS[sp][1]:
        w, v = want[video], res['videos'][video]
        n = len(w['starts'])
        assert v['repair'] == w['summary'] and v['scalar'] == w['scalar'] and v['kept'] == int(w['keep'].sum())
        assert v['repair']['clips_without_repair'] == len(w['starts0']) and v['repair']['clips_with_repair'] == n == sum(v['clips'].values())
        assert 'repair' in v['timing']['kernel_ms'] and 'flags' in v['timing']['kernel_ms']
        poses = res['poses'][row:row + n].cpu().numpy()
        assert poses.tobytes() == w['poses'].tobytes()
        assert np.array_equal(res['repaired_per_clip'][row:row + n].cpu().numpy(), w['per_clip'])
        filled = np.stack([w['rep']['filled'][s:s + R.FRAMES] for s in w['starts']])
        assert filled.any() and (poses[:, :, 2, :][filled] == 0).all()  # filled points carry confidence 0
        table = res['table'][res['table']['interval_id'] == video]
        assert sorted(table['start']) == w['starts']
        row += n
    assert row == len(res['table']) == res['poses'].shape[0] == res['repaired_per_clip'].shape[0]
    assert res['videos']['r70']['repair']['frames_recovered'] > 0 and res['videos']['r257']['repair']['missing_recovered'] >= 1
    assert res['videos']['r257']['missing'] == 3


@pytest.mark.parametrize("sp", ['rp_f32', 'rp_f64'])
def test_repair_off_is_the_call_without_the_argument(root, sp):
    start = R.SPEAKERS[sp][2]
    plain = cb.build_clips(root, sp, start_frame=start, num_frames=R.FRAMES, write=False)
    off = cb.build_clips(root, sp, start_frame=start, num_frames=R.FRAMES, write=False, repair_max_gap=0)
    assert sorted(plain) == sorted(off) and 'repaired_per_clip' not in off
    for k in ('poses', 'audio', 'audio_lengths'):
        assert plain[k].dtype == off[k].dtype and plain[k].shape == off[k].shape
        assert plain[k].cpu().numpy().tobytes() == off[k].cpu().numpy().tobytes()
    assert plain['table'].equals(off['table']) and np.array_equal(plain['order'], off['order'])
    for video, v in off['videos'].items():
        assert 'repair' not in v and 'repair' not in v['timing']['kernel_ms']
        assert {k: x for k, x in v.items() if k != 'timing'} == {k: x for k, x in plain['videos'][video].items() if k != 'timing'}
    assert sum(off['videos']['r70']['clips'].values()) == 0 and len(off['table']) > 0


def test_nan_on_a_kept_frame_is_still_the_existing_error(root):
    with pytest.raises(ValueError, match=r"r1_000000\.npy: non-finite keypoint coordinates"):
        cb.build_clips(root, 'rp_nan_f32', start_frame=0, num_frames=R.FRAMES, write=False, repair_max_gap=4)


def test_written_clip_reads_back_with_zero_score_at_the_repaired_keypoints(tmp_path):
    from speechdrivestemplates_amd.config import get_cfg_defaults
    from speechdrivestemplates_amd.core.datasets import gesture_dataset as gd
    sp, max_gap = 'rp_f32', 1
    root = str(tmp_path)
    R.write_speaker(root, sp)
    res = cb.build_clips(root, sp, start_frame=R.SPEAKERS[sp][2], num_frames=R.FRAMES, repair_max_gap=max_gap)
    assert list(res['table'].columns) == cb.COLUMNS and 'repair' in res['videos']['r70']
    want = model_speaker(sp, max_gap, None)['r70']
    s = want['starts'][0]
    with np.load(os.path.join(root, sp, cb.clip_relpath(sp, 'r70', s, R.FRAMES))) as z:
        assert sorted(z.files) == ['audio', 'imgs', 'pose'] and z['pose'].tobytes() == want['poses'][0].tobytes()
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(os.path.dirname(GOLDEN), "..", "configs", "voice2pose_sdt_bp.yaml"))
    cfg.merge_from_list(["DATASET.ROOT_DIR", root, "DATASET.SPEAKER", sp, "DATASET.NUM_FRAMES", R.FRAMES])
    cfg.freeze()
    k2 = 2 * 121
    stat = {'scale_factor': 1.0, 'mean': np.zeros(k2), 'std': np.ones(k2)}
    gd.register_speaker_stat(sp, parted=dict(stat), global_=dict(stat))
    ds = gd.GestureDataset(root, sp, 'train', cfg)
    rows = [i for i in range(len(ds)) if ds.clips.iloc[i]['interval_id'] == 'r70' and int(ds.clips.iloc[i]['start']) == s]
    assert len(rows) == 1
    item = ds[rows[0]]
    cols = [gd._KEEP_137[j] for j in gd._DROP_ROOT]  # the 137-keypoint index of each of the dataset's 121 columns
    filled = want['rep']['filled'][s:s + R.FRAMES][:, cols]
    score = item['poses_score'].numpy()
    assert score.shape == (R.FRAMES, 2, 121) and filled.any()
    assert np.array_equal(score == 0, np.repeat(filled[:, None, :], 2, axis=1))


def test_cli_prints_the_clip_counts(root, capsys):
    sp, max_gap, despike = SPEAKER_PARAMS[1]
    assert cb.main(["--root", root, "--speaker", sp, "--start-frame", str(R.SPEAKERS[sp][2]), "--frames", str(R.FRAMES), "--no-write",
                    "--repair-max-gap", str(max_gap), "--despike", str(despike[0]), str(despike[1]), str(despike[2])]) == 0
    out = capsys.readouterr().out
    want = model_speaker(sp, max_gap, despike)
    for video in R.SPEAKERS[sp][1]:
        line = [ln for ln in out.splitlines() if ln.startswith('video %s:' % video)]
        s = want[video]['summary']
        assert len(line) == 1 and 'clips %d -> %d' % (len(want[video]['starts0']), len(want[video]['starts'])) in line[0]
        assert 'repair filled %d points, %d spikes (%d not filled)' % (s['points_filled'], s['spikes'], s['spikes_unfilled']) in line[0]
    assert re.search(r"video r70: .* clips 0 -> [1-9]", out)
