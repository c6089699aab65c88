"""The clip builder on the GPU (csrc/clip_builder.hip, clip_builder.py): every kernel stage against its numpy
contract model bit for bit (float32 and float64 keypoints, the edge cases synth_keypoint_videos.check() asserts), the resampler at
three ratios, determinism, and per-frame keypoints + wav -> clips -> statistics -> dataset -> one train step end to end."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import synth_keypoint_videos as S  # noqa: E402

from speechdrivestemplates_amd import clip_builder as cb  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    r = str(tmp_path_factory.mktemp("keypoint_videos"))
    for sp in S.SPEAKERS:
        S.write_speaker(r, sp)
    return r


def model_audio(video, start=S.START):
    """the contract model's 16 kHz track of a video, cut at the start frame"""
    rate, pcm = S.video_audio(video)
    return cb.model_resample(cb.model_pcm_to_mono(pcm)[cb.source_cut(start, rate):], rate)


def model_clips(video, dtype, chunks, scale_confidence=None):
    """-> (starts, poses (n, 64, 3, 137), [audio slices], scalar, keep)"""
    a, present = S.video_frames(video, dtype)
    keep, dist = cb.model_frame_flags(a, present)
    means, _ = cb.model_shoulder_means(dist[keep], chunks)
    scalar = cb.model_scalar(means)
    starts = cb.model_clip_starts(keep, S.START, S.FRAMES)
    scaled = cb.model_scale(a, scalar, cb.scales_confidence(chunks, scale_confidence))
    poses = np.stack([scaled[s:s + S.FRAMES] for s in starts]) if starts else np.zeros((0, S.FRAMES, 3, 137), a.dtype)
    track = model_audio(video)
    audio = []
    for s in starts:
        a0, a1 = cb.audio_offsets(s, S.START, S.FRAMES)
        audio.append(track[a0:a1])
    return starts, poses, audio, scalar, keep


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("video", sorted(S.VIDEOS))
def test_pose_stages_equal_the_models_bit_for_bit(video, dtype):
    a, present = S.video_frames(video, dtype)
    keep, dist = cb.model_frame_flags(a, present)
    src = torch.from_numpy(a).cuda()
    pres = torch.from_numpy(present.astype(np.uint8)).cuda()
    for chunks in (1, 3):
        o = cb.device_frame_stages(src, pres, S.START, S.FRAMES, chunks)
        torch.cuda.synchronize()
        assert np.array_equal(o['keep'].cpu().numpy().astype(bool), keep)
        assert np.array_equal(o['dist'].cpu().numpy(), dist)
        assert not o['bad'].any()
        prefix = o['prefix'].cpu().numpy()
        assert np.array_equal(prefix, np.concatenate([[0], np.cumsum(keep)]))
        assert np.array_equal(o['dist_kept'].cpu().numpy()[:prefix[-1]], dist[keep])
        means, dropped = cb.model_shoulder_means(dist[keep], chunks)
        assert np.array_equal(o['means'].cpu().numpy(), means)
        starts = cb.model_clip_starts(keep, S.START, S.FRAMES)
        n_clips = int(o['n_clips'].item())
        assert n_clips == len(starts) and list(o['starts'][:n_clips].cpu().numpy()) == starts
        scalar = cb.model_scalar(means)
        for conf in (True, False):
            got = cb.device_gather_poses(src, o['starts'], n_clips, S.FRAMES, scalar, conf)
            torch.cuda.synchronize()
            scaled = cb.model_scale(a, scalar, conf)
            assert got.shape == (n_clips, S.FRAMES, 3, 137) and str(got.dtype) == 'torch.' + dtype
            for i, s in enumerate(starts):
                assert np.array_equal(got[i].cpu().numpy(), scaled[s:s + S.FRAMES]), (video, dtype, chunks, conf, s)
    if video in ('vidC', 'vidD'):
        assert n_clips == 0
    if video == 'vidA':
        assert 0 < n_clips and dropped == 1  # (chunks == 3 here: 247 kept frames)


def test_confidence_row_scaled_with_one_chunk_and_untouched_with_three(root):
    a, _ = S.video_frames('vidB', 'float32')
    one = cb.build_clips(root, 'kp_f32', shoulder_chunks=1, write=False)
    three = cb.build_clips(root, 'kp_f32', shoulder_chunks=3, write=False)
    n_a = sum(one['videos']['vidA']['clips'].values())
    s1, s3 = one['videos']['vidB']['scalar'], three['videos']['vidB']['scalar']
    assert one['videos']['vidB']['scale_confidence'] and not three['videos']['vidB']['scale_confidence']
    assert one['videos']['vidA']['shoulder_dropped'] == 0 and three['videos']['vidA']['shoulder_dropped'] == 1
    first = a[S.START:S.START + S.FRAMES]  # vidB's first clip starts at START
    assert np.array_equal(one['poses'][n_a, :, 2].cpu().numpy(), first[:, 2] * np.float32(s1))
    assert np.array_equal(three['poses'][n_a, :, 2].cpu().numpy(), first[:, 2])
    assert np.array_equal(three['poses'][n_a, :, :2].cpu().numpy(), first[:, :2] * np.float32(s3))
    over = cb.build_clips(root, 'kp_f32', shoulder_chunks=3, scale_confidence=True, write=False)
    assert np.array_equal(over['poses'][n_a, :, 2].cpu().numpy(), first[:, 2] * np.float32(s3))


@pytest.mark.parametrize("fmt,channels,n,first", [("int16", 2, 10007, 0), ("int16", 2, 10007, 333), ("uint8", 1, 4099, 65),
                                                  ("float32", 1, 5001, 17), ("int32", 2, 3001, 1), ("float32", 3, 2049, 0), ("float32", 8, 1025, 3)])
def test_pcm_conversion_and_mixdown(fmt, channels, n, first):
    g = np.random.Generator(np.random.PCG64(n))
    shape = (n, channels) if channels > 1 else (n,)
    if fmt == "float32":
        pcm = g.uniform(-1, 1, shape).astype(np.float32)
    else:
        info = np.iinfo(fmt)
        pcm = g.integers(info.min, int(info.max) + 1, shape).astype(fmt)
    got = cb.device_pcm_to_mono(pcm, first).cpu().numpy()
    assert np.array_equal(got, cb.model_pcm_to_mono(pcm)[first:])


# lengths that are no multiple of the 64-sample tile, of `down` (3, 441, 1) or of 64, one tile, and a few samples
@pytest.mark.parametrize("sr_in,n", [(48000, 50003), (48000, 64), (48000, 5), (44100, 33335), (44100, 441), (44100, 1),
                                     (8000, 12347), (8000, 31)])
def test_resampler_equals_the_model_bit_for_bit(sr_in, n):
    x = np.random.Generator(np.random.PCG64(sr_in + n)).uniform(-1, 1, n).astype(np.float32)
    want = cb.model_resample(x, sr_in)
    got = cb.device_resample(torch.from_numpy(x).cuda(), sr_in).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(got, want), (int((got != want).sum()), float(np.abs(got - want).max()))


def test_16k_audio_is_not_filtered():
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).uniform(-1, 1, 1000).astype(np.float32)).cuda()
    assert cb.device_resample(x, 16000) is x


def test_audio_gather_gives_short_and_empty_trailing_slices():
    track = np.arange(1000, dtype=np.float32)
    a0, a1 = [0, 900, 990, 1000, 1200], [100, 1000, 1090, 1100, 1300]
    out, lengths = cb.device_gather_audio(torch.from_numpy(track).cuda(), a0, a1)
    assert list(lengths.cpu().numpy()) == [100, 100, 10, 0, 0] and out.shape == (5, 100)
    for i, (b, e) in enumerate(zip(a0, a1)):
        want = np.zeros(100, np.float32)
        want[:len(track[b:e])] = track[b:e]
        assert np.array_equal(out[i].cpu().numpy(), want)


@pytest.mark.parametrize("sp", ["kp_f32", "kp_f64"])
def test_write_false_equals_the_models_and_two_calls_are_identical(root, sp):
    dtype = S.SPEAKERS[sp][0]
    r1 = cb.build_clips(root, sp, shoulder_chunks=3, write=False)
    r2 = cb.build_clips(root, sp, shoulder_chunks=3, write=False)
    for k in ('poses', 'audio', 'audio_lengths'):
        assert r1[k].cpu().numpy().tobytes() == r2[k].cpu().numpy().tobytes()
    assert r1['table'].equals(r2['table'])
    row = 0
    lengths = r1['audio_lengths'].cpu().numpy()
    short = 0
    for video in S.SPEAKERS[sp][1]:
        starts, poses, audio, scalar, keep = model_clips(video, dtype, 3)
        v = r1['videos'][video]
        assert v['scalar'] == scalar and v['kept'] == int(keep.sum()) and v['dropped'] == len(keep) - int(keep.sum())
        assert v['missing'] == len(S.VIDEOS[video]['missing']) and sum(v['clips'].values()) == len(starts)
        assert np.array_equal(r1['poses'][row:row + len(starts)].cpu().numpy(), poses)
        for i, w in enumerate(audio):
            assert lengths[row + i] == len(w)
            assert np.array_equal(r1['audio'][row + i, :len(w)].cpu().numpy(), w) and not r1['audio'][row + i, len(w):].any()
            short += len(w) < 68266
        row += len(starts)
    assert row == len(r1['table']) == r1['poses'].shape[0] and short > 0  # vidB's audio ends before its video
    assert sorted(r1['order']) == list(range(row))
    assert list(r1['table']['dataset']) == sorted(r1['table']['dataset'], key=['train', 'idle', 'dev'].index)


def test_videos_without_clips_give_empty_outputs(root):
    r = cb.build_clips(root, 'kp_empty_f64', write=False)
    assert r['poses'].shape == (0, 64, 3, 137) and len(r['table']) == 0
    assert r['videos']['vidC']['clips'] == {'train': 0, 'idle': 0, 'dev': 0} and r['videos']['vidD']['outliers'] == 5


def test_non_finite_coordinate_names_the_file(tmp_path):
    root = str(tmp_path)
    base = S.write_speaker(root, 'kp_f32')
    bad = os.path.join(base, 'tmp', 'raw_pose_2d', 'vidB', 'vidB_000090.npy')
    a = np.load(bad)
    a[1, 50] = np.nan
    np.save(bad, a)
    with pytest.raises(ValueError, match=r"vidB_000090\.npy: non-finite"):
        cb.build_clips(root, 'kp_f32', write=False)


def test_end_to_end_clips_statistics_dataset_and_one_train_step(tmp_path):
    from speechdrivestemplates_amd.config import get_cfg_defaults
    from speechdrivestemplates_amd.core.datasets.gesture_dataset import DeviceClipStore, GestureDataset
    from speechdrivestemplates_amd.core.pipelines import get_pipeline
    from speechdrivestemplates_amd.speaker_stats import compute_speaker_stats, save_speaker_stats
    sp = 'kp_f32'
    root, model_root = str(tmp_path / "data"), str(tmp_path / "model")
    S.write_speaker(root, sp)
    res = cb.build_clips(root, sp)
    base = os.path.join(root, sp)
    for name in ('processed_137.csv', 'clips.csv', os.path.join('tmp', 'intermediate_csv', 'tmp_vidA.csv')):
        assert os.path.exists(os.path.join(base, name))
    import pandas as pd
    df = pd.read_csv(os.path.join(base, 'processed_137.csv'))
    ref = pd.read_csv(os.path.join(base, 'clips.csv'))
    assert list(df.columns) == cb.COLUMNS and list(df['pose_fn']) == list(res['table']['pose_fn']) == list(ref['pose_fn'])
    assert set(df['dataset']) <= {'train', 'idle', 'dev'} and set(ref['dataset']) <= {'train', 'idle', 'val'}
    # the contract model's clips, as files, under a second root with the same csv
    os.makedirs(os.path.join(model_root, sp, 'clips', 'npz'))
    shutil.copy(os.path.join(base, 'processed_137.csv'), os.path.join(model_root, sp, 'processed_137.csv'))
    dev = cb.build_clips(root, sp, write=False)
    pos = 0
    for video in S.SPEAKERS[sp][1]:
        starts, poses, audio, _, _ = model_clips(video, 'float32', 1)
        for i, s in enumerate(starts):
            rel = cb.clip_relpath(sp, video, s, S.FRAMES)
            with np.load(os.path.join(base, rel)) as z:
                assert z['pose'].dtype == np.float32 and np.array_equal(z['pose'], poses[i]) and np.array_equal(z['audio'], audio[i])
                assert list(z['imgs']) == list(cb.frame_image_paths(root, sp, video, s, S.FRAMES))
                # write=False returns what the files hold
                assert np.array_equal(dev['poses'][pos].cpu().numpy(), z['pose'])
                n = int(dev['audio_lengths'][pos])
                assert n == len(z['audio']) and np.array_equal(dev['audio'][pos, :n].cpu().numpy(), z['audio'])
            np.savez(os.path.join(model_root, sp, rel), pose=poses[i], audio=audio[i])
            pos += 1
    assert pos == len(df)
    stats = compute_speaker_stats(root, sp, csv='processed_137.csv', num_chunks=2, scale_like='oliver')
    path = save_speaker_stats(str(tmp_path / "stat.npz"), stats)
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(os.path.dirname(GOLDEN), "..", "configs", "voice2pose_sdt_bp.yaml"))
    cfg.merge_from_list(["DATASET.ROOT_DIR", root, "DATASET.SPEAKER", sp, "DATASET.SPEAKER_STAT_FILE", path,
                         "TRAIN.BATCH_SIZE", 4, "TEST.BATCH_SIZE", 4, "SYS.NUM_WORKERS", 0, "SYS.LOG_INTERVAL", 10 ** 9,
                         "TRAIN.SAVE_VIDEO", False, "TEST.SAVE_VIDEO", False, "TEST.SAVE_NPZ", False])
    cfg.freeze()
    torch.manual_seed(0)
    pipe = get_pipeline(cfg.PIPELINE_TYPE)(cfg)
    pipe.setup_dataset(cfg, 'train')
    n_dev = int((df['dataset'] == 'dev').sum())
    for split, n in (('train', int((df['dataset'] == 'train').sum())), ('val', n_dev)):
        got, want = GestureDataset(root, sp, split, cfg), GestureDataset(model_root, sp, split, cfg)
        assert len(got) == len(want) == n  # (at 2 videos of at most 260 frames the 13 idle clips leave no validation clip)
        for i in range(n):
            a, b = got[i], want[i]
            assert torch.equal(a['poses'], b['poses']) and torch.equal(a['poses_score'], b['poses_score'])
            assert np.array_equal(a['audio'], b['audio']) and torch.isfinite(a['poses']).all()
    store = DeviceClipStore(pipe.train_dataset)
    pipe.setup_model(cfg)
    pipe.setup_optimizer()
    pipe.model.train()
    pipe.train_step(store.batch([0, 1, 2, 3]), 1, 1, 1)
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in pipe.last_losses.values() if torch.is_tensor(v)), pipe.last_losses
    pipe.close()


def test_cli_prints_the_summary(root, capsys):
    assert cb.main(["--root", root, "--speaker", "kp_f64", "--shoulder-chunks", "3", "--no-write"]) == 0
    out = capsys.readouterr().out
    assert "video vidA: 251 frames, 247 kept, 4 dropped (1 missing), 1 shoulder frames dropped by chunking" in out
    assert "speaker kp_f64: 37 clips" in out
