"""The retime stage of the clip builder on the GPU (csrc/clip_builder.hip, clip_builder.py): device_retime against
the numpy contract model bit for bit on every synthetic track, rate, design and dtype, determinism, the untouched input, the three
properties, the refused sizes, build_clips on a speaker recorded at 30 fps (poses, audio, imgs, summary, repair behind it, 15 fps as a
no-op), one written clip through GestureDataset, and the command line."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import synth_retime_videos as V  # noqa: E402

from speechdrivestemplates_amd import clip_builder as cb  # noqa: E402

pytestmark = pytest.mark.gpu

RECORDS = ('present_t', 'valid_t', 'taps_used', 'nearest_src', 'counts')
DTYPES = {'present_t': np.uint8, 'valid_t': np.uint8, 'taps_used': np.uint8, 'nearest_src': np.int32, 'counts': np.int64}


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    r = str(tmp_path_factory.mktemp("retime_videos"))
    for sp in V.SPEAKERS:
        V.write_speaker(r, sp)
        V.write_speaker(r, sp, every=2, name=sp + '_15')  # the same wavs next to every second frame: keypoints at 15 fps
    return r


def on_device(a, present):
    return torch.from_numpy(a).cuda(), torch.from_numpy(np.asarray(present).astype(np.uint8)).cuda()


def host(o):
    return {k: o[k].cpu().numpy() for k in ('src_t',) + RECORDS}


@pytest.mark.parametrize("p,q", V.RATES)
@pytest.mark.parametrize("video", V.TRACKS)
def test_device_retime_equals_the_model_bit_for_bit(video, p, q):
    for dtype in ('float32', 'float64'):
        a, present = V.video_frames(video, dtype)
        src, pres = on_device(a, present)
        for mode in V.MODES:
            want = cb.model_retime(a, present, p, q, mode)
            o = cb.device_retime(src, pres, (p, q), mode)
            again = cb.device_retime(src, pres, '%d/%d' % (p, q), mode, 0.75)
            torch.cuda.synchronize()
            got, got2 = host(o), host(again)
            assert o['src_t'].dtype == src.dtype and o['src_t'].data_ptr() != src.data_ptr() and (o['P'], o['Q'], o['mode']) == (p, q, mode)
            assert got['src_t'].shape == want['src_t'].shape
            assert got['src_t'].tobytes() == want['src_t'].tobytes(), (dtype, mode, int((got['src_t'] != want['src_t']).sum()))
            for k in RECORDS:
                assert got[k].dtype == DTYPES[k], k
                assert np.array_equal(got[k], want[k].astype(DTYPES[k])), (dtype, mode, k)
            for k in ('src_t',) + RECORDS:
                assert got[k].tobytes() == got2[k].tobytes(), (dtype, mode, k)
            assert o['phases'] == cb.model_retime_plan(a.shape[0], p, q)['phases']
        assert src.cpu().numpy().tobytes() == a.tobytes() and np.array_equal(pres.cpu().numpy(), present.astype(np.uint8))  # read only


@pytest.mark.parametrize("dtype", ['float32', 'float64'])
def test_properties_hold_on_the_device(dtype):
    for video in ('t7', 't64', 't257'):
        a, present = V.video_frames(video, dtype)
        src, pres = on_device(a, present)
        valid = cb.model_valid(a, present)
        for rho in (2, 4):  # an integer ratio: nearest and linear pick source frame rho * j wherever it is valid
            m = np.repeat(valid[::rho][:, None, :], 3, axis=1)
            for mode in ('nearest', 'linear'):
                got = host(cb.device_retime(src, pres, 15 * rho, mode))
                assert got['src_t'][m].tobytes() == a[::rho][m].tobytes() and (got['src_t'][~m] == 0).all()
                assert np.array_equal(got['valid_t'].astype(bool), valid[::rho])
        z = V.clean(a, present)
        zsrc, _ = on_device(z, present)
        for mode in V.MODES:  # 15 fps: every design gives the input back
            got = host(cb.device_retime(zsrc, pres, '15/1', mode))
            assert got['src_t'].tobytes() == z.tobytes() and np.array_equal(got['present_t'], present.astype(np.uint8))
            assert np.array_equal(got['nearest_src'], np.arange(len(z)))


def test_unsupported_sizes_raise_value_error():
    a, present = V.video_frames('t7', 'float32')
    src, pres = on_device(a, present)
    with pytest.raises(ValueError, match="frame count"):
        cb.device_retime(src[:0], pres[:0], 30)
    for fps in (241, '1/2', (1 << 20) + 1, '16385/16384'):
        with pytest.raises(ValueError, match="fps"):
            cb.device_retime(src, pres, fps)
    with pytest.raises(ValueError, match="fps must be an exact fraction"):
        cb.device_retime(src, pres, 29.97)
    with pytest.raises(ValueError, match="mode"):
        cb.device_retime(src, pres, 30, 'cubic')
    for s in (0.0, 1.25):
        with pytest.raises(ValueError, match="min_support"):
            cb.device_retime(src, pres, 30, 'linear', s)
    torch.cuda.synchronize()


def model_speaker(sp, mode='linear', min_support=0.75, max_gap=0):
    """per video of the speaker: the model pipeline -- model_retime, model_repair if asked for, then the existing models"""
    dtype, videos, start, (p, q) = V.SPEAKERS[sp]
    out = {}
    for video in videos:
        a, present = V.video_frames(video, dtype)
        rt = cb.model_retime(a, present, p, q, mode, min_support)
        src, pres = rt['src_t'], rt['present_t']
        keep0, _ = cb.model_frame_flags(src, pres)
        rep = None
        if max_gap:
            rep = cb.model_repair(src, pres, max_gap)
            src, pres = rep['src_r'], rep['present_r']
        keep, dist = cb.model_frame_flags(src, pres)
        means, _ = cb.model_shoulder_means(dist[keep], 1)
        scalar = cb.model_scalar(means)
        starts = cb.model_clip_starts(keep, start, V.FRAMES)
        scaled = cb.model_scale(src, scalar, True)
        out[video] = dict(starts=starts, starts0=cb.model_clip_starts(keep0, start, V.FRAMES), rt=rt, rep=rep, scalar=scalar, keep=keep,
                          n_src=a.shape[0], summary=cb.model_retime_summary(rt, a.shape[0], p, q, mode),
                          poses=np.stack([scaled[s:s + V.FRAMES] for s in starts]) if starts else np.zeros((0, V.FRAMES, 3, 137), a.dtype))
    return out


@pytest.mark.parametrize("sp,mode", [('rt_f32', 'linear'), ('rt_f64', 'smooth'), ('rt_f32', 'nearest')])
def test_build_clips_at_30_fps_equals_the_model_pipeline(root, sp, mode):
    start = V.SPEAKERS[sp][2]
    res = cb.build_clips(root, sp, start_frame=start, num_frames=V.FRAMES, write=False, source_fps=30, retime=mode)
    want = model_speaker(sp, mode)
    row = 0
    for video in V.SPEAKERS[sp][1]:
        w, v = want[video], res['videos'][video]
        n = len(w['starts'])
        assert n > 0 and v['retime'] == w['summary'] and v['scalar'] == w['scalar'] and v['kept'] == int(w['keep'].sum())
        assert v['frames'] == w['summary']['frames'] == (w['n_src'] - 1) // 2 + 1 and v['retime']['source_frames'] == w['n_src']
        assert v['missing'] == int((~w['rt']['present_t']).sum())
        assert 'retime' in v['timing']['kernel_ms'] and 'flags' in v['timing']['kernel_ms']
        assert res['poses'][row:row + n].cpu().numpy().tobytes() == w['poses'].tobytes()
        table = res['table'][res['table']['interval_id'] == video]
        assert sorted(table['start']) == w['starts']
        row += n
    assert row == len(res['table']) == res['poses'].shape[0]
    assert res['videos']['sa']['retime']['nonfinite_in'] == 1 and res['videos']['sa']['retime']['points_invalid_in'] > 2 * 137


@pytest.mark.parametrize("sp", ['rt_f32', 'rt_f64'])
def test_audio_is_that_of_the_15_fps_build_and_15_fps_launches_nothing(root, sp):
    start = V.SPEAKERS[sp][2]
    kw = dict(start_frame=start, num_frames=V.FRAMES, write=False)
    at30 = cb.build_clips(root, sp, source_fps=(30, 1), retime='linear', **kw)
    at15 = cb.build_clips(root, sp + '_15', **kw)  # the same wavs, every second frame as 15 fps keypoints
    assert len(at30['table']) == len(at15['table']) > 0 and list(at30['table']['start']) == list(at15['table']['start'])
    for k in ('audio', 'audio_lengths', 'poses'):
        assert at30[k].shape == at15[k].shape and at30[k].cpu().numpy().tobytes() == at15[k].cpu().numpy().tobytes(), k
    same = cb.build_clips(root, sp + '_15', source_fps='15/1', retime='smooth', **kw)  # P == 15 Q: the stage is not launched
    assert sorted(same) == sorted(at15) and same['table'].equals(at15['table']) and np.array_equal(same['order'], at15['order'])
    for k in ('poses', 'audio', 'audio_lengths'):
        assert same[k].dtype == at15[k].dtype and same[k].cpu().numpy().tobytes() == at15[k].cpu().numpy().tobytes(), k
    for video, v in same['videos'].items():
        assert 'retime' not in v and 'retime' not in v['timing']['kernel_ms']
        assert {k: x for k, x in v.items() if k != 'timing'} == {k: x for k, x in at15['videos'][video].items() if k != 'timing'}


def test_repair_behind_the_retime_fills_a_dropout_that_retiming_preserved(root):
    sp = 'rt_f32'
    start = V.SPEAKERS[sp][2]
    res = cb.build_clips(root, sp, start_frame=start, num_frames=V.FRAMES, write=False, source_fps='30', repair_max_gap=1)
    want = model_speaker(sp, max_gap=1)
    w, v = want['sa'], res['videos']['sa']
    assert not w['rt']['valid_t'][20, 110] and w['rep']['filled'][20, 110]  # source frame 40 of keypoint 110: kept by the retime, then filled
    assert v['repair']['points_filled'] == int(w['rep']['filled'].sum()) >= 7
    assert v['repair']['clips_without_repair'] == len(w['starts0']) < v['repair']['clips_with_repair'] == len(w['starts'])
    n = len(w['starts'])
    assert res['poses'][:n].cpu().numpy().tobytes() == w['poses'].tobytes() and v['retime'] == w['summary']
    assert sorted(res['table'][res['table']['interval_id'] == 'sa']['start']) == w['starts']


def test_written_clip_names_source_frames_and_loads_through_the_dataset(tmp_path):
    from speechdrivestemplates_amd.config import get_cfg_defaults
    from speechdrivestemplates_amd.core.datasets import gesture_dataset as gd
    sp = 'rt_f32'
    root = str(tmp_path)
    V.write_speaker(root, sp, frame_files=True)
    res = cb.build_clips(root, sp, start_frame=V.SPEAKERS[sp][2], num_frames=V.FRAMES, source_fps=30)
    assert list(res['table'].columns) == cb.COLUMNS and 'retime' in res['videos']['sb']
    want = model_speaker(sp)
    for video in ('sa', 'sb'):
        s = want[video]['starts'][-1]
        with np.load(os.path.join(root, sp, cb.clip_relpath(sp, video, s, V.FRAMES))) as z:
            assert sorted(z.files) == ['audio', 'imgs', 'pose'] and z['pose'].tobytes() == want[video]['poses'][-1].tobytes()
            imgs = [str(p) for p in z['imgs']]
        assert imgs == [os.path.join(root, sp, 'frames', video, '%s_%06d.jpg' % (video, 2 * (s + i))) for i in range(V.FRAMES)]
        assert all(os.path.exists(p) for p in imgs)
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(os.path.dirname(GOLDEN), "..", "configs", "voice2pose_sdt_bp.yaml"))
    cfg.merge_from_list(["DATASET.ROOT_DIR", root, "DATASET.SPEAKER", sp, "DATASET.NUM_FRAMES", V.FRAMES])
    cfg.freeze()
    k2 = 2 * 121
    stat = {'scale_factor': 1.0, 'mean': np.zeros(k2), 'std': np.ones(k2)}
    gd.register_speaker_stat(sp, parted=dict(stat), global_=dict(stat))
    ds = gd.GestureDataset(root, sp, 'train', cfg)
    s = want['sa']['starts'][0]
    rows = [i for i in range(len(ds)) if ds.clips.iloc[i]['interval_id'] == 'sa' and int(ds.clips.iloc[i]['start']) == s]
    assert len(rows) == 1
    item = ds[rows[0]]
    assert item['poses_score'].shape == (V.FRAMES, 2, 121) and np.isfinite(item['poses_score'].numpy()).all()


def test_cli_prints_the_source_rate_and_the_frame_counts(root, capsys):
    sp = 'rt_f32'
    assert cb.main(["--root", root, "--speaker", sp, "--start-frame", str(V.SPEAKERS[sp][2]), "--frames", str(V.FRAMES), "--no-write",
                    "--source-fps", "30000/1001", "--retime", "smooth", "--retime-min-support", "0.5"]) == 0
    out = capsys.readouterr().out
    for video, n_src in (('sa', 330), ('sb', 270)):
        n_out = cb.model_retime_plan(n_src, 30000, 1001)['n_out']
        line = [ln for ln in out.splitlines() if ln.startswith('video %s:' % video)]
        assert len(line) == 1 and 'source 30000/1001 fps: %d -> %d frames' % (n_src, n_out) in line[0]
    assert re.search(r"video sb: 135 frames, .* source 30000/1001 fps: 270 -> 135 frames \(smooth", out)
