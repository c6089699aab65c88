"""The audio activity gate of the clip builder on the GPU (csrc/speech_gate.hip, clip_builder.py): every stage
against its numpy contract model bit for bit at the shapes where a kernel can go wrong (hop, wave and workgroup boundaries), determinism,
the refused sizes, and build_clips on a synthetic speaker whose track puts windows exactly on the min_permille boundary."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import synth_keypoint_videos as K  # noqa: E402
import synth_speech_gate as S  # noqa: E402

from speechdrivestemplates_amd import clip_builder as cb  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------------------ energies
@pytest.mark.parametrize("n", S.SIZES_ENERGY)
def test_hop_energy_equals_the_model_bit_for_bit(n):
    x = S.track(n)
    e, flag = cb.device_hop_energy(dev(x))
    e2, flag2 = cb.device_hop_energy(dev(x))
    want = cb.model_hop_energy(x)
    got = e.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (n // 160,) and int(flag.item()) == 0 and int(flag2.item()) == 0
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    assert np.array_equal(bits(got), bits(e2.cpu().numpy()))


def test_non_finite_samples_set_the_flag_and_touch_no_other_hop():
    """the finite hops keep their bits; the hit hop is NaN on both sides (inf and NaN in one sum), its payload is not part of the contract"""
    x = S.track(160 * 6 + 3)
    clean = cb.model_hop_energy(x)
    x[160 * 4 + 50], x[160 * 4 + 90] = np.nan, np.inf
    e, flag = cb.device_hop_energy(dev(x))
    got, want = e.cpu().numpy(), cb.model_hop_energy(x)
    ok = np.arange(6) != 4
    assert int(flag.item()) == 1 and np.isnan(got[4]) and np.isnan(want[4])
    assert np.array_equal(bits(got[ok]), bits(want[ok])) and np.array_equal(bits(got[ok]), bits(clean[ok]))
    x[160 * 4 + 50] = 0.25  # the inf alone
    e, flag = cb.device_hop_energy(dev(x))
    assert int(flag.item()) == 1 and np.array_equal(bits(e.cpu().numpy()[ok]), bits(clean[ok]))
    assert np.array_equal(np.isinf(e.cpu().numpy()), np.isinf(cb.model_hop_energy(x)))


# -------------------------------------------------------------------------------------------------------------------- floor and mask
@pytest.mark.parametrize("h", [1, 2, 63, 64, 65, 4097])
def test_floor_and_mask_equal_the_models(h):
    for kind in ('random', 'ties', 'equal'):
        e = S.energies(h, kind)
        e_dev = dev(e)
        for pct in (0, 50, 10):
            f = cb.model_floor(e, pct)
            for margin, abs_floor in ((10 ** 1.2, 160e-6), (1.0, 0.0), (10 ** 0.3, 1e-300)):
                want, thr = cb.model_mask(e, f, margin, abs_floor)
                raw, stats = cb.device_speech_mask(e_dev, pct, margin, abs_floor)
                raw2, stats2 = cb.device_speech_mask(e_dev, pct, margin, abs_floor)
                s = stats.cpu().numpy()
                assert np.array_equal(bits(s), bits([f, thr])), (kind, pct, margin, s, f, thr)
                assert raw.dtype == torch.uint8 and np.array_equal(raw.cpu().numpy().astype(bool), want), (kind, pct, margin)
                assert torch.equal(raw, raw2) and np.array_equal(bits(s), bits(stats2.cpu().numpy()))


def test_mask_without_hops():
    raw, stats = cb.device_speech_mask(torch.empty(0, dtype=torch.float64, device='cuda'), 10, 15.8, 1e-4)
    assert raw.numel() == 0 and stats.cpu().tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------------------------------ smoothing
@pytest.mark.parametrize("h", [1, 2, 64, 65, 1025])
def test_smoothing_equals_the_model(h):
    g = np.random.Generator(np.random.PCG64(h))
    masks = [np.zeros(h, bool), np.ones(h, bool), g.random(h) < 0.5, g.random(h) < 0.1, g.random(h) < 0.95]
    for mr, hg in ((2, 2), (5, 20), (3, 7)):  # the host test's pattern across the wave (64) and workgroup (256) boundaries and both ends
        p = S.smoothing_pattern(mr, hg)
        masks += [S.laid_across(p, h, at) for at in (0, 64 - len(p) // 2, 256 - len(p) // 2, 256 - mr, 512 - hg - 1, 1024 - len(p) // 3, h - len(p))
                  if 0 <= at < h]
        masks += [~m for m in masks[-2:]]
    long_run = np.zeros(h, bool)
    long_run[1:min(h, 1025) - 0] = True  # an active run of 1024 (or to the end) and, inverted, a gap of that length
    masks += [long_run, ~long_run, np.concatenate([[True], ~long_run[1:-1], [True]]) if h > 2 else long_run]
    for m in masks:
        m_dev = dev(m.astype(np.uint8))
        for min_run, hang in ((0, 0), (1, 1), (2, 2), (5, 20), (3, 7), (1024, 0), (0, 1024), (1024, 1024), (1023, 1023)):
            want = cb.model_smooth(m, min_run, hang)
            got = cb.device_speech_smooth(m_dev, min_run, hang)
            assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy().astype(bool), want), (h, min_run, hang, m.tolist()[:80])
        assert torch.equal(cb.device_speech_smooth(m_dev, 5, 20), cb.device_speech_smooth(m_dev, 5, 20))
        assert np.array_equal(m_dev.cpu().numpy().astype(bool), m)  # read only


# -------------------------------------------------------------------------------------------------------------------------- windows
def windows_case(active, n, starts, offs, permille):
    o = cb.device_speech_windows(dev(active.astype(np.uint8)), n, dev(np.asarray(starts, np.int32)), offs, permille)
    counts = cb.model_window_counts(active, n, offs)
    kept = cb.model_windows_kept(counts, permille)
    k = int(o['n_kept'].item())
    assert k == kept.sum()
    assert np.array_equal(o['prefix'].cpu().numpy(), np.concatenate([[0], np.cumsum(active)]).astype(np.int32))
    if len(offs):
        assert np.array_equal(o['counts_all'].cpu().numpy(), counts)
    assert np.array_equal(o['starts'][:k].cpu().numpy(), np.asarray(starts, np.int32)[kept])
    assert np.array_equal(o['index'][:k].cpu().numpy(), np.flatnonzero(kept)) and np.array_equal(o['counts'][:k].cpu().numpy(), counts[kept])
    assert (np.diff(o['starts'][:k].cpu().numpy()) > 0).all()
    return kept


def test_windows_counts_and_compaction():
    g = np.random.Generator(np.random.PCG64(3))
    h = 1500
    n = h * 160 + 77
    active = g.random(h) < 0.5
    active[200:700], active[800:1300] = True, False
    starts = np.arange(80, 80 + 5 * 700, 5)  # 700 candidates: three workgroups of the measure / pack passes
    offs = [cb.audio_offsets(int(s), 80, 64) for s in starts]
    assert any(a0 >= n for a0, _ in offs) and any(a0 < n < a1 for a0, a1 in offs) and any(a0 % 160 for a0, _ in offs)
    kept = windows_case(active, n, starts, offs, 500)
    assert 0 < kept.sum() < len(starts) and not kept[-1]  # windows past the end of the track are dropped
    assert not windows_case(active, n, [], [], 500).size                                     # no candidate
    long_h = 12000  # two minutes: the first 300 windows (two workgroups) lie inside
    assert windows_case(np.ones(long_h, bool), long_h * 160, starts[:300], offs[:300], 1000).all()        # all kept
    assert not windows_case(np.zeros(long_h, bool), long_h * 160, starts[:300], offs[:300], 1).any()      # all dropped
    assert not windows_case(np.zeros(0, bool), 159, starts[:3], offs[:3], 1).any()           # a track without a hop
    exact = np.zeros(h, bool)
    exact[::2] = True
    e_offs = [(0, 160 * 426), (160, 160 * 427), (0, 160 * 427), (1, 160 * 427), (160 * 3 + 1, 160 * 4 + 159)]
    kept = windows_case(exact, n, [80, 85, 90, 95, 100], e_offs, 500)
    assert kept.tolist() == [True, True, True, True, False]  # 213 / 426 on the boundary both ways, 214 / 427, 213 / 426, no whole hop
    assert windows_case(exact, n, [80, 85, 90, 95, 100], e_offs, 501).tolist() == [False, False, True, False, False]


# ------------------------------------------------------------------------------------------------------------------- refused sizes
def test_unsupported_sizes_are_refused_before_any_launch():
    from speechdrivestemplates_amd import _lib
    lib = _lib.load()
    big = 160 * (1 << 24) + 160
    assert lib.sdt_clip_speech_workspace_bytes(big, 0) < 0 and lib.sdt_clip_speech_workspace_bytes(-1, 0) < 0
    assert lib.sdt_clip_speech_workspace_bytes(0, (1 << 30) + 1) < 0 and lib.sdt_clip_speech_workspace_bytes(big - 1, 1 << 30) > 0
    small = torch.zeros(64, dtype=torch.float64, device='cuda')
    p = C.c_void_p(small.data_ptr())
    torch.cuda.synchronize()
    for status in (lib.sdt_clip_speech_energy(p, big, p, p, None),
                   lib.sdt_clip_speech_mask(p, (1 << 24) + 1, 10, 15.8, 1e-4, p, p, p, 1 << 20, None),
                   lib.sdt_clip_speech_mask(p, 8, 51, 15.8, 1e-4, p, p, p, 1 << 20, None),
                   lib.sdt_clip_speech_smooth(p, (1 << 24) + 1, 5, 20, p, p, 1 << 20, None),
                   lib.sdt_clip_speech_smooth(p, 8, 1025, 20, p, p, 1 << 20, None),
                   lib.sdt_clip_speech_windows(p, big // 160, big, p, p, p, 1, 500, p, p, p, p, p, p, p, 1 << 20, None),
                   lib.sdt_clip_speech_windows(p, 1, 160, p, p, p, 1, 1001, p, p, p, p, p, p, p, 1 << 20, None)):
        assert status == -3  # SDT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (small == 0).all()  # nothing ran
    m = torch.zeros(8, dtype=torch.uint8, device='cuda')
    for call in (lambda: cb.device_speech_smooth(m, 1025, 0), lambda: cb.device_speech_smooth(m, 0, 1025), lambda: cb.device_speech_smooth(m, -1, 0),
                 lambda: cb.device_speech_mask(small, 51, 15.8, 1e-4), lambda: cb.device_speech_windows(m, 8 * 160, m.int(), [(0, 160)], 0)):
        with pytest.raises(ValueError):
            call()


# ----------------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def root(tmp_path_factory):
    r = str(tmp_path_factory.mktemp("gate_videos"))
    S.write_speaker(r)
    S.write_speaker(r, S.SPEAKER + '_w')
    K.write_speaker(r, 'kp_f32')
    return r


@pytest.fixture(scope="module")
def ungated(root):
    return cb.build_clips(root, S.SPEAKER, write=False)


def test_build_clips_with_the_gate_equals_the_model(root, ungated):
    res = cb.build_clips(root, S.SPEAKER, write=False, speech_gate=S.GATE)
    again = cb.build_clips(root, S.SPEAKER, write=False, speech_gate=dict(S.GATE))
    rows, kept_rows, counts = 0, [], []
    for video in S.VIDEOS:
        rate, pcm = S.video_audio(video)
        x = cb.model_pcm_to_mono(pcm)[cb.source_cut(K.START, rate):]
        a, present = K.video_frames(video, 'float32')
        starts = cb.model_clip_starts(cb.model_frame_flags(a, present)[0], K.START, K.FRAMES)
        g = cb.model_speech_gate(x, starts, K.START, K.FRAMES, S.GATE)
        assert res['videos'][video]['speech_gate'] == g['summary'] and ungated['videos'][video].get('speech_gate') is None
        assert sum(res['videos'][video]['clips'].values()) == g['kept'].sum() and res['videos'][video]['audio_samples'] == len(x)
        kept_rows += [rows + i for i in np.flatnonzero(g['kept'])]
        counts.append(g['counts'])
        rows += len(starts)
    kept_rows = np.array(kept_rows)
    assert 0 < len(kept_rows) < rows == ungated['poses'].shape[0]
    assert np.array_equal(res['speech_counts'].cpu().numpy(), np.concatenate(counts)) and res['speech_counts'].dtype == torch.int32
    c = np.concatenate(counts).astype(np.int64)
    assert (1000 * c[:, 0] == 500 * c[:, 1]).any()  # a kept window exactly on the boundary
    # poses and audio of the kept windows: the very rows of the ungated build
    assert res['poses'].cpu().numpy().tobytes() == ungated['poses'][kept_rows].cpu().numpy().tobytes()
    assert torch.equal(res['audio_lengths'], ungated['audio_lengths'][kept_rows])
    width = res['audio'].shape[1]
    assert res['audio'].cpu().numpy().tobytes() == ungated['audio'][kept_rows][:, :width].contiguous().cpu().numpy().tobytes()
    by_clip = ungated['table'].assign(_row=ungated['order'])
    want = by_clip[by_clip['_row'].isin(kept_rows)]
    assert sorted(res['table']['pose_fn']) == sorted(want['pose_fn']) and list(res['table'].columns) == cb.COLUMNS
    assert np.array_equal(np.sort(res['order']), np.arange(len(kept_rows)))
    # the split runs over the kept clips
    for video in S.VIDEOS:
        n = (res['table']['interval_id'] == video).sum()
        assert res['videos'][video]['clips'] == {lab: cb.split_labels(n).count(lab) for lab in ('train', 'idle', 'dev')}
    for k in ('poses', 'audio', 'audio_lengths', 'speech_counts'):
        assert torch.equal(res[k], again[k]), k
    assert all(k.startswith('gate_') or k in ungated['videos'][v]['timing']['kernel_ms'] for v in S.VIDEOS
               for k in res['videos'][v]['timing']['kernel_ms'])


def test_written_speaker_has_sidecars_and_loads(root):
    name = S.SPEAKER + '_w'
    res = cb.build_clips(root, name, speech_gate=S.GATE)
    base = os.path.join(root, name)
    assert os.path.exists(res['files']['processed_137.csv']) and os.path.exists(res['files']['clips.csv'])
    n_files = len(os.listdir(os.path.join(base, 'clips', 'npz')))
    assert n_files == len(res['table']) == sum(v['speech_gate']['kept'] for v in res['videos'].values())
    for video in S.VIDEOS:
        assert os.path.exists(os.path.join(base, 'tmp', 'intermediate_csv', 'tmp_%s.csv' % video))
        z = np.load(os.path.join(base, 'tmp', 'activity', video + '.npz'))
        g = res['videos'][video]['speech_gate']
        assert set(z.files) == {'energy', 'active_raw', 'active', 'starts_all', 'counts_all'}
        assert len(z['energy']) == g['hops'] and z['active'].sum() == g['active'] and z['active_raw'].sum() == g['active_raw']
        assert len(z['starts_all']) == g['windows'] == len(z['counts_all']) and cb.model_windows_kept(z['counts_all'], 500).sum() == g['kept']
    from speechdrivestemplates_amd.config import get_cfg_defaults
    from speechdrivestemplates_amd.core.datasets.gesture_dataset import GestureDataset, register_configured_speaker_stats
    from speechdrivestemplates_amd.speaker_stats import compute_speaker_stats, save_speaker_stats
    stats = compute_speaker_stats(root, name, csv='processed_137.csv', num_chunks=2, scale_like='oliver')
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(os.path.dirname(GOLDEN), "..", "configs", "voice2pose_sdt_bp.yaml"))
    cfg.merge_from_list(['DATASET.ROOT_DIR', root, 'DATASET.SPEAKER', name, 'DATASET.SPEAKER_STAT_FILE',
                         save_speaker_stats(os.path.join(root, 'gate_stat.npz'), stats)])
    cfg.freeze()
    assert register_configured_speaker_stats(cfg)
    ds = GestureDataset(root, name, 'train', cfg)
    assert len(ds) == (res['table']['dataset'] == 'train').sum() > 0
    for i in range(len(ds)):
        assert torch.isfinite(ds[i]['poses']).all() and len(ds[i]['audio']) > 0


def test_gate_off_is_byte_identical(root, tmp_path):
    assert inspect.signature(cb.build_clips).parameters['speech_gate'].default is None
    a = cb.build_clips(root, 'kp_f32', write=False)
    b = cb.build_clips(root, 'kp_f32', write=False, speech_gate=None)
    for k in ('poses', 'audio', 'audio_lengths'):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    assert a['table'].equals(b['table']) and 'speech_counts' not in b and set(a) == set(b)
    assert all(list(a['videos'][v]['timing']['kernel_ms']) == list(b['videos'][v]['timing']['kernel_ms']) and 'speech_gate' not in b['videos'][v]
               for v in a['videos'])
    trees = []
    for i, kw in enumerate(({}, {'speech_gate': None})):
        r = str(tmp_path / ('r%d' % i))
        K.write_speaker(r, 'kp_f32')
        cb.build_clips(r, 'kp_f32', **kw)
        files = {}
        for d, _, names in os.walk(os.path.join(r, 'kp_f32')):
            for fn in names:
                p = os.path.join(d, fn)
                if fn.endswith('.npz'):  # (a zip's bytes hold timestamps: compare the members)
                    z = np.load(p)
                    files[os.path.relpath(p, r)] = {k: z[k].tobytes() for k in z.files if k != 'imgs'}
                else:
                    files[os.path.relpath(p, r)] = open(p, 'rb').read()
        trees.append(files)
    assert trees[0] == trees[1] and not any('activity' in p for p in trees[1])


def test_activity_report_prints_one_wav(root, capsys):
    wav = os.path.join(root, S.SPEAKER, 'audio_full', 'vidB.wav')
    got = cb.activity_report(wav, S.GATE)
    rate, pcm = S.video_audio('vidB')
    want = cb.model_speech_gate(cb.model_pcm_to_mono(pcm), [], K.START, K.FRAMES, S.GATE)['summary']  # from the first sample, no windows
    assert got == want and got['hops'] == len(pcm) // 160 and 0 < got['active'] < got['hops']
    assert cb.main(['--activity-report', wav, '--gate-hang-ms', '10', '--gate-min-ms', '20']) == 0
    out = capsys.readouterr().out
    assert wav in out and '%d of %d hops active' % (got['active'], got['hops']) in out and 'threshold' in out
