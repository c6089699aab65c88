"""Speaker statistics on the GPU (csrc/speaker_stats.hip, speaker_stats.py) against the reference's own
4_1 / 4_2 functions recorded in tests/golden/speaker_stats_reference.npz: bitwise equality (np.array_equal on float64), for every
case, window size and read path; the loud failures; and a custom speaker trained end to end through DATASET.SPEAKER_STAT_FILE."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import synth_speaker_stats as S  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "speaker_stats_reference.npz")
_Z = []


def fx():
    if not _Z:
        _Z.append(np.load(FIXTURE))
    return _Z[0]


@pytest.fixture(scope="module")
def speakers(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("speakers"))
    for sp in S.SPEAKERS:
        S.write_named(root, sp)
    return root


def compute(root, case, **kw):
    from speechdrivestemplates_amd.speaker_stats import compute_speaker_stats
    sp, C = S.CASES[case]
    return compute_speaker_stats(root, sp, num_chunks=C, scale_factor=1.0, **kw)


def assert_fixture_bits(st, case):
    z = fx()
    for m, i in (('parted', 0), ('global', 1)):
        for what, t137 in (('mean', st['mean137']), ('std', st['std137'])):
            want = z['%s/%s_%s' % (case, m, what)]
            assert st[m][what].dtype == np.float64 and np.array_equal(st[m][what], want), \
                (case, m, what, int(np.sum(st[m][what] != want)), float(np.max(np.abs(st[m][what] - want))))
            assert np.array_equal(t137[i], z['%s/%s_%s137' % (case, m, what)]), (case, m, what, '137')
    assert st['clips_used'] == int(z[case + '/clips_used']) and st['clips_dropped'] == int(z[case + '/clips_dropped'])


@pytest.mark.parametrize("case", [c for c in sorted(S.CASES) if not c.startswith("zero")])
def test_statistics_equal_the_reference_bits(speakers, case):
    st = compute(speakers, case)
    assert_fixture_bits(st, case)
    # detections: the lower body is never seen, ONE_CHUNK_KP is missing from two clips only
    assert (st['counts'][:, S.LOWER_BODY] == 0).all()
    assert 0 < st['counts'][1, S.ONE_CHUNK_KP] < st['counts'][1, 0]


@pytest.mark.parametrize("case", ["f64_c3", "f32_c3", "f64_c10"])
@pytest.mark.parametrize("window,budget", [(1, None), (7, None), (10 ** 6, None), (1, 0), (7, 0), (3, 0)])
def test_window_size_and_reread_path_give_the_same_bits(speakers, case, window, budget):
    kw = {'window': window}
    if budget is not None:
        kw['device_budget_bytes'] = budget
    st = compute(speakers, case, **kw)
    assert st['timing']['resident'] == (budget is None)
    assert_fixture_bits(st, case)


def test_zero_std_raises_unless_allowed(speakers):
    from speechdrivestemplates_amd.speaker_stats import KEPT_137
    with pytest.raises(ValueError, match=r"zero std .*keypoint 15 of 137 \(%d of 121\), 0 detections" % KEPT_137.index(15)):
        compute(speakers, "zero_c3")
    st = compute(speakers, "zero_c3", allow_zero_std=True)
    assert_fixture_bits(st, "zero_c3")
    k = KEPT_137.index(15)
    assert st['global']['std'][k] == 0.0 and st['global']['std'][121 + k] == 0.0 and st['counts'][1, 15] == 0


def test_nan_clip_raises_naming_the_file(tmp_path):
    from speechdrivestemplates_amd.speaker_stats import compute_speaker_stats, plan_speaker_stats
    root = str(tmp_path)
    S.write_stats_speaker(root, "nan_speaker", n_train=9, seed=9, nan_at=(5, 10, 40), audio_len=16)
    bad = plan_speaker_stats(root, "nan_speaker", num_chunks=3)['paths'][5]
    with pytest.raises(ValueError, match="%s: non-finite" % bad.replace(".", r"\.")):
        compute_speaker_stats(root, "nan_speaker", num_chunks=3, scale_factor=1.0, window=2)


def test_cli_writes_a_loadable_npz(speakers, tmp_path, capsys):
    from speechdrivestemplates_amd import speaker_stats
    from speechdrivestemplates_amd.core.datasets import gesture_dataset as gd
    out = str(tmp_path / "cli.npz")
    assert speaker_stats.main(["--root", speakers, "--speaker", "synth_f64", "--scale-like", "oliver", "--chunks", "3", "--out", out]) == 0
    assert "synth_f64: 21 clips used, 2 dropped, 3 chunks" in capsys.readouterr().out
    gd.load_speaker_stats(out, "cli_speaker")
    stp = gd.PoseTransforms().get_speaker_stat("cli_speaker", 121, True)
    assert np.array_equal(stp['mean'], fx()['f64_c3/parted_mean'])
    gd.load_builtin_speaker_stats()
    assert stp['scale_factor'] == gd.SPEAKERS_STAT_121_parted['oliver']['scale_factor']
    assert gd.PoseTransforms().get_speaker_stat("cli_speaker", 121, False)['scale_factor'] == gd.SPEAKERS_STAT_121['oliver']['scale_factor']


def test_custom_speaker_trains_with_only_the_stat_file(tmp_path):
    """compute + save the statistics of a speaker the built-in table does not know, set DATASET.SPEAKER_STAT_FILE, and run one
    voice2pose_sdt_bp train step at 4 clips and one validation step from a DeviceClipStore"""
    from speechdrivestemplates_amd.config import get_cfg_defaults
    from speechdrivestemplates_amd.core.datasets.gesture_dataset import DeviceClipStore
    from speechdrivestemplates_amd.core.pipelines import get_pipeline
    from speechdrivestemplates_amd.speaker_stats import compute_speaker_stats, save_speaker_stats
    root = str(tmp_path / "data")
    S.write_stats_speaker(root, "custom_gpu_speaker", n_train=12, seed=12)
    path = save_speaker_stats(str(tmp_path / "custom.npz"), compute_speaker_stats(root, "custom_gpu_speaker", num_chunks=3, scale_like="oliver"))
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(os.path.dirname(GOLDEN), "..", "configs", "voice2pose_sdt_bp.yaml"))
    cfg.merge_from_list(["DATASET.ROOT_DIR", root, "DATASET.SPEAKER", "custom_gpu_speaker", "DATASET.SPEAKER_STAT_FILE", path,
                         "TRAIN.BATCH_SIZE", 4, "TEST.BATCH_SIZE", 4, "SYS.NUM_WORKERS", 0, "SYS.LOG_INTERVAL", 10 ** 9,
                         "TRAIN.SAVE_VIDEO", False, "TEST.SAVE_VIDEO", False, "TEST.SAVE_NPZ", False])
    cfg.freeze()
    torch.manual_seed(0)
    pipe = get_pipeline(cfg.PIPELINE_TYPE)(cfg)
    pipe.setup_dataset(cfg, 'train')
    store = DeviceClipStore(pipe.train_dataset)
    pipe.setup_model(cfg)
    pipe.setup_optimizer()
    pipe.model.train()
    pipe.train_step(store.batch([0, 1, 2, 3]), 1, 1, 1)
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in pipe.last_losses.values() if torch.is_tensor(v)), pipe.last_losses
    pipe.model.eval()
    test_store = DeviceClipStore(pipe.test_dataset)
    losses, _ = pipe.test_step(test_store.batch(list(range(min(4, len(test_store))))), 1, epoch=1)
    assert all(torch.isfinite(v).all() for v in losses.values()), losses
    assert float(losses['L2_dist']) > 0
    pipe.close()
