"""GPU skeleton renderer (csrc/render.hip, render.py, video.py) against the reference's recorded cv2.line calls
(tests/golden/skeleton_calls_reference.npz) and the float64 contract rasterizer of tests/test_render_host.py, plus the pipeline
wiring: Trainer.demo / test / train with SYS.RENDER_VIDEO on and off.  Explicit bars, no margins file."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_render_host import FIXTURE, fixture_strokes, raster_contract

pytestmark = pytest.mark.gpu

CASES = {"clip": "clip", "clip_odd": "clip", "pair": "pair", "long36": "long", "long64": "long", "long360": "long"}
_Z = []
_CONTRACT = {}


def fx():
    if not _Z:
        _Z.append(np.load(FIXTURE))
    return _Z[0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def render_case(case, poses=None):
    from speechdrivestemplates_amd import render
    z = fx()
    H, W = (int(v) for v in z[case + "/canvas"])
    p = dev(z[case + "/poses"] if poses is None else poses)
    s = float(z["scaling"])
    if CASES[case] == "clip":
        return render.render_pose_clip(p, (H, W), s).cpu().numpy()
    if CASES[case] == "pair":
        return render.render_pose_pair_clip(p, dev(z[case + "/gt"]), (H, W), s).cpu().numpy()
    return render.render_long_image(p).cpu().numpy()[None]


def contract_case(case, drop=None):
    """the contract rasterizer on the reference's calls -> [(image, reach, full)] per image; drop: {image: set of call indices}"""
    key = (case, None if drop is None else tuple(sorted((k, tuple(sorted(v))) for k, v in drop.items())))
    if key not in _CONTRACT:
        z = fx()
        H, W = (int(v) for v in z[case + "/canvas"])
        out = []
        for image, strokes in sorted(fixture_strokes(z, case).items()):
            keep = [s for i, s in enumerate(strokes) if drop is None or i not in drop.get(image, ())]
            out.append(raster_contract(H, W, keep, return_reach=True))
        _CONTRACT[key] = out
    return _CONTRACT[key]


def check_frames(got, want, what):
    """bars: untouched pixels exactly 255, pixels fully inside the topmost stroke exactly its colour, |diff| <= 1 everywhere and
    nonzero on at most 0.1 % of the touched pixels"""
    assert got.shape[0] == len(want), (what, got.shape, len(want))
    touched = differ = 0
    for i, (img, reach, full) in enumerate(want):
        g = got[i]
        assert g.shape == img.shape, (what, g.shape, img.shape)
        assert (g[~reach] == 255).all(), "%s image %d: %d untouched pixels are not background" % (what, i, int((g[~reach] != 255).any(-1).sum()))
        assert (g[full] == img[full]).all(), "%s image %d: fully covered pixels differ" % (what, i)
        d = np.abs(g.astype(np.int16) - img.astype(np.int16))
        assert d.max() <= 1, "%s image %d: max |diff| %d at %s" % (what, i, d.max(), np.unravel_index(d.argmax(), d.shape))
        touched += int(reach.sum())
        differ += int((d.max(-1) > 0).sum())
    assert differ <= 1e-3 * touched, "%s: %d of %d touched pixels differ by 1 LSB" % (what, differ, touched)
    return differ, touched


# -- (a) the stroke table is the reference's calls, exactly ------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_stroke_table_equals_the_reference_calls(case):
    from speechdrivestemplates_amd import render
    from test_render_host import cv2_colour
    z = fx()
    calls = z[case + "/calls"].astype(np.int64)
    H, W = (int(v) for v in z[case + "/canvas"])
    view = CASES[case]
    tab = render.stroke_table(view, dev(z[case + "/poses"]), dev(z[case + "/gt"]) if view == "pair" else None, (H, W), float(z["scaling"]))
    assert tab["canvas"] == (H, W)
    n = len(calls)
    assert len(tab["endpoints"]) == n and tab["drawn"].all() and tab["skipped"] == 0
    assert (tab["image"] == calls[:, 0]).all()
    x_off = calls[:, 1]
    assert (tab["endpoints"] == np.stack([calls[:, 4] + x_off, calls[:, 5], calls[:, 6] + x_off, calls[:, 7]], 1)).all()
    assert (tab["colour"] == cv2_colour(z[case + "/colour"])).all()
    assert (tab["thickness"] == calls[:, 8]).all()
    assert (tab["clip"] == np.stack([x_off, x_off + calls[:, 3]], 1)).all()


# -- (b) frames against the contract rasterizer ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_frames_match_the_contract(case):
    check_frames(render_case(case), contract_case(case), case)


def test_batched_launches_match_single_ones():
    from speechdrivestemplates_amd import render
    z = fx()
    p = dev(z["clip/poses"]).reshape(2, 4, 2, 121)
    got = render.render_pose_clip(p, (720, 1280), float(z["scaling"])).cpu().numpy()
    assert got.shape == (2, 4, 720, 1280, 3)
    check_frames(got.reshape(8, 720, 1280, 3), contract_case("clip"), "clip batch 2x4")
    p = dev(np.stack([z["long36/poses"], z["long36/poses"]]))
    got = render.render_long_image(p).cpu().numpy()
    assert got.shape == (2, 720, 2975, 3)
    check_frames(got, contract_case("long36") * 2, "long36 batch 2")
    p, g = dev(z["pair/poses"]), dev(z["pair/gt"])
    got = render.render_pose_pair_clip(p.float(), g.float(), (720, 1280), float(z["scaling"]))  # float32 input is widened first
    assert got.dtype == torch.uint8 and got.is_cuda and got.shape == (6, 720, 1280, 3)


# -- (c) non-finite / huge keypoints ------------------------------------------------------------------------------------------
def test_nonfinite_keypoints_drop_their_edges_only():
    from speechdrivestemplates_amd import render
    z = fx()
    p = np.array(z["clip/poses"][:2])
    p[0, 0, 100] = np.nan   # right-hand wrist: the first edge of each of the 5 fingers
    p[1, 1, 50] = 1e30      # face keypoint 41: edges [40, 41] and [41, 36] of the right eye
    render._warned[0] = False
    with pytest.warns(UserWarning, match="not drawn"):
        got = render.render_pose_clip(dev(p), (720, 1280), float(z["scaling"])).cpu().numpy()
    assert render.last_skipped == 7
    tab = render.stroke_table("clip", dev(p))
    assert tab["skipped"] == 7 and (~tab["drawn"]).sum() == 7
    drop = {}
    for i in np.flatnonzero(~tab["drawn"]):
        drop.setdefault(int(tab["image"][i]), set()).add(int(i % 108))
    assert sorted(len(v) for v in drop.values()) == [2, 5]
    check_frames(got, contract_case("clip", drop)[:2], "clip with NaN / 1e30")
    # away from the dropped edges the frames are what the clean poses give
    clean = render_case("clip")[:2]
    strokes = fixture_strokes(z, "clip")
    for i in range(2):
        gone = [s for j, s in enumerate(strokes[i]) if j in drop[i]]
        _, near, _ = raster_contract(720, 1280, [s[:5] + (s[5] + 2,) + s[6:] for s in gone], return_reach=True)  # 1 px margin
        assert near.any() and (got[i][~near] == clean[i][~near]).all()
        assert (got[i][near] != clean[i][near]).any()


def test_render_refuses_cpu_tensors_and_graph_capture():
    from speechdrivestemplates_amd import render
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render.render_pose_clip(torch.zeros(2, 2, 121, dtype=torch.float64))
    x = torch.zeros(2, 2, 121, dtype=torch.float64, device="cuda")
    real = torch.cuda.is_current_stream_capturing
    torch.cuda.is_current_stream_capturing = lambda: True  # (no real capture is opened for a call that must refuse before any launch)
    try:
        with pytest.raises(RuntimeError, match="capture"):
            render.render_pose_clip(x)
    finally:
        torch.cuda.is_current_stream_capturing = real


# -- (d)-(f) pipelines ---------------------------------------------------------------------------------------------------------
def _demo(tmp_path, render_on):
    from scipy.io import wavfile

    from speechdrivestemplates_amd.config import get_cfg_defaults
    from speechdrivestemplates_amd.core.datasets.gesture_dataset import load_speaker_stats
    from speechdrivestemplates_amd.core.pipelines import get_pipeline
    from test_model_gpu import _make_pipeline
    load_speaker_stats(os.path.join(GOLDEN, "speaker_stat_oliver.npz"), "oliver")
    pipe, _ = _make_pipeline("voice2pose_sdt_bp", 16, 0.5)
    pipe.base_path = str(tmp_path)
    ckpt = pipe.save_checkpoint(1, 1)
    wavfile.write(str(tmp_path / "x.wav"), 16000, (np.random.default_rng(2).standard_normal(int(16000 * 2.4)) * 2000).astype(np.int16))
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(os.path.dirname(GOLDEN), "..", "configs", "voice2pose_sdt_bp.yaml"))
    opts = ["DATASET.SPEAKER", "oliver", "DEMO.CODE_INDEX", 0, "SYS.OUTPUT_DIR", str(tmp_path / "out"), "TEST.SAVE_NPZ", False,
            "TEST.SAVE_VIDEO", True, "SYS.VIDEO_FORMAT", ["mp4", "img"]]
    if render_on:
        opts += ["SYS.RENDER_VIDEO", True]
    cfg.merge_from_list(opts)
    cfg.freeze()
    demo = get_pipeline(cfg.PIPELINE_TYPE)(cfg)
    outs = demo.demo(cfg, "demo", ckpt, str(tmp_path / "x.wav"))
    demo.close()
    base = glob.glob(str(tmp_path / "out" / "*demo"))
    assert len(base) == 1
    return outs, base[0]


def test_demo_writes_long_image_and_video(tmp_path):
    from PIL import Image

    from speechdrivestemplates_amd import render
    outs, base = _demo(tmp_path, True)
    p = outs[0]["poses_pred_batch"][0]
    assert p.shape == (36, 2, 121)
    jpg = os.path.join(base, "imgs", "epoch0-DEMO-step1.jpg")
    assert os.path.exists(jpg)
    want = render.render_long_image(p).cpu().numpy()
    rgb = np.asarray(Image.open(jpg).convert("RGB")).astype(np.float64)
    assert rgb.shape == want.shape == (720, 2975, 3)
    err = rgb[..., ::-1] - want
    psnr = 10 * np.log10(255.0 ** 2 / np.mean(err ** 2))
    assert psnr > 30, psnr  # JPEG quality 95 of thin lines on white
    vids = os.path.join(base, "videos")
    assert os.path.exists(os.path.join(vids, "epoch0-DEMO-step1.wav"))
    if not os.path.exists(os.path.join(vids, "epoch0-DEMO-step1.mp4")):  # no ffmpeg on this machine: the frames stay
        frames = sorted(os.listdir(os.path.join(vids, "epoch0-DEMO-step1")))
        assert frames == ["%06d.jpg" % i for i in range(36)]


def test_demo_default_writes_no_pictures(tmp_path):
    _, base = _demo(tmp_path, False)
    assert not os.path.exists(os.path.join(base, "videos")) and not os.path.exists(os.path.join(base, "imgs"))


def _train_cfg(tmp_path, name, render_on):
    from speechdrivestemplates_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(os.path.dirname(GOLDEN), "..", "configs", name + ".yaml"))
    opts = ["DATASET.NAME", "SyntheticGestureDataset", "DATASET.SYNTHETIC_CLIPS", 8, "TRAIN.BATCH_SIZE", 4, "TEST.BATCH_SIZE", 4,
            "TRAIN.NUM_EPOCHS", 1, "SYS.NUM_WORKERS", 0, "SYS.LOG_INTERVAL", 100, "SYS.OUTPUT_DIR", str(tmp_path),
            "TRAIN.SAVE_VIDEO", True, "TEST.SAVE_VIDEO", True, "TEST.SAVE_NPZ", False, "TRAIN.NUM_RESULT_SAMPLE", 1,
            "TEST.NUM_RESULT_SAMPLE", 1, "SYS.VIDEO_FORMAT", ["mp4"]]
    if render_on:
        opts += ["SYS.RENDER_VIDEO", True]
    cfg.merge_from_list(opts)
    cfg.freeze()
    return cfg


def _videos(base, stem):
    d = os.path.join(base, "videos")
    return os.path.exists(os.path.join(d, stem + ".mp4")) or os.path.isdir(os.path.join(d, stem))


@pytest.mark.parametrize("name", ["voice2pose_sdt_bp", "pose2pose"])
def test_train_validate_test_write_pair_videos(tmp_path, name):
    from speechdrivestemplates_amd.core.pipelines import get_pipeline
    torch.manual_seed(3)
    cfg = _train_cfg(tmp_path, name, True)
    pipe = get_pipeline(cfg.PIPELINE_TYPE)(cfg)
    pipe.train(cfg, "r", None)  # 2 steps, saving interval 2 -> TRAIN video at step 2; validation: 2 batches -> VAL video at step 2
    base = glob.glob(str(tmp_path / "*_r"))[0]
    assert _videos(base, "epoch1-TRAIN-step2") and _videos(base, "epoch1-VAL-step2"), os.listdir(os.path.join(base, "videos"))
    if name == "voice2pose_sdt_bp":
        assert os.path.exists(os.path.join(base, "videos", "epoch1-TRAIN-step2.wav"))
        ckpt = glob.glob(os.path.join(base, "checkpoints", "*.pth"))[0]
        pipe2 = get_pipeline(cfg.PIPELINE_TYPE)(cfg)
        pipe2.test(cfg, "t", ckpt)
        pipe2.close()
        tbase = glob.glob(str(tmp_path / "*_t"))[0]
        assert _videos(tbase, "epoch0-TEST-step2")
        d = os.path.join(tbase, "videos", "epoch0-TEST-step2")
        if os.path.isdir(d):
            assert len(os.listdir(d)) == 64  # one pair frame per pose frame
    pipe.close()


def test_train_default_writes_no_videos(tmp_path):
    from speechdrivestemplates_amd.core.pipelines import get_pipeline
    cfg = _train_cfg(tmp_path, "pose2pose", False)
    pipe = get_pipeline(cfg.PIPELINE_TYPE)(cfg)
    pipe.train(cfg, "r", None)
    pipe.close()
    base = glob.glob(str(tmp_path / "*_r"))[0]
    assert not os.path.exists(os.path.join(base, "videos")) and not os.path.exists(os.path.join(base, "imgs"))
