"""Host side of the skeleton renderer (render.py, video.py): a float64 numpy rasterizer of the drawing contract,
checked on hand-computed pixels; the long-image window arithmetic against the reference's recorded calls; VideoWriter's file naming
and SYS.VIDEO_FORMAT handling without ffmpeg.  No GPU needed."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "skeleton_calls_reference.npz")


# -- the drawing contract in float64 (shared with tests/test_render_gpu.py) ----------------------------------------------------
def cv2_colour(raw):
    """cv2's Scalar -> uint8: round to nearest (ties to even, like cvRound), saturate"""
    return np.clip(np.rint(np.asarray(raw, dtype=np.float64)), 0, 255).astype(np.int64)


def raster_contract(H, W, strokes, return_reach=False):
    """strokes: iterable of (x0, y0, x1, y1, (b, g, r), thickness, clip_x0, clip_x1) in draw order, integer endpoints in canvas
    columns.  Coverage c = clamp(r + 0.5 - d, 0, 1) with r = thickness / 2 and d the distance from the pixel centre to the segment;
    each stroke blends bg + c * (colour - bg) and rounds (half up) to uint8 before the next one.  -> (H, W, 3) uint8 [, reach, full]:
    reach = pixels some stroke covers with c > 0, full = pixels the last stroke that reaches them covers with c == 1."""
    img = np.full((H, W, 3), 255.0)
    reach = np.zeros((H, W), bool)
    full = np.zeros((H, W), bool)
    for x0, y0, x1, y1, col, th, cx0, cx1 in strokes:
        g = th // 2 + 1
        lx, hx = max(min(x0, x1) - g, cx0, 0), min(max(x0, x1) + g, cx1 - 1, W - 1)
        ly, hy = max(min(y0, y1) - g, 0), min(max(y0, y1) + g, H - 1)
        if lx > hx or ly > hy:
            continue
        ys, xs = np.mgrid[ly:hy + 1, lx:hx + 1].astype(np.float64)
        ux, uy = float(x1 - x0), float(y1 - y0)
        l2 = ux * ux + uy * uy
        t = np.clip(((xs - x0) * ux + (ys - y0) * uy) / l2, 0.0, 1.0) if l2 > 0 else np.zeros_like(xs)
        d = np.hypot(xs - x0 - t * ux, ys - y0 - t * uy)
        c = np.clip(th / 2.0 + 0.5 - d, 0.0, 1.0)
        m = c > 0
        if not m.any():
            continue
        sub = img[ly:hy + 1, lx:hx + 1]
        new = np.floor(sub + c[..., None] * (np.asarray(col, np.float64) - sub) + 0.5)
        sub[m] = new[m]
        reach[ly:hy + 1, lx:hx + 1] |= m
        full[ly:hy + 1, lx:hx + 1][m] = c[m] >= 1.0
    out = img.astype(np.uint8)
    if return_reach:
        return out, reach, full
    return out


def fixture_strokes(z, case):
    """the reference's recorded cv2.line calls of ``case`` -> {image: [stroke tuples in call order]} in canvas columns"""
    calls, colours = z[case + "/calls"], z[case + "/colour"]
    out = {}
    for c, col in zip(calls, colours):
        image, x_off, _vh, vw, x0, y0, x1, y1, th, _lt = (int(v) for v in c)
        out.setdefault(image, []).append((x0 + x_off, y0, x1 + x_off, y1, tuple(cv2_colour(col)), th, x_off, x_off + vw))
    return out


# -- hand-computed pixels ----------------------------------------------------------------------------------------------------
def test_contract_horizontal_stroke_rows():
    img = raster_contract(12, 32, [(10, 5, 20, 5, (0, 0, 0), 4, 0, 32)])
    # r = 2: d = 0, 1 -> c = 1 (0); d = 2 -> c = 0.5 -> 255 - 127.5 = 127.5 -> 128; d = 3 -> c = 0 (255)
    assert img[:, 15, 0].tolist() == [255, 255, 255, 128, 0, 0, 0, 128, 255, 255, 255, 255]
    # the round cap: 2 px beyond the endpoint c = 0.5, 3 px beyond nothing
    assert img[5, 22, 0] == 128 and img[5, 23, 0] == 255 and img[5, 8, 0] == 128 and img[5, 7, 0] == 255


def test_contract_zero_length_segment_is_a_disc():
    img = raster_contract(11, 11, [(5, 5, 5, 5, (0, 0, 0), 2, 0, 11)])
    c_diag = 1.5 - np.sqrt(2.0)  # r + 0.5 - d at the diagonal neighbours
    want = {(5, 5): 0, (4, 5): 128, (5, 6): 128, (4, 4): int(np.floor(255 - 255 * c_diag + 0.5)), (3, 5): 255, (5, 7): 255}
    for (y, x), v in want.items():
        assert img[y, x, 0] == v, ((y, x), img[y, x, 0], v)
    assert want[(4, 4)] == 233
    assert (img[..., 0] == img[..., 1]).all()


def test_contract_overlap_joint_darkens_per_stroke():
    # two strokes meet at (10, 5); pixel (x 10, y 3) lies at distance 2 from both (the joint point), so c = 0.5 twice:
    # 255 -> 128 -> 64, not 128 (cv2 writes uint8 per call, so joints darken the same way)
    a = (4, 5, 10, 5, (0, 0, 0), 4, 0, 32)
    b = (10, 5, 10, 12, (0, 0, 0), 4, 0, 32)
    assert raster_contract(16, 32, [a])[3, 10, 0] == 128 and raster_contract(16, 32, [b])[3, 10, 0] == 128
    both = raster_contract(16, 32, [a, b])
    assert both[3, 10, 0] == 64
    assert both[5, 10, 0] == 0 and both[3, 14, 0] == 255


def test_contract_window_clip():
    full = raster_contract(10, 40, [(5, 5, 30, 5, (10, 20, 30), 3, 0, 40)])
    clipped = raster_contract(10, 40, [(5, 5, 30, 5, (10, 20, 30), 3, 10, 20)])
    assert (clipped[:, :10] == 255).all() and (clipped[:, 20:] == 255).all()
    assert (clipped[:, 10:20] == full[:, 10:20]).all()
    assert tuple(clipped[5, 15]) == (10, 20, 30)


def test_contract_colour_conversion_matches_cv2_rule():
    assert cv2_colour([255, 255 / 8 * 3, 1 - 255 / 8 * 3]).tolist() == [255, 96, 0]
    assert [int(cv2_colour([0, 255 / 8 * (f + 3), 0])[1]) for f in range(5)] == [96, 128, 159, 191, 223]


# -- the reference's recorded calls -------------------------------------------------------------------------------------------
def test_fixture_is_small_data():
    assert os.path.getsize(FIXTURE) < 1 << 20
    z = np.load(FIXTURE)
    assert all(z[k].dtype != object for k in z.files)


@pytest.mark.parametrize("T", [36, 64, 360])
def test_long_image_arithmetic_matches_the_reference(T):
    from speechdrivestemplates_amd import render
    z = np.load(FIXTURE)
    calls = z["long%d/calls" % T]
    width, windows = render.long_image_layout(T)
    assert (720, width) == tuple(z["long%d/canvas" % T])
    # the windows in draw order: each drawn with one skeleton (108 calls for K = 121), at the reference's column offsets
    offs = calls[:, 1]
    assert len(calls) == 108 * len(windows)
    assert offs.reshape(len(windows), 108).min(1).tolist() == [x0 for _, x0 in windows]
    assert (calls[:, 3] == render.LONG_W).all() and (calls[:, 2] == render.LONG_H).all()
    # pose_step = 720 * 0.7 is 503.99999999999994 in float64: windows start at 0, 503, 1007, ... and T = 64 / 36 / 360 give
    # 8 / 5 / 45 windows on canvases 4991 / 2975 / 23639 px wide
    assert {36: (5, 2975), 64: (8, 4991), 360: (45, 23639)}[T] == (len(windows), width)
    rows = render.long_instances(2, T)[2]
    assert len(rows) == 2 * len(windows) and rows[len(windows)][0] == T  # second clip's poses start at T


def test_instance_layouts():
    from speechdrivestemplates_amd import render
    rows = render.pair_instances(3, (720, 1280), 0.85)
    assert [r[0] for r in rows] == [0, 3, 1, 4, 2, 5]  # prediction then ground truth, per frame
    assert rows[0][1:3] == (float(int(1280 * 0.33)), 360.0) and rows[1][1] == float(int(1280 * 0.67))
    rows = render.clip_instances(2, (721, 1279), 0.85)
    assert rows[1] == (1, 639.0, 360.0, 0.85, 0, 0, 1279, 0)


# -- VideoWriter -------------------------------------------------------------------------------------------------------------
def _cfg(tmp_path, formats, async_=False):
    from speechdrivestemplates_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_list(["SYS.VIDEO_FORMAT", formats, "SYS.ASYNC_VIDEO_SAVING", async_, "SYS.OUTPUT_DIR", str(tmp_path)])
    cfg.freeze()
    return cfg


def _frames(T=3, H=24, W=40):
    f = np.full((T, H, W, 3), 255, np.uint8)
    f[:, 0:16, 0:16] = (255, 0, 0)   # pure blue in BGR (flat 16x16 blocks: small JPEG error)
    f[:, 0:16, 16:32] = (0, 0, 255)  # pure red
    return f


@pytest.mark.parametrize("async_", [False, True])
def test_video_writer_without_ffmpeg_keeps_frames_and_wav(tmp_path, monkeypatch, async_):
    from PIL import Image

    from speechdrivestemplates_amd import video
    monkeypatch.setattr(video.shutil, "which", lambda name: None)
    cfg = _cfg(tmp_path, ["mp4", "img"], async_)
    assert cfg.SYS.RENDER_VIDEO is False  # the opt-in key exists and is off by default
    w = video.VideoWriter(cfg)
    frames, audio = _frames(), np.zeros(1600, np.float32)
    w.save_video(cfg, "TEST", frames, 3, 1, audio=audio, base_path=str(tmp_path))
    w.save_video(cfg, "DEMO", frames, 2, 0, long_img=frames[0], audio=audio, base_path=str(tmp_path), extra_id=4)
    w.close()
    vids = tmp_path / "videos"
    assert sorted(os.listdir(vids)) == ["epoch0-DEMO-step2-4", "epoch0-DEMO-step2-4.wav", "epoch1-TEST-step3", "epoch1-TEST-step3.wav"]
    assert sorted(os.listdir(vids / "epoch1-TEST-step3")) == ["000000.jpg", "000001.jpg", "000002.jpg"]
    assert os.listdir(tmp_path / "imgs") == ["epoch0-DEMO-step2-4.jpg"]  # 'img' writes the DEMO long image only
    rgb = np.asarray(Image.open(tmp_path / "imgs" / "epoch0-DEMO-step2-4.jpg").convert("RGB"))
    assert rgb.shape == (24, 40, 3)
    assert np.abs(rgb[..., ::-1].astype(int) - frames[0]).mean() < 6  # BGR in, RGB JPEG out
    assert np.abs(rgb[8, 8].astype(int) - (0, 0, 255)).max() < 24 and np.abs(rgb[8, 24].astype(int) - (255, 0, 0)).max() < 24
    from scipy.io import wavfile
    sr, a = wavfile.read(vids / "epoch1-TEST-step3.wav")
    assert sr == cfg.DATASET.AUDIO_SR and a.shape == (1600,)


def test_video_writer_formats(tmp_path, monkeypatch):
    from speechdrivestemplates_amd import video
    monkeypatch.setattr(video.shutil, "which", lambda name: None)
    cfg = _cfg(tmp_path, ["tensorboard"])
    w = video.VideoWriter(cfg)
    w.save_video(cfg, "TRAIN", _frames(), 1, 1, global_step=5, base_path=str(tmp_path))  # warned once, nothing written
    assert os.listdir(tmp_path) == []
    cfg = _cfg(tmp_path, ["img"])
    video.VideoWriter(cfg).save_video(cfg, "VAL", _frames(), 1, 1, long_img=_frames()[0], base_path=str(tmp_path))
    assert os.listdir(tmp_path) == []  # no long image outside DEMO, and no frames without 'mp4'
    cfg = _cfg(tmp_path, ["mp4"])
    video.VideoWriter(cfg).save_video(cfg, "TRAIN", _frames(), 7, 2, global_step=9, base_path=str(tmp_path))
    assert sorted(os.listdir(tmp_path / "videos")) == ["epoch2-TRAIN-step7"]  # no audio given: no wav
