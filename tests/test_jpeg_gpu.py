"""GPU JPEG encoder (csrc/jpeg.hip, jpeg.py, video.py): byte equality with the integer contract encoder of
tests/test_jpeg_host.py on the smallest shapes that can go wrong, rendered frames against PIL under the bars measured there, and
VideoWriter.save_video with SYS.DEVICE_JPEG / the 'avi' format."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_jpeg_host import (PSNR_DEFICIT_DB, check_against_pil, decode_bgr, model_encode, noise_image, parse_avi, pil_encode, psnr,
                            segments, strokes_image)
from test_render_host import FIXTURE

pytestmark = pytest.mark.gpu


def mixed(H, W, seed):
    """flat top half (EOB-only blocks, zero DC differences), noise below"""
    x = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    x[: H // 2] = (40 * seed + 30) % 256
    return x


# name -> (image, quality).  noise_q100: 82 MCUs of long codes (about 250 kbit per interval) do not fit the wave's staging buffer at once, so the interval is cut into
# chunks that carry a partial byte; wide_strokes: 69 MCUs, more than one round of 64 lanes.  The noise seed was chosen with the model so
# that the scan contains stuffed 0xFF bytes (asserted below).
CASES = {
    "one_mcu_16x16": lambda: (mixed(16, 16, 1), 95),
    "replicated_8x8": lambda: (mixed(8, 8, 2), 95),
    "replicated_1x1": lambda: (np.array([[[12, 200, 99]]], np.uint8), 95),
    "ragged_17x33": lambda: (mixed(17, 33, 3), 95),
    "three_intervals_48x80": lambda: (mixed(48, 80, 4), 95),
    "rst_wrap_160x48": lambda: (mixed(160, 48, 5), 95),
    "noise_q100_33x1300": lambda: (noise_image(33, 1300, seed=7), 100),
    "white_32x48": lambda: (np.full((32, 48, 3), 255, np.uint8), 95),
    "wide_strokes_20x1100": lambda: (strokes_image(20, 1100, seed=6), 75),
}
_MODEL = {}


def model(name):
    if name not in _MODEL:
        img, q = CASES[name]()
        _MODEL[name] = (img, q, model_encode(img, q))
    return _MODEL[name]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", list(CASES))
def test_bytes_equal_the_contract_model(name):
    from speechdrivestemplates_amd import jpeg
    img, q, want = model(name)
    got = jpeg.encode_frames(dev(img)[None], q)
    assert len(got) == 1 and isinstance(got[0], bytes)
    if got[0] != want:
        n = min(len(got[0]), len(want))
        first = next((i for i in range(n) if got[0][i] != want[i]), n)
        raise AssertionError("%s: %d bytes, model %d, first difference at byte %d" % (name, len(got[0]), len(want), first))
    im, _ = decode_bgr(got[0])
    assert im.size == (img.shape[1], img.shape[0])
    if name.startswith("noise"):
        _, start = segments(want)
        assert b"\xff\x00" in want[start:]
    if name.startswith("rst_wrap"):
        assert b"\xff\xd7" in want and want.count(b"\xff\xd0") >= 2


def test_batch_of_three_images_is_compacted_in_order():
    from speechdrivestemplates_amd import jpeg
    imgs = np.stack([mixed(17, 33, 3), noise_image(17, 33, seed=8), np.full((17, 33, 3), 255, np.uint8)])
    got = jpeg.encode_frames(dev(imgs), 95)
    want = [model("ragged_17x33")[2], model_encode(imgs[1], 95), model_encode(imgs[2], 95)]
    assert len(set(len(w) for w in want)) == 3  # different lengths: a wrong offset table cannot pass
    assert got == want
    again = jpeg.encode_frames(dev(imgs), 95)
    assert again == got  # two calls, identical bytes
    assert jpeg.encode_frames(dev(imgs[1]), 95) == [want[1]]  # (H, W, 3) is one image


def test_groups_of_a_long_batch_match_one_launch(monkeypatch):
    from speechdrivestemplates_amd import _lib, jpeg
    imgs = dev(np.stack([mixed(17, 33, s) for s in range(5)]))
    whole = jpeg.encode_frames(imgs, 95)
    monkeypatch.setattr(jpeg, "MAX_WORKSPACE", 2 * _lib.load().sdt_jpeg_workspace_bytes(1, 17, 33))  # two images per launch group: 2 + 2 + 1
    assert jpeg.encode_frames(imgs, 95) == whole


def test_input_checks():
    from speechdrivestemplates_amd import _lib, jpeg
    x = dev(mixed(32, 48, 1))
    with pytest.raises(ValueError, match="contiguous"):
        jpeg.encode_frames(x[:, ::2])
    with pytest.raises(ValueError, match="uint8"):
        jpeg.encode_frames(x.float())
    with pytest.raises(ValueError):
        jpeg.encode_frames(x[..., :2].contiguous())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        jpeg.encode_frames(x.cpu())
    # the C ABI refuses sizes that do not fit what it was given, before any launch
    lib = _lib.load()
    need = lib.sdt_jpeg_workspace_bytes(1, 32, 48)
    assert need == 2 * 3 * 6 * 136 + 2 * 8 and lib.sdt_jpeg_intervals(1, 32, 48) == 2 and lib.sdt_jpeg_workspace_bytes(1, 0, 48) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    off = torch.zeros(4, dtype=torch.int64, device="cuda")
    tables = jpeg._tables_on(x.device, 95)
    p = lambda t: C.c_void_p(t.data_ptr())
    args = lambda frames_bytes, ws_bytes, n_off: (p(x), frames_bytes, 1, 32, 48, p(tables), p(ws), ws_bytes, p(off), n_off, p(off[3:]), None)
    assert lib.sdt_jpeg_measure(*args(x.numel() - 1, need, 3)) != 0
    assert lib.sdt_jpeg_measure(*args(x.numel(), need - 1, 3)) != 0
    assert lib.sdt_jpeg_measure(*args(x.numel(), need, 2)) != 0
    assert b"sdt_jpeg_measure" in lib.sdt_last_error()


def test_pack_with_foreign_offsets_sets_the_error_word():
    """offsets that do not belong to the input are caught by the range check: nothing is written past an interval's end"""
    from speechdrivestemplates_amd import _lib, jpeg
    from speechdrivestemplates_amd.ops import _stream
    lib = _lib.load()
    x = dev(noise_image(16, 48, seed=1))
    tables = jpeg._tables_on(x.device, 95)
    need = lib.sdt_jpeg_workspace_bytes(1, 16, 48)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    head = torch.zeros(3, dtype=torch.int64, device="cuda")
    err = head[2:].view(torch.int32)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.sdt_jpeg_measure(p(x), x.numel(), 1, 16, 48, p(tables), p(ws), need, p(head), 2, p(err), _stream()))
    total = int(head[1].item())
    assert total > 100 and int(err[0].item()) == 0
    out = torch.full((total,), 0xAB, dtype=torch.uint8, device="cuda")
    short = torch.tensor([0, total - 40], dtype=torch.int64, device="cuda")
    _lib.check(lib.sdt_jpeg_pack(p(ws), need, 1, 16, 48, p(tables), p(short), 2, p(out), total, p(err), _stream()))
    assert int(err[0].item()) & jpeg.ERR_RANGE
    assert (out[total - 40:].cpu().numpy() == 0xAB).all()


# -- rendered frames ------------------------------------------------------------------------------------------------------------
def test_rendered_pair_frame_and_long_image_against_pil():
    from speechdrivestemplates_amd import jpeg, render
    z = np.load(FIXTURE)
    frame = render.render_pose_pair_clip(dev(z["pair/poses"][:1]), dev(z["pair/gt"][:1]), (720, 1280), float(z["scaling"]))
    long_img = render.render_long_image(dev(z["long36/poses"]))
    assert tuple(frame.shape) == (1, 720, 1280, 3) and tuple(long_img.shape) == (720, 2975, 3)
    check_against_pil(jpeg.encode_frames(frame)[0], frame[0].cpu().numpy(), 95, "pair frame 720x1280")
    check_against_pil(jpeg.encode_frames(long_img)[0], long_img.cpu().numpy(), 95, "long image 720x2975")


# -- the writer -------------------------------------------------------------------------------------------------------------------
def _cfg(formats, device_jpeg):
    from speechdrivestemplates_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_list(["SYS.VIDEO_FORMAT", formats, "SYS.DEVICE_JPEG", device_jpeg])
    cfg.freeze()
    return cfg


def _save(tmp_path, name, formats, device_jpeg, frames, long_img, audio):
    from speechdrivestemplates_amd import video
    cfg = _cfg(formats, device_jpeg)
    w = video.VideoWriter(cfg)
    base = tmp_path / name
    w.save_video(cfg, "DEMO", frames, 3, 1, long_img=long_img, audio=audio, base_path=str(base))
    w.close()
    return base, w.last_timing


def test_save_video_with_device_jpeg(tmp_path, monkeypatch):
    from speechdrivestemplates_amd import jpeg, render, video
    monkeypatch.setattr(video.shutil, "which", lambda name: None)  # the frame-directory route, wherever this runs
    z = np.load(FIXTURE)
    frames = render.render_pose_clip(dev(z["clip/poses"][:4]), (720, 1280), float(z["scaling"]))
    long_img = render.render_long_image(dev(z["long36/poses"]))
    audio = (np.sin(np.arange(16000 * 4 // 15) * 0.03) * 0.5).astype(np.float32)
    src, src_long = frames.cpu().numpy(), long_img.cpu().numpy()
    off, t_off = _save(tmp_path, "off", ["mp4", "img"], False, frames, long_img, audio)
    on, t_on = _save(tmp_path, "on", ["mp4", "img", "avi"], True, frames, long_img, audio)
    assert set(t_off) == {"d2h", "encode", "encode_img"} and set(t_on) == {"d2h", "encode", "encode_img", "encode_avi"}
    want = jpeg.encode_frames(frames)
    for i in range(4):
        rel = os.path.join("videos", "epoch1-DEMO-step3", "%06d.jpg" % i)
        # key off: exactly what write_jpg makes of the raw frame
        video.write_jpg(str(tmp_path / "want.jpg"), src[i])
        assert (off / rel).read_bytes() == (tmp_path / "want.jpg").read_bytes()
        # key on: the device encoder's file, as good as the key-off one
        data = (on / rel).read_bytes()
        assert data == want[i]
        assert psnr(decode_bgr(data)[1], src[i]) >= psnr(decode_bgr((off / rel).read_bytes())[1], src[i]) - PSNR_DEFICIT_DB
    rel = os.path.join("imgs", "epoch1-DEMO-step3.jpg")
    video.write_jpg(str(tmp_path / "want.jpg"), src_long)
    assert (off / rel).read_bytes() == (tmp_path / "want.jpg").read_bytes()
    assert (on / rel).read_bytes() == jpeg.encode_frames(long_img)[0]
    assert psnr(decode_bgr((on / rel).read_bytes())[1], src_long) >= psnr(decode_bgr((off / rel).read_bytes())[1], src_long) - PSNR_DEFICIT_DB
    for base in (off, on):
        assert (base / "videos" / "epoch1-DEMO-step3.wav").exists()
    assert not (off / "videos" / "epoch1-DEMO-step3.avi").exists()
    info = parse_avi((on / "videos" / "epoch1-DEMO-step3.avi").read_bytes())
    assert info["frames"] == want and info["avih"][4] == 4 and info["avih"][8:10] == (1280, 720)
    assert info["audio"] == np.round(audio.astype(np.float64) * 32767).astype("<i2").tobytes()


def test_avi_alone_uses_the_device_encoder_without_the_key(tmp_path):
    from speechdrivestemplates_amd import jpeg
    frames = dev(np.stack([strokes_image(48, 80, seed=s) for s in range(3)]))
    base, timing = _save(tmp_path, "avi", ["avi"], False, frames, None, None)
    assert os.listdir(str(base / "videos")) == ["epoch1-DEMO-step3.avi"] and "encode" not in timing
    info = parse_avi((base / "videos" / "epoch1-DEMO-step3.avi").read_bytes())
    assert info["frames"] == jpeg.encode_frames(frames) and len(info["streams"]) == 1
    # host frames: PIL's files
    base, _ = _save(tmp_path, "avi_host", ["avi"], False, frames.cpu().numpy(), None, None)
    info = parse_avi((base / "videos" / "epoch1-DEMO-step3.avi").read_bytes())
    assert info["frames"] == [pil_encode(f) for f in frames.cpu().numpy()]
