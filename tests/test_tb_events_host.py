"""TensorBoard event files (tb_events.py) without a GPU: CRC-32C, the record framing and the protobuf fields read back by a parser
written here, truncation, the command-line listing, and the Trainer wiring with SYS.TENSORBOARD off and on."""
import glob
import io
import os
import struct
import types

import numpy as np
import pytest

from speechdrivestemplates_amd import tb_events as TB


# -- a minimal reader of its own: framing, both masked CRCs, varints ---------------------------------------------------------------
def _crc(data):
    c = 0xFFFFFFFF
    for b in data:
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
    return c ^ 0xFFFFFFFF


def _masked(data):
    c = _crc(data)
    return ((c >> 15 | c << 17) + 0xA282EAD8) % (1 << 32)


def _varint(buf, pos):
    v = shift = 0
    while True:
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << shift
        shift += 7
        if b < 0x80:
            return v, pos


def _message(buf):
    out, pos = [], 0
    while pos < len(buf):
        key, pos = _varint(buf, pos)
        wire = key & 7
        if wire == 0:
            v, pos = _varint(buf, pos)
        elif wire == 1:
            v, pos = buf[pos:pos + 8], pos + 8
        elif wire == 5:
            v, pos = buf[pos:pos + 4], pos + 4
        else:
            assert wire == 2
            n, pos = _varint(buf, pos)
            v, pos = buf[pos:pos + n], pos + n
        assert pos <= len(buf)
        out.append((key >> 3, wire, v))
    return out


def parse(path):
    """[(step, file_version, [(tag, float | None, image dict | None)])]; raises ValueError on a damaged file"""
    buf = open(path, "rb").read()
    pos, events = 0, []
    while pos < len(buf):
        if len(buf) - pos < 12:
            raise ValueError("truncated header")
        n, crc = struct.unpack_from("<QI", buf, pos)
        if crc != _masked(buf[pos:pos + 8]):
            raise ValueError("length crc")
        if len(buf) - pos < 16 + n:
            raise ValueError("truncated record")
        data = buf[pos + 12:pos + 12 + n]
        if struct.unpack_from("<I", buf, pos + 12 + n)[0] != _masked(data):
            raise ValueError("data crc")
        pos += 16 + n
        step, version, values, wall = 0, None, [], None
        for f, w, v in _message(data):
            if (f, w) == (1, 1):
                wall, = struct.unpack("<d", v)
            elif (f, w) == (2, 0):
                step = v
            elif (f, w) == (3, 2):
                version = v.decode()
            elif (f, w) == (5, 2):
                for f2, w2, value in _message(v):
                    assert (f2, w2) == (1, 2)
                    tag = val = img = None
                    for f3, w3, x in _message(value):
                        if (f3, w3) == (1, 2):
                            tag = x.decode()
                        elif (f3, w3) == (2, 5):
                            val, = struct.unpack("<f", x)
                        elif (f3, w3) == (4, 2):
                            img = {k: y for k, y in ((("height", "width", "colorspace", "encoded")[f4 - 1], y) for f4, _, y in _message(x))}
                    values.append((tag, val, img))
        assert wall is not None and wall > 1e9
        events.append((step, version, values))
    return events


def _png_bytes():
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)).save(buf, "PNG")
    return buf.getvalue()


def _gif_bytes():
    from speechdrivestemplates_amd import gif
    x = np.random.Generator(np.random.PCG64(3)).integers(0, 256, (2, 10, 15, 3), dtype=np.uint8)
    return gif.model_encode_gif(x, 15)


SCALARS = [("train/G_loss", 0.123456789, 7), ("train/lr_G", 1e-4, 7), ("val/L2_dist", -3.5e10, 2), ("train/ETA", 0.0, 1 << 40)]


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    d = tmp_path_factory.mktemp("tb")
    w = TB.EventWriter(str(d))
    for tag, v, step in SCALARS:
        w.add_scalar(tag, v, step)
    png, gif_ = _png_bytes(), _gif_bytes()
    w.add_image_bytes("train/clip_code", png, 5, 7, 3)
    w.add_image_bytes("val/video/4", gif_, 4, 6, 2)
    w.flush()
    w.close()
    return w.path, png, gif_


def test_crc32c_known_answers():
    assert TB.crc32c(b"123456789") == 0xE3069283
    assert TB.crc32c(bytes(32)) == 0x8A9136AA
    assert TB.crc32c(b"") == 0
    c = 0xE3069283
    assert TB.masked_crc32c(b"123456789") == ((c >> 15 | c << 17) + 0xA282EAD8) % (1 << 32)


def test_file_name_and_records_read_back(written):
    path, png, gif_ = written
    name = os.path.basename(path)
    parts = name.split(".")
    assert name.startswith("events.out.tfevents.") and len(parts[3]) == 10 and parts[3].isdigit() and len(parts) >= 5 and parts[4]
    events = parse(path)
    assert events[0] == (0, "brain.Event:2", [])
    assert len(events) == 1 + len(SCALARS) + 2
    for (step, version, values), (tag, v, s) in zip(events[1:], SCALARS):
        assert version is None and step == s
        assert values == [(tag, float(np.float32(v)), None)]
    step, _, [(tag, val, img)] = events[-2]
    assert (step, tag, val) == (3, "train/clip_code", None)
    assert img == {"height": 5, "width": 7, "colorspace": 3, "encoded": png}
    step, _, [(tag, val, img)] = events[-1]
    assert (step, tag, val) == (2, "val/video/4", None)
    assert img == {"height": 4, "width": 6, "colorspace": 3, "encoded": gif_}
    # the module's own reader agrees with the parser above
    mine = TB.read_events(path)
    assert [e["step"] for e in mine] == [e[0] for e in events]
    assert mine[-1]["values"][0]["image"]["encoded"] == gif_


@pytest.mark.parametrize("cut", [1, 5, 20, 1000])
def test_truncated_file_is_detected(written, tmp_path, cut):
    buf = open(written[0], "rb").read()
    short = tmp_path / "events.out.tfevents.short"
    short.write_bytes(buf[:-cut])
    with pytest.raises(ValueError):
        parse(str(short))
    with pytest.raises(TB.CorruptFile):
        TB.read_records(str(short))


def test_a_flipped_bit_is_detected(written, tmp_path):
    buf = bytearray(open(written[0], "rb").read())
    buf[len(buf) // 2] ^= 0x10
    bad = tmp_path / "events.out.tfevents.bad"
    bad.write_bytes(bytes(buf))
    with pytest.raises(TB.CorruptFile):
        TB.read_records(str(bad))


def test_cli_lists_the_same_records(written, tmp_path, capsys):
    path, png, gif_ = written
    TB.main([path, "--extract", str(tmp_path / "x")])
    lines = capsys.readouterr().out.strip().split("\n")
    assert lines[0] == "- file_version brain.Event:2"
    for line, (tag, v, step) in zip(lines[1:], SCALARS):
        s, t, x = line.split(" ")
        assert (int(s), t) == (step, tag) and np.float32(float(x)) == np.float32(v)
    assert lines[5] == "3 train/clip_code image 5x7 %d bytes" % len(png)
    assert lines[6] == "2 val/video/4 image 4x6 %d bytes" % len(gif_)
    files = sorted(os.listdir(tmp_path / "x"))
    assert [f[-4:] for f in files] == [".png", ".gif"]
    assert (tmp_path / "x" / files[0]).read_bytes() == png and (tmp_path / "x" / files[1]).read_bytes() == gif_


# -- the Trainer wiring, on a stub pipeline (no GPU: Trainer.__init__ is not run) -----------------------------------------------------
def _stub(tmp_path, tensorboard):
    import torch

    from speechdrivestemplates_amd.config import get_cfg_defaults
    from speechdrivestemplates_amd.core.pipelines.trainer import Trainer
    cfg = get_cfg_defaults()
    assert cfg.SYS.TENSORBOARD is False  # the opt-in key exists and is off by default
    cfg.merge_from_list(["SYS.TENSORBOARD", tensorboard, "SYS.OUTPUT_DIR", str(tmp_path)])
    cfg.freeze()
    t = Trainer.__new__(Trainer)
    t.cfg, t.base_path, t.step_tic = cfg, str(tmp_path), 0.0
    t.check_kernels = lambda: None
    t.get_rank = lambda: 0
    two_groups = types.SimpleNamespace(param_groups=[{"lr": 1e-4}, {"lr": 5e-5}])
    t.optimizers = {"G": two_groups, "D": types.SimpleNamespace(param_groups=[{"lr": 2e-4}])}
    losses = {"G_reg_loss": torch.tensor(0.5), "G_clipcode_kl_loss": torch.tensor(0.25), "G_loss": torch.tensor(0.75)}
    return t, losses


def test_tensorboard_off_writes_no_event_file(tmp_path):
    t, losses = _stub(tmp_path, False)
    assert t.setup_tb_writer() is None
    t.logger_writer_step("TRAIN", losses, 3, epoch=1, global_step=11)
    t.tb_epoch_scalars("val", {"L2_dist": 1.0}, 1)
    t.close()
    assert glob.glob(str(tmp_path / "**" / "events.out.tfevents*"), recursive=True) == []


def test_tensorboard_on_logs_the_reference_tag_set(tmp_path):
    t, losses = _stub(tmp_path, True)
    w = t.setup_tb_writer()
    assert w is not None and t.setup_tb_writer() is w
    t.logger_writer_step("TRAIN", losses, 3, epoch=1, global_step=11)
    t.logger_writer_step("VAL", losses, 4, epoch=1)  # the reference writes nothing for a validation step (trainer.py:265-269)
    t.tb_epoch_scalars("val", {"L2_dist": 2.0}, 1)
    t.close()
    assert t.tb_writer is None
    files = glob.glob(str(tmp_path / "events.out.tfevents*"))
    assert len(files) == 1
    events = parse(files[0])[1:]
    got = [(step, values[0][0], values[0][1]) for step, _, values in events]
    f32 = lambda v: float(np.float32(v))
    assert got == [(11, "train/lr_G", f32(1e-4)), (11, "train/lr_G_1", f32(5e-5)), (11, "train/lr_D", f32(2e-4)),
                   (11, "train/G_reg_loss", 0.5), (11, "train/G_clipcode_kl_loss", 0.25), (11, "train/G_loss", 0.75),
                   (1, "val/L2_dist", 2.0)]


def test_video_writer_numpy_frames_into_the_event_file(tmp_path):
    """the 'tensorboard' token with a writer: numpy frames take the host route (model downscale + PIL's GIF writer)"""
    from PIL import Image

    from speechdrivestemplates_amd import video
    from speechdrivestemplates_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_list(["SYS.VIDEO_FORMAT", ["tensorboard"], "SYS.ASYNC_VIDEO_SAVING", True])
    cfg.freeze()
    frames = np.random.Generator(np.random.PCG64(5)).integers(0, 256, (3, 20, 30, 3), dtype=np.uint8)
    w = TB.EventWriter(str(tmp_path))
    vw = video.VideoWriter(cfg)
    vw.save_video(cfg, "TRAIN", frames, 2, 1, global_step=9, writer=w, base_path=str(tmp_path))
    vw.save_video(cfg, "VAL", frames, 6, 4, writer=w, base_path=str(tmp_path), extra_id=1)
    vw.save_video(cfg, "DEMO", frames, 1, 0, writer=w, base_path=str(tmp_path))
    vw.close()
    w.close()
    assert os.listdir(tmp_path) == [os.path.basename(w.path)]
    events = parse(w.path)[1:]
    assert [(s, v[0][0]) for s, _, v in events] == [(9, "train/video"), (4, "val/video/6/1")]
    for _, _, values in events:
        img = values[0][2]
        assert (img["height"], img["width"]) == (8, 12)
        im = Image.open(io.BytesIO(img["encoded"]))
        assert im.format == "GIF" and im.n_frames == 3 and im.size == (12, 8)
