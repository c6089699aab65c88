"""The GPU GIF encoder (gif.py, csrc/gif.hip) against the numpy contract model, byte for byte, on the smallest shapes that reach each
hazard; PIL's decoder on the GPU's files; the range check of the packing pass; and VideoWriter.save_video's 'tensorboard' route."""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def noise(shape, seed):
    return rng(seed).integers(0, 256, shape, dtype=np.uint8)


def colour_of(bins):
    """(n,) bins -> (n, 3) BGR pixels that fall into them"""
    bins = np.asarray(bins)
    return np.stack([(bins & 31) << 3, ((bins >> 5) & 31) << 3, (bins >> 10) << 3], -1).astype(np.uint8)


def tie_clip():
    """300 occupied bins: 200 above the cut, 100 with equal counts at it (the 56 lowest of those belong to the palette)"""
    bins = np.sort(rng(3).choice(32768, 300, replace=False))
    heavy = rng(4).choice(300, 200, replace=False)
    x = np.empty((1, 8, 300, 3), np.uint8)
    x[0, :6] = colour_of(bins)[None]
    x[0, 6:] = colour_of(bins[heavy[np.arange(300) % 200]])[None]
    return x, bins, heavy


def flat_rows(shape, seed):
    x = noise(shape, seed)
    x[:, ::2] = x[:, ::2, :1]
    return x


# name -> (frames, downscale)
CASES = {
    "windows 13x22": lambda: (noise((3, 13, 22, 3), 1), True),                     # 2- and 3-wide windows; 120 pixels: <= 256 bins
    "windows 10x15": lambda: (noise((2, 10, 15, 3), 2), True),
    "more than 256 bins": lambda: (noise((2, 9, 300, 3), 3), False),
    "ties at the cut": lambda: (tie_clip()[0], False),
    "widths 10 11 12": lambda: (noise((1, 3, 9595, 3), 6), True),                  # h = 1, w = 3838: one segment of the largest size
    "flat rows": lambda: (flat_rows((2, 6, 700, 3), 4), False),                   # the longest matches; 3 column tiles
    "split row": lambda: (noise((1, 3, 10000, 3), 7), True),                       # w = 4000: two segments of 2000
    "one pixel wide": lambda: (noise((2, 9, 3, 3), 8), True),
    "frame ends on and off a byte": lambda: (rng(58).integers(0, 2, (3, 8, 40, 3), dtype=np.uint8) * 255, False),
    "five output rows": lambda: (noise((1, 14, 660, 3), 9), True),                 # h = 5: a second row group; w = 264: a second tile
}


@functools.lru_cache(maxsize=None)
def model(name):
    from speechdrivestemplates_amd import gif
    x, downscale = CASES[name]()
    rgb, indices, palette = gif.model_quantise(x, downscale)
    data = gif.container([gif.model_frame_stream(f) for f in indices], indices.shape[1], indices.shape[2], palette, 15)
    for a in (x, rgb, indices, palette):
        a.setflags(write=False)
    return x, downscale, rgb, indices, palette, data


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared model arrays are read-only)


@pytest.mark.parametrize("name", list(CASES))
def test_quantise_and_file_equal_the_model(name):
    from speechdrivestemplates_amd import gif
    x, downscale, rgb, indices, palette, data = model(name)
    g_rgb, g_idx, g_pal = gif.quantise(dev(x), downscale)
    assert tuple(g_idx.shape) == indices.shape and tuple(g_rgb.shape) == rgb.shape and tuple(g_pal.shape) == (256, 3)
    assert (g_rgb.cpu().numpy() == rgb).all()
    assert (g_pal.cpu().numpy() == palette).all()
    assert (g_idx.cpu().numpy() == indices).all()
    out = gif.encode_gif(dev(x), 15, downscale)
    assert len(out) == len(data) and out == data


def test_the_cases_reach_their_hazards():
    from speechdrivestemplates_amd import gif
    for name, many in (("windows 13x22", False), ("more than 256 bins", True), ("ties at the cut", True)):
        assert (len(np.unique(gif.model_bins(model(name)[2]))) > 256) == many
    _, bins, heavy = tie_clip()
    light = np.sort(np.setdiff1d(np.arange(300), heavy))
    hist = np.bincount(gif.model_bins(model("ties at the cut")[2]).ravel(), minlength=32768)
    assert (hist[bins[light]] == 6).all() and (hist[bins[heavy]] > 6).all()
    expect = np.sort(np.concatenate([bins[heavy], bins[light[:56]]]))
    assert gif.model_palette(hist)[0].tolist() == expect.tolist()
    idx = model("widths 10 11 12")[3]
    assert idx.shape == (1, 1, 3838) and len(gif.model_lzw_segment(idx[0, 0].tolist())) >= 1791
    assert model("split row")[3].shape == (1, 1, 4000) and model("one pixel wide")[3].shape == (2, 3, 1)
    ends = [int(gif.model_frame_codes(f)[1].sum()) % 8 for f in model("frame ends on and off a byte")[3]]
    assert ends[0] == 0 and ends[1] != 0


def test_two_calls_return_identical_bytes_and_pil_decodes_them():
    from PIL import Image

    from speechdrivestemplates_amd import gif
    x, downscale, rgb, indices, palette, _ = model("flat rows")
    a, b = gif.encode_gif(dev(x), 25, downscale), gif.encode_gif(dev(x), 25, downscale)
    assert a == b
    im = Image.open(io.BytesIO(a))
    assert im.n_frames == 2 and im.size == (700, 6) and im.info["duration"] == 40
    for t in range(2):
        im.seek(t)
        assert (np.asarray(im.convert("RGB")) == palette[indices[t]]).all()


def test_loud_failures():
    from speechdrivestemplates_amd import gif
    with pytest.raises(ValueError):
        gif.encode_gif(torch.zeros((1, 2, 9, 3), dtype=torch.uint8, device="cuda"), 15)  # h = 0
    with pytest.raises(ValueError):
        gif.encode_gif(torch.zeros((1, 9, 9, 3), dtype=torch.float32, device="cuda"), 15)
    with pytest.raises(RuntimeError):
        gif.encode_gif(torch.zeros((1, 9, 9, 3), dtype=torch.uint8), 15)  # a CPU tensor: no fallback


def test_pack_with_foreign_offsets_sets_the_error_word():
    """offsets that do not belong to the input are caught by the range check: nothing is written past a frame's end"""
    from speechdrivestemplates_amd import _lib, gif
    from speechdrivestemplates_amd.ops import _stream
    lib = _lib.load()
    indices = dev(model("more than 256 bins")[3][:1])  # (1, 9, 300)
    T, h, w = indices.shape
    need = lib.sdt_gif_workspace_bytes(T, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    n_off = T + 1 + T * h
    head = torch.zeros(n_off + 1, dtype=torch.int64, device="cuda")
    err = head[n_off:].view(torch.int32)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.sdt_gif_measure(p(indices), indices.numel(), T, h, w, p(ws), need, p(head), n_off, p(err), _stream()))
    total = int(head[1].item())
    assert total > 400 and int(err[0].item()) == 0
    padded = (total + 3) & ~3
    out = torch.full((padded + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    _lib.check(lib.sdt_gif_pack(p(ws), need, T, h, w, p(head), n_off, p(out), padded, p(err), _stream()))
    good = out.cpu().numpy()
    assert int(err[0].item()) == 0 and good[:total].tobytes() == gif.model_frame_stream(model("more than 256 bins")[3][0])
    assert (good[padded:] == 0xAB).all()  # nothing past out_bytes
    short = head.clone()
    short[1] = total - 40  # the frame claims to end 40 bytes early: the last row's bits fall outside its range
    out.fill_(0xAB)
    _lib.check(lib.sdt_gif_pack(p(ws), need, T, h, w, p(short), n_off, p(out), padded, p(short[n_off:].view(torch.int32)), _stream()))
    assert int(short[n_off:].view(torch.int32)[0].item()) & gif.ERR_RANGE
    bad = out.cpu().numpy()
    assert (bad[total - 40:padded] == 0).all() and (bad[padded:] == 0xAB).all()
    assert (bad[:total - 40] == good[:total - 40]).all()


def test_save_video_puts_the_clip_into_the_event_file(tmp_path):
    from PIL import Image

    from speechdrivestemplates_amd import tb_events, video
    from speechdrivestemplates_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_list(["SYS.VIDEO_FORMAT", ["tensorboard"], "SYS.TENSORBOARD", True])
    cfg.freeze()
    frames = dev(noise((4, 20, 30, 3), 5))
    writer = tb_events.EventWriter(str(tmp_path))
    vw = video.VideoWriter(cfg)
    vw.save_video(cfg, "TRAIN", frames, 2, 1, global_step=9, writer=writer, base_path=str(tmp_path))
    vw.save_video(cfg, "TEST", frames, 6, 0, writer=writer, base_path=str(tmp_path), extra_id=2)
    vw.save_video(cfg, "DEMO", frames, 1, 0, writer=writer, base_path=str(tmp_path))
    vw.close()
    writer.close()
    assert os.listdir(tmp_path) == [os.path.basename(writer.path)]
    events = [e for e in tb_events.read_events(writer.path) if e["values"]]
    assert [(e["step"], e["values"][0]["tag"]) for e in events] == [(9, "train/video"), (0, "test/video/6/2")]
    from speechdrivestemplates_amd import gif
    expect = gif.model_encode_gif(frames.cpu().numpy(), cfg.DATASET.FPS)
    for e in events:
        img = e["values"][0]["image"]
        assert (img["height"], img["width"], img["colorspace"]) == (8, 12, 3)
        assert img["encoded"] == expect
        im = Image.open(io.BytesIO(img["encoded"]))
        assert im.format == "GIF" and im.n_frames == 4 and im.size == (12, 8)
