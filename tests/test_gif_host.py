"""The GIF contract's numpy model (gif.py: model_*) without a GPU: the downscale against torch's area interpolation, the palette rule,
and complete files against PIL's decoder."""
import io

import numpy as np
import pytest
import torch

from speechdrivestemplates_amd import gif


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def noise(shape, seed):
    return rng(seed).integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("H,W", [(720, 1280), (13, 22), (10, 15)])
def test_downscale_is_within_one_level_of_area_interpolation(H, W):
    x = noise((2, H, W, 3), H)
    x[1, : H // 2] = x[1, :1, :1]  # a flat half: exact means
    mine = gif.model_downscale(x)
    t = torch.from_numpy(x[..., ::-1].copy()).permute(0, 3, 1, 2).float() / 255
    ref = torch.nn.functional.interpolate(t, scale_factor=0.4, mode="area") * 255
    ref = ref.permute(0, 2, 3, 1).numpy()
    assert mine.shape == ref.shape == (2, (2 * H) // 5, (2 * W) // 5, 3)
    diff = np.abs(mine.astype(np.int64) - np.rint(ref).astype(np.int64))
    print("downscale %dx%d: max level difference %d, %d of %d differ" % (H, W, diff.max(), (diff > 0).sum(), diff.size))
    assert diff.max() <= 1, "%d values differ by more than one level" % (diff > 1).sum()
    assert (mine[1, : (2 * (H // 2)) // 5 - 1] == x[1, 0, 0, ::-1]).all()


def test_window_geometry_at_the_canvas_size():
    r0, r1 = gif._windows(720, 288)
    assert ((r1 - r0) == 3).all() and (r0[1:] - r1[:-1] == -1)[::2].all()  # 3-wide windows; every second pair overlaps by one row
    c0, c1 = gif._windows(1280, 512)
    assert ((c1 - c0) == 3).all()


def _hist(pairs):
    h = np.zeros(32768, np.int64)
    for b, c in pairs:
        h[b] = c
    return h


def test_palette_three_bins():
    bins, palette, table = gif.model_palette(_hist([(0, 5), (32767, 1), (0x1234, 9)]))
    assert bins.tolist() == [0, 0x1234, 32767]
    assert palette[:3].tolist() == [[0, 0, 0], [(4 << 3) | 1, (17 << 3) | 4, (20 << 3) | 5], [255, 255, 255]]
    assert not palette[3:].any()
    assert table[0] == 0 and table[0x1234] == 1 and table[32767] == 2
    assert table[1] == 0 and table[32766] == 2 and table[0x1235] == 1
    # a bin at equal distance from two entries goes to the lower one: (0, 0, 16) lies 16 from black ... compare by hand
    d = lambda a, b: sum((((a >> s) & 31) - ((b >> s) & 31)) ** 2 for s in (10, 5, 0))
    for b in (16, 0x0210, 0x4000, 12345):
        best = min(range(3), key=lambda k: (d(b, int(bins[k])), k))
        assert table[b] == best


def test_palette_exactly_256_bins():
    occupied = np.sort(rng(1).choice(32768, 256, replace=False))
    bins, palette, table = gif.model_palette(_hist(zip(occupied, rng(2).integers(1, 100, 256))))
    assert bins.tolist() == occupied.tolist()
    assert (table[occupied] == np.arange(256)).all()


def test_palette_ties_at_the_cut_go_to_the_lower_bins():
    occupied = np.sort(rng(3).choice(32768, 300, replace=False))
    counts = np.full(300, 7)
    heavy = rng(4).choice(300, 200, replace=False)
    counts[heavy] = 50  # 200 bins above the cut, 100 bins at it: the 56 lowest of those are taken
    bins, _, table = gif.model_palette(_hist(zip(occupied, counts)))
    light = np.sort(np.setdiff1d(np.arange(300), heavy))
    expect = np.sort(np.concatenate([occupied[heavy], occupied[light[:56]]]))
    assert bins.tolist() == expect.tolist()
    # all 300 equal: the 256 lowest bins
    bins, _, _ = gif.model_palette(_hist(zip(occupied, np.full(300, 3))))
    assert bins.tolist() == occupied[:256].tolist()


def decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    frames = []
    for t in range(im.n_frames):
        im.seek(t)
        frames.append(np.asarray(im.convert("RGB")))
    return im, np.stack(frames)


def flat_rows(shape, seed):
    x = noise(shape, seed)
    x[:, ::2] = x[:, ::2, :1]  # every second row flat: the longest matches
    return x


CASES = {
    "random 13x22": lambda: (noise((3, 13, 22, 3), 1), True),
    "random 10x15": lambda: (noise((2, 10, 15, 3), 2), True),
    "w7": lambda: (noise((1, 4, 7, 3), 3), False),
    "w300 flat rows": lambda: (flat_rows((2, 6, 300, 3), 4), False),
    "w1024": lambda: (flat_rows((1, 2, 1024, 3), 5), False),
    "w3838": lambda: (noise((1, 3, 9595, 3), 6), True),
    "w4000 split": lambda: (noise((1, 3, 10000, 3), 7), True),
    "one pixel wide": lambda: (noise((2, 9, 3, 3), 8), True),
    "three frames few colours": lambda: (noise((3, 25, 40, 3), 9) // 64 * 85, True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_complete_files_decode_in_pil_to_the_quantised_frames(name):
    x, downscale = CASES[name]()
    rgb, indices, palette = gif.model_quantise(x, downscale)
    data = gif.model_encode_gif(x, 15, downscale)
    im, frames = decode(data)
    assert im.n_frames == x.shape[0] and im.size == (indices.shape[2], indices.shape[1])
    assert im.info["duration"] == 70 and im.info.get("loop") == 0  # round(100 / 15) = 7 centiseconds
    assert (frames == palette[indices]).all()
    if len(np.unique(gif.model_bins(rgb))) <= 256:  # every colour has its own palette entry: only the 5-bit truncation is lost
        assert np.abs(frames.astype(int) - rgb.astype(int)).max() <= 7


def test_segments_and_widths():
    assert gif.segments(1) == [(0, 1)] and gif.segments(3838) == [(0, 3838)]
    assert gif.segments(4000) == [(0, 2000), (2000, 2000)] and gif.segments(3839) == [(0, 1920), (1920, 1919)]
    assert gif.segments(65535)[-1][0] + gif.segments(65535)[-1][1] == 65535 and max(n for _, n in gif.segments(65535)) <= 3838
    # the closed form of the width rule against the rule itself
    width, nxt = 9, 258
    for k in range(3839):
        assert gif.width_after(k) == width
        nxt += 1
        if nxt > (1 << width) and width < 12:
            width += 1
    x, _ = CASES["w3838"]()
    _, indices, _ = gif.model_quantise(x)
    assert len(gif.model_lzw_segment(indices[0, 0].tolist())) >= 1791  # the row reaches 12-bit codes


def test_few_colour_clip_keeps_every_channel_within_seven():
    x = noise((2, 30, 50, 3), 11) % 6 * 51  # 216 colours
    rgb, indices, palette = gif.model_quantise(x, False)
    assert len(np.unique(gif.model_bins(rgb))) <= 256
    assert np.abs(palette[indices].astype(int) - rgb.astype(int)).max() <= 7
