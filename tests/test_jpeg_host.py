"""Host side of the GPU JPEG encoder (speechdrivestemplates_amd/jpeg.py, avi.py, video.py), no GPU needed.

``model_encode`` is the integer contract encoder in numpy: csrc/jpeg.hip must produce its bytes exactly (tests/test_jpeg_gpu.py imports
it).  Here the model itself is held against PIL (libjpeg-turbo): its files decode, its tables are PIL's, and its decoded quality and
file size stay within bars that were measured once on the three inputs below and are recorded in DESIGN.md section 14."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

# measured with PIL 12.2 (libjpeg-turbo) at quality 95, model against PIL's own encode of the same pixels:
#   input      PSNR model / PIL (dB)    size model / PIL (bytes)
#   strokes    29.440 / 29.440          50738 / 50675  (1.0012)
#   blocks     28.669 / 28.669           3295 /  3272  (1.0070)
#   noise      12.722 / 12.722           7864 /  7851  (1.0017)   (4:2:0 chroma cannot carry per-pixel colour noise: PIL's figure too)
# The PSNRs are equal because the transform is libjpeg's integer DCT; the extra bytes are the DRI segment, the RSTn markers and the
# padding of every interval.  Bars = the worst measured deficit + 0.1 dB (decoder differences between runs) and the worst measured
# size ratio + 2 %.
PSNR_DEFICIT_DB = 0.0 + 0.1
SIZE_RATIO = 1.0070 + 0.02


# -- the contract encoder -----------------------------------------------------------------------------------------------------
def _fdct_1d(d, first):
    """one pass of the 13-bit LLM integer DCT along the last axis of an int64 array"""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
        sh = 11
    else:
        o[0], o[4] = (t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2
        sh = 15
    r = 1 << (sh - 1)
    z1 = (t12 + t13) * 4433
    o[2] = (z1 + t13 * 6270 + r) >> sh
    o[6] = (z1 - t12 * 15137 + r) >> sh
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    a4, a5, a6, a7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = (a4 + z1 + z3 + r) >> sh, (a5 + z2 + z4 + r) >> sh, (a6 + z2 + z3 + r) >> sh, (a7 + z1 + z4 + r) >> sh
    return np.stack(o, -1)


def _blocks(plane):
    """(h, w) -> (h // 8, w // 8, 8, 8)"""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def model_coefficients(bgr, quality):
    """(H, W, 3) uint8 BGR -> quantised coefficients in zigzag order: Y (2 rows, 2 cols of blocks per MCU), Cb, Cr block grids"""
    from speechdrivestemplates_amd import jpeg
    H, W, _ = bgr.shape
    x = np.pad(bgr, ((0, -H % 16), (0, -W % 16), (0, 0)), mode="edge").astype(np.int64)
    B, G, R = x[..., 0], x[..., 1], x[..., 2]
    y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    bias = 1 + (np.arange(x.shape[1] // 2) & 1)
    sub = [(c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2 for c in (cb, cr)]
    zz = np.asarray(jpeg.ZIGZAG)
    out = []
    for plane, q in zip([y] + sub, [jpeg.quant_tables(quality)[i] for i in (0, 1, 1)]):
        b = _blocks(plane - 128)
        c = _fdct_1d(b, True)                                   # rows
        c = _fdct_1d(c.swapaxes(-1, -2), False).swapaxes(-1, -2)  # columns
        q = np.asarray(q, np.int64).reshape(8, 8)
        a = (np.abs(c) + 4 * q) // (8 * q)
        c = np.where(c < 0, -a, a)
        out.append(c.reshape(c.shape[0], c.shape[1], 64)[..., zz])
    return out


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def interval(self):
        """pad with 1-bits to a byte, stuff 0x00 after 0xFF"""
        pad = -self.n % 8
        acc, n = (self.acc << pad) | ((1 << pad) - 1), self.n + pad
        return acc.to_bytes(n // 8, "big").replace(b"\xff", b"\xff\x00")


def _put_value(bits, entry_of, run, v):
    nb = int(abs(v)).bit_length()
    e = entry_of[(run << 4) | nb]
    assert e >> 16, "no Huffman code for run %d size %d" % (run, nb)
    bits.put(e & 0xFFFF, e >> 16)
    if nb:
        bits.put((v - 1 if v < 0 else v) & ((1 << nb) - 1), nb)


def model_scan(bgr, quality=95):
    """the scan data the GPU must reproduce: restart intervals of one MCU row, RSTn between them, EOI at the end"""
    from speechdrivestemplates_amd import jpeg
    y, cb, cr = (c.tolist() for c in model_coefficients(bgr, quality))
    dc = [jpeg.huffman_codes(jpeg.DC_LUM, 16), jpeg.huffman_codes(jpeg.DC_CHR, 16)]
    ac = [jpeg.huffman_codes(jpeg.AC_LUM, 256), jpeg.huffman_codes(jpeg.AC_CHR, 256)]
    rows, mcus = len(cb), len(cb[0])
    out = bytearray()
    for r in range(rows):
        bits = _Bits()
        pred = [0, 0, 0]
        for m in range(mcus):
            blocks = [(0, y[2 * r][2 * m]), (0, y[2 * r][2 * m + 1]), (0, y[2 * r + 1][2 * m]), (0, y[2 * r + 1][2 * m + 1]),
                      (1, cb[r][m]), (2, cr[r][m])]
            for comp, c in blocks:
                t = min(comp, 1)
                _put_value(bits, dc[t], 0, c[0] - pred[comp])
                pred[comp] = c[0]
                run = 0
                for k in range(1, 64):
                    if c[k] == 0:
                        run += 1
                        continue
                    while run > 15:
                        bits.put(ac[t][0xF0] & 0xFFFF, ac[t][0xF0] >> 16)
                        run -= 16
                    _put_value(bits, ac[t], run, c[k])
                    run = 0
                if run:
                    bits.put(ac[t][0] & 0xFFFF, ac[t][0] >> 16)
        out += bits.interval()
        out += bytes([0xFF, 0xD9 if r == rows - 1 else 0xD0 + (r & 7)])
    return bytes(out)


def model_encode(bgr, quality=95):
    from speechdrivestemplates_amd import jpeg
    return jpeg.header(bgr.shape[0], bgr.shape[1], quality) + model_scan(bgr, quality)


# -- inputs and measures --------------------------------------------------------------------------------------------------------
def strokes_image(H=256, W=384, seed=0):
    """rendered-style frame: thin coloured anti-aliased strokes on white"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W, 3), 255.0)
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(40):
        x0, x1 = rng.uniform(0, W, 2)
        y0, y1 = rng.uniform(0, H, 2)
        ux, uy = x1 - x0, y1 - y0
        t = np.clip(((xx - x0) * ux + (yy - y0) * uy) / (ux * ux + uy * uy), 0, 1)
        dist = np.hypot(xx - x0 - t * ux, yy - y0 - t * uy)
        cov = np.clip(rng.choice([1.5, 2.0, 2.5]) - dist, 0, 1)[..., None]
        img = img + cov * (rng.integers(0, 256, 3) - img)
    return np.floor(img + 0.5).astype(np.uint8)


def blocks_image(H=128, W=208, seed=1):
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 256, ((H + 23) // 24, (W + 23) // 24, 3), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(cells, np.ones((24, 24, 1), np.uint8))[:H, :W])


def noise_image(H=64, W=96, seed=2):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


INPUTS = {"strokes": strokes_image, "blocks": blocks_image, "noise": noise_image}


def decode_bgr(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im, np.asarray(im.convert("RGB"))[..., ::-1]


def psnr(a, b):
    err = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if err == 0 else 10 * np.log10(255.0 ** 2 / err)


def pil_encode(bgr, quality=95):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, "JPEG", quality=quality)
    return buf.getvalue()


def check_against_pil(data, bgr, quality, what):
    """the PSNR and size bars of DESIGN.md section 14: ``data`` (a file of ours) against PIL's own encode of the same pixels"""
    im, got = decode_bgr(data)
    assert im.size == (bgr.shape[1], bgr.shape[0]) and im.mode == "RGB", (what, im.size, im.mode)
    ref = pil_encode(bgr, quality)
    ours, pils = psnr(got, bgr), psnr(decode_bgr(ref)[1], bgr)
    print("%s: PSNR ours %.3f dB, PIL %.3f dB; bytes ours %d, PIL %d (ratio %.4f)" % (what, ours, pils, len(data), len(ref), len(data) / len(ref)))
    assert ours >= pils - PSNR_DEFICIT_DB, "%s: PSNR %.3f dB, PIL's %.3f dB" % (what, ours, pils)
    assert len(data) <= SIZE_RATIO * len(ref), "%s: %d bytes, PIL's %d" % (what, len(data), len(ref))
    return ours, pils


def segments(data):
    """marker segments up to SOS -> [(marker, payload)]"""
    assert data[:2] == b"\xff\xd8"
    i, out = 2, []
    while True:
        assert data[i] == 0xFF
        marker, length = data[i + 1], struct.unpack(">H", data[i + 2:i + 4])[0]
        out.append((marker, data[i + 4:i + 2 + length]))
        i += 2 + length
        if marker == 0xDA:
            return out, i


# -- the model against PIL ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 16), (8, 8), (1, 1), (17, 33), (48, 80)])
def test_model_files_decode_to_the_right_size(shape):
    bgr = np.random.default_rng(5).integers(0, 256, shape + (3,), dtype=np.uint8)
    bgr[: shape[0] // 2] = 200  # half flat, half noise
    data = model_encode(bgr, 95)
    im, got = decode_bgr(data)
    assert im.size == (shape[1], shape[0]) and im.mode == "RGB" and im.format == "JPEG"
    pils = psnr(decode_bgr(pil_encode(bgr, 95))[1], bgr)
    assert psnr(got, bgr) >= pils - PSNR_DEFICIT_DB, (psnr(got, bgr), pils)


@pytest.mark.parametrize("quality", [50, 75, 95, 100])
def test_header_tables_equal_pils(quality):
    from speechdrivestemplates_amd import jpeg
    ours, _ = segments(jpeg.header(32, 48, quality))
    pils, _ = segments(pil_encode(noise_image(32, 48), quality))
    for marker in (0xE0, 0xDB, 0xC0, 0xC4, 0xDA):  # JFIF 1.01 density 1:1, both DQT, SOF0, the four DHT, SOS
        assert [p for m, p in ours if m == marker] == [p for m, p in pils if m == marker], hex(marker)
    assert [m for m, _ in ours] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert dict(ours)[0xDD] == struct.pack(">H", 3)
    if quality == 95:
        assert list(jpeg.quant_tables(95)[0][:8]) == [2, 1, 1, 2, 2, 4, 5, 6]


def test_device_table_words():
    from speechdrivestemplates_amd import jpeg
    t = jpeg.device_tables(95)
    assert t.dtype == np.uint32 and t.shape == (jpeg.TABLE_WORDS,)
    assert (t[:128] >= 1).all() and (t[:128] <= 255).all()
    lengths = t[128:] >> 16
    assert lengths.max() == 16 and (lengths[:12] > 0).all() and (lengths[16:28] > 0).all()
    assert int((lengths[32:288] > 0).sum()) == 162 and int((lengths[288:] > 0).sum()) == 162
    with pytest.raises(ValueError):
        jpeg.quant_tables(0)
    assert sorted(jpeg.ZIGZAG) == list(range(64)) and jpeg.ZIGZAG[:6] == (0, 1, 8, 16, 9, 2)


@pytest.mark.parametrize("name", list(INPUTS))
def test_model_quality_and_size_against_pil(name):
    bgr = INPUTS[name]()
    check_against_pil(model_encode(bgr, 95), bgr, 95, name)


def test_model_restart_markers_and_stuffing():
    bgr = noise_image(160, 48, seed=3)  # ten intervals: the RST index wraps past 7
    data = model_encode(bgr, 100)
    _, start = segments(data)
    scan = data[start:]
    assert scan.endswith(b"\xff\xd9")
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] not in (0x00, 0xFF)]
    assert marks == [0xD0 + (i & 7) for i in range(9)] + [0xD9]
    assert b"\xff\x00" in scan
    assert psnr(decode_bgr(data)[1], bgr) >= psnr(decode_bgr(pil_encode(bgr, 100))[1], bgr) - PSNR_DEFICIT_DB


# -- the AVI writer -----------------------------------------------------------------------------------------------------------
def riff_chunks(data, start, end):
    """[(fourcc, payload offset, size)] of the chunks in data[start:end]; a LIST's payload starts with its type"""
    out = []
    while start + 8 <= end:
        cc, size = data[start:start + 4], struct.unpack("<I", data[start + 4:start + 8])[0]
        out.append((cc, start + 8, size))
        start += 8 + size + (size & 1)
    return out


def parse_avi(data):
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    top = riff_chunks(data, 12, len(data))
    info = {"frames": [], "audio": b"", "streams": []}
    for cc, off, size in top:
        if cc == b"LIST" and data[off:off + 4] == b"hdrl":
            for c2, o2, s2 in riff_chunks(data, off + 4, off + size):
                if c2 == b"avih":
                    info["avih"] = struct.unpack("<14I", data[o2:o2 + 56])
                if c2 == b"LIST" and data[o2:o2 + 4] == b"strl":
                    s = {c3: data[o3:o3 + s3] for c3, o3, s3 in riff_chunks(data, o2 + 4, o2 + s2)}
                    info["streams"].append(s)
        if cc == b"LIST" and data[off:off + 4] == b"movi":
            info["movi"] = off  # idx1 offsets count from the 'movi' fourcc
            for c2, o2, s2 in riff_chunks(data, off + 4, off + size):
                if c2 == b"00dc":
                    info["frames"].append(data[o2:o2 + s2])
                if c2 == b"01wb":
                    info["audio"] += data[o2:o2 + s2]
        if cc == b"idx1":
            info["idx1"] = [struct.unpack("<4s3I", data[off + 16 * i:off + 16 * i + 16]) for i in range(size // 16)]
    return info


@pytest.mark.parametrize("with_audio", [True, False])
def test_avi_round_trip(tmp_path, with_audio):
    from speechdrivestemplates_amd import avi
    frames = [strokes_image(48, 80, seed=s) for s in range(5)]
    jpegs = [pil_encode(f) if i % 2 else model_encode(f) for i, f in enumerate(frames)]
    audio = (np.sin(np.arange(16000 * 5 // 15) * 0.05) * 1.3).astype(np.float32) if with_audio else None  # clips at +-1
    path = str(tmp_path / "clip.avi")
    avi.write_avi(path, jpegs, fps=15, width=80, height=48, audio=audio, sample_rate=16000)
    data = open(path, "rb").read()
    info = parse_avi(data)
    assert len(info["frames"]) == 5
    for got, want, src in zip(info["frames"], jpegs, frames):
        assert got == want
        im, px = decode_bgr(got)
        assert im.size == (80, 48) and psnr(px, src) >= psnr(decode_bgr(pil_encode(src))[1], src) - PSNR_DEFICIT_DB
    avih = info["avih"]
    assert avih[0] == 1000000 // 15 and avih[4] == 5 and avih[6] == (2 if with_audio else 1) and avih[8:10] == (80, 48)
    assert avih[3] & 0x10  # AVIF_HASINDEX
    assert len(info["streams"]) == (2 if with_audio else 1)
    vs = info["streams"][0]
    assert vs[b"strh"][:8] == b"vidsMJPG"
    scale, rate, _, length = struct.unpack("<4I", vs[b"strh"][20:36])
    assert (rate, scale, length) == (15, 1, 5)
    size, w, h, planes, bpp, comp = struct.unpack("<IiiHH4s", vs[b"strf"][:20])
    assert (size, w, h, planes, bpp, comp) == (40, 80, 48, 1, 24, b"MJPG")
    if with_audio:
        want = np.round(np.clip(audio.astype(np.float64), -1, 1) * 32767).astype("<i2").tobytes()
        assert info["audio"] == want and (np.frombuffer(want, "<i2").max() == 32767)
        as_ = info["streams"][1]
        assert as_[b"strh"][:4] == b"auds"
        fmt, ch, sr, bps, align, bits = struct.unpack("<HHIIHH", as_[b"strf"][:16])
        assert (fmt, ch, sr, bps, align, bits) == (1, 1, 16000, 32000, 2, 16)
        assert struct.unpack("<4I", as_[b"strh"][20:36])[3] == len(want) // 2
    n_chunks = 5 + (1 if with_audio else 0)
    assert len(info["idx1"]) == n_chunks
    for cc, flags, off, size in info["idx1"]:
        at = info["movi"] + off
        assert data[at:at + 4] == cc and struct.unpack("<I", data[at + 4:at + 8])[0] == size
        assert cc in (b"00dc", b"01wb") and flags & 0x10


def test_avi_int16_audio_passes_through(tmp_path):
    from speechdrivestemplates_amd import avi
    pcm = np.arange(-5, 6, dtype=np.int16) * 1000
    path = str(tmp_path / "a.avi")
    avi.write_avi(path, [pil_encode(blocks_image(16, 16))], fps=15, width=16, height=16, audio=pcm, sample_rate=16000)
    assert parse_avi(open(path, "rb").read())["audio"] == pcm.astype("<i2").tobytes()
    with pytest.raises(ValueError):
        avi.write_avi(path, [], fps=15, width=16, height=16)


# -- the writer's host routes -------------------------------------------------------------------------------------------------
def _cfg(formats, device_jpeg=False):
    from speechdrivestemplates_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_list(["SYS.VIDEO_FORMAT", formats, "SYS.DEVICE_JPEG", device_jpeg])
    cfg.freeze()
    return cfg


def test_config_defaults():
    from speechdrivestemplates_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    assert cfg.SYS.DEVICE_JPEG is False and "avi" not in cfg.SYS.VIDEO_FORMAT


@pytest.mark.parametrize("device_jpeg", [False, True])
def test_save_video_host_frames_keep_the_pil_route(tmp_path, monkeypatch, device_jpeg):
    """numpy frames never reach the device encoder, with or without SYS.DEVICE_JPEG: the files are write_jpg's bytes"""
    from speechdrivestemplates_amd import video
    monkeypatch.setattr(video.shutil, "which", lambda name: None)  # the frame-directory route, wherever this runs
    frames = np.stack([strokes_image(48, 80, seed=s) for s in range(4)])
    long_img = strokes_image(48, 200, seed=9)
    cfg = _cfg(["mp4", "img", "avi"], device_jpeg)
    w = video.VideoWriter(cfg)
    w.save_video(cfg, "DEMO", frames, 7, 2, long_img=long_img, audio=np.zeros(4000, np.float32), base_path=str(tmp_path))
    w.close()
    assert set(w.last_timing) >= {"d2h", "encode", "encode_img"}
    for i in range(4):
        video.write_jpg(str(tmp_path / "want.jpg"), frames[i])
        want = (tmp_path / "want.jpg").read_bytes()
        assert (tmp_path / "videos" / "epoch2-DEMO-step7" / ("%06d.jpg" % i)).read_bytes() == want
    video.write_jpg(str(tmp_path / "want.jpg"), long_img)
    assert (tmp_path / "imgs" / "epoch2-DEMO-step7.jpg").read_bytes() == (tmp_path / "want.jpg").read_bytes()
    info = parse_avi((tmp_path / "videos" / "epoch2-DEMO-step7.avi").read_bytes())
    assert len(info["frames"]) == 4 and info["avih"][8:10] == (80, 48) and len(info["audio"]) == 8000
    for got, src in zip(info["frames"], frames):
        assert got == pil_encode(src)
