"""Motion-JPEG AVI writer (host only): a playable video with the clip's audio where there is no ffmpeg.

A RIFF 'AVI ' file with one 'MJPG' video stream (one ``00dc`` chunk per JPEG file, every frame a key frame), optionally one PCM s16
mono audio stream (one ``01wb`` chunk in front of the frames), the ``avih`` / ``strh`` / ``strf`` headers with frame counts and sizes
filled in, and an ``idx1`` index whose offsets count from the 'movi' fourcc.  The JPEG bytes are written as they are given: baseline
4:2:0 files from jpeg.encode_frames or from PIL both qualify.  Files are limited to 4 GiB (no OpenDML extension).
"""
import struct

import numpy as np

AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10


def pcm_s16(audio):
    """float audio -> clipped to [-1, 1], scaled by 32767 and rounded; integer audio is taken as int16 samples"""
    a = np.asarray(audio).reshape(-1)
    if a.dtype.kind == "f":
        a = np.round(np.clip(a.astype(np.float64), -1.0, 1.0) * 32767.0)
    return a.astype("<i2")


def _chunk(fourcc, payload):
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\x00" if len(payload) & 1 else b"")


def _list(kind, payload):
    return b"LIST" + struct.pack("<I", len(payload) + 4) + kind + payload


def write_avi(path, jpegs, fps, width, height, audio=None, sample_rate=16000):
    """``jpegs``: the frames as complete JPEG files (bytes); ``audio``: None or a 1-D array (see pcm_s16)"""
    jpegs = list(jpegs)
    if not jpegs:
        raise ValueError("an AVI file needs at least one frame")
    if fps <= 0:
        raise ValueError("fps must be positive, got %r" % (fps,))
    rate, scale = (int(fps), 1) if float(fps) == int(fps) else (int(round(fps * 1000)), 1000)
    pcm = pcm_s16(audio).tobytes() if audio is not None else None
    chunks = ([(b"01wb", pcm)] if pcm is not None else []) + [(b"00dc", j) for j in jpegs]
    movi, index, pos = [], [], 4  # offsets count from the 'movi' fourcc
    for cc, payload in chunks:
        index.append(struct.pack("<4s3I", cc, AVIIF_KEYFRAME, pos, len(payload)))
        c = _chunk(cc, payload)
        movi.append(c)
        pos += len(c)
    largest = max(len(j) for j in jpegs)
    seconds = len(jpegs) * scale / rate
    total = sum(len(j) for j in jpegs) + (len(pcm) if pcm is not None else 0)
    avih = struct.pack("<14I", 1000000 * scale // rate, int(total / seconds) + 1, 0, AVIF_HASINDEX, len(jpegs), 0, 2 if pcm is not None else 1,
                       largest, width, height, 0, 0, 0, 0)
    strh_v = struct.pack("<4s4sIHHIIIIIIiI4h", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, len(jpegs), largest, -1, 0, 0, 0, width, height)
    strf_v = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    hdrl = _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh_v) + _chunk(b"strf", strf_v))
    if pcm is not None:
        strh_a = struct.pack("<4s4sIHHIIIIIIiI4h", b"auds", b"\x00\x00\x00\x00", 0, 0, 0, 0, 1, int(sample_rate), 0, len(pcm) // 2, len(pcm),
                             -1, 2, 0, 0, 0, 0)
        strf_a = struct.pack("<HHIIHH", 1, 1, int(sample_rate), 2 * int(sample_rate), 2, 16)
        hdrl += _list(b"strl", _chunk(b"strh", strh_a) + _chunk(b"strf", strf_a))
    body = b"AVI " + _list(b"hdrl", hdrl) + _list(b"movi", b"".join(movi)) + _chunk(b"idx1", b"".join(index))
    if len(body) + 8 >= 1 << 32:
        raise ValueError("the clip does not fit into a 4 GiB AVI file")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return path
