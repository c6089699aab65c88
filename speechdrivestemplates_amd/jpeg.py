"""Baseline JPEG files from device frames (csrc/jpeg.hip): the renderer's (N, H, W, 3) uint8 BGR tensors are
transformed, quantised and Huffman-coded on the GPU, and only the compressed bytes cross to the host.

The files are baseline sequential (SOF0), YCbCr 4:2:0, one scan, the Annex K default Huffman tables, the Annex K quantisation tables
under the IJG quality scaling, and one restart interval per MCU row.  The arithmetic is integer only (the contract is in DESIGN.md
section 14 and include/sdt_hip.h), so the bytes are reproducible on a host.  The headers are built here, once per (H, W, quality); the
kernels receive the same tables, so what a header announces is what the scan was coded with.

    python -m speechdrivestemplates_amd.jpeg IN.npy OUT_PREFIX [--quality 95] [--rgb]
        IN.npy: (N, H, W, 3) or (H, W, 3) uint8 frames, BGR unless --rgb; writes OUT_PREFIX%06d.jpg
"""
import ctypes as C
import functools
import struct

import numpy as np

# ITU-T T.81 Annex K.1: luminance and chrominance quantisation tables, natural (row-major) order
BASE_LUM = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
            103, 99)
BASE_CHR = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) \
    + (99,) * 32
# Annex K.3: the default Huffman tables as (number of codes of length 1..16, symbols in code order)
DC_LUM = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHR = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUM = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),
          (1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36,
           51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74,
           83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133,
           134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179,
           180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
           225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250))
AC_CHR = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119),
          (0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21,
           98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72,
           73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131,
           132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170,
           178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216,
           217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250))

TABLE_WORDS = 672  # SDT_JPEG_TABLE_WORDS
ERR_STAGE, ERR_RANGE = 1, 2
MAX_WORKSPACE = 1 << 30  # bytes of coefficients per launch group: longer batches are cut into groups of whole images


def zigzag_order():
    """natural (row * 8 + column) index of the coefficient at each zigzag position"""
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, i // 8 if (i // 8 + i % 8) % 2 else i % 8))
    return tuple(order)


ZIGZAG = zigzag_order()


def quant_tables(quality):
    """IJG quality scaling of the Annex K tables -> (luminance, chrominance), natural order, values 1..255"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality must be in 1..100, got %r" % (quality,))
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(tuple(min(max((b * s + 50) // 100, 1), 255) for b in base) for base in (BASE_LUM, BASE_CHR))


def huffman_codes(spec, size):
    """(counts, symbols) -> ``size`` entries indexed by symbol: code | length << 16 (0 = the symbol has no code)"""
    counts, symbols = spec
    out = [0] * size
    code = k = 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = code | (length << 16)
            code += 1
            k += 1
        code <<= 1
    return out


def device_tables(quality):
    """the uint32 words csrc/jpeg.hip reads (include/sdt_hip.h: ``tables``)"""
    lum, chr_ = quant_tables(quality)
    words = list(lum) + list(chr_) + huffman_codes(DC_LUM, 16) + huffman_codes(DC_CHR, 16) + huffman_codes(AC_LUM, 256) + \
        huffman_codes(AC_CHR, 256)
    assert len(words) == TABLE_WORDS
    return np.asarray(words, np.uint32)


def _segment(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


@functools.lru_cache(maxsize=32)
def header(H, W, quality=95):
    """SOI, JFIF APP0 (1.01, density 1:1), two DQT, SOF0, four DHT, DRI (one MCU row), SOS: everything in front of the scan data"""
    H, W = int(H), int(W)
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError("JPEG dimensions must be in 1..65535, got %d x %d" % (H, W))
    lum, chr_ = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for idx, tab in ((0, lum), (1, chr_)):
        out += _segment(0xDB, bytes([idx]) + bytes(tab[i] for i in ZIGZAG))
    out += _segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (counts, symbols) in ((0x00, DC_LUM), (0x10, AC_LUM), (0x01, DC_CHR), (0x11, AC_CHR)):
        out += _segment(0xC4, bytes([tc_th]) + bytes(counts) + bytes(symbols))
    out += _segment(0xDD, struct.pack(">H", (W + 15) // 16))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


_tables_cache = {}


def _tables_on(device, quality):
    key = (str(device), int(quality))
    if key not in _tables_cache:
        import torch
        _tables_cache[key] = torch.from_numpy(device_tables(quality).view(np.int32)).to(device)
    return _tables_cache[key]


def _p(t):
    return C.c_void_p(t.data_ptr())


def _check_frames(frames):
    import torch
    if not torch.is_tensor(frames):
        raise TypeError("frames must be a torch tensor on the GPU")
    if frames.dtype != torch.uint8:
        raise ValueError("frames must be uint8, got %s" % frames.dtype)
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    if frames.dim() != 4 or frames.shape[-1] != 3 or min(frames.shape) < 1:
        raise ValueError("frames must be (N, H, W, 3) or (H, W, 3) with N, H, W >= 1, got %s" % (tuple(frames.shape),))
    if not frames.is_contiguous():
        raise ValueError("frames must be contiguous (the renderer's layout); call .contiguous() first")
    if max(frames.shape[1:3]) > 65535:
        raise ValueError("JPEG dimensions must be at most 65535, got %d x %d" % (frames.shape[1], frames.shape[2]))
    return frames


def encode_scans(frames, quality=95):
    """(N, H, W, 3) uint8 BGR device tensor -> list of N ``bytes``: each image's scan data up to and including EOI (no headers).
    Per launch group: the measuring launches size every interval, 16 bytes (the total and the error word) are read back, the packing launch writes into a
    buffer of exactly that size behind its offset table, and one pinned copy brings table and payload to the host."""
    import torch

    from . import _lib
    from .ops import _req_cuda, _stream
    frames = _check_frames(frames)
    _req_cuda(frames)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("JPEG encoding cannot run inside a hipGraph capture (it reads the compressed size back)")
    lib = _lib.load()
    N, H, W, _ = (int(v) for v in frames.shape)
    dev = frames.device
    tables = _tables_on(dev, quality)
    per_image = lib.sdt_jpeg_workspace_bytes(1, H, W)
    if per_image <= 0:
        raise ValueError("unsupported frame size %d x %d" % (H, W))
    group = max(1, min(N, MAX_WORKSPACE // per_image, 65535))
    rows = (H + 15) // 16
    st = _stream()
    scans = []
    for first in range(0, N, group):
        part = frames[first:first + group]
        n = int(part.shape[0])
        ws_bytes = lib.sdt_jpeg_workspace_bytes(n, H, W)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        n_off = n * rows + 1
        head = torch.empty(n_off + 1, dtype=torch.int64, device=dev)  # offsets, then the error word
        err = head[n_off:].view(torch.int32)
        _lib.check(lib.sdt_jpeg_measure(_p(part), part.numel(), n, H, W, _p(tables), _p(ws), ws_bytes, _p(head), n_off, _p(err), st))
        total, flags = (int(v) for v in head[n_off - 1:].cpu())  # the one readback before the payload: 16 bytes
        if flags & 0xffffffff:
            raise RuntimeError("JPEG encoder reported error word %d while measuring (malformed tables?)" % (flags & 0xffffffff))
        packed = torch.empty((n_off + 1) * 8 + total, dtype=torch.uint8, device=dev)
        phead = packed[:(n_off + 1) * 8].view(torch.int64)
        phead.copy_(head)
        perr = phead[n_off:].view(torch.int32)
        payload = packed[(n_off + 1) * 8:]
        _lib.check(lib.sdt_jpeg_pack(_p(ws), ws_bytes, n, H, W, _p(tables), _p(phead), n_off, _p(payload), total, _p(perr), st))
        host = torch.empty(packed.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(packed, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        buf = host.numpy()
        table = buf[:(n_off + 1) * 8].view(np.int64)
        flags = int(table[n_off:].view(np.int32)[0])
        if flags:
            raise RuntimeError("JPEG encoder reported error word %d (%s)" % (
                flags, ", ".join(s for b, s in ((ERR_STAGE, "an MCU exceeded the staging buffer"),
                                                (ERR_RANGE, "a byte position left its interval's range")) if flags & b)))
        data = buf[(n_off + 1) * 8:]
        for i in range(n):
            scans.append(data[table[i * rows]:table[(i + 1) * rows]].tobytes())
    return scans


def encode_frames(frames, quality=95):
    """(N, H, W, 3) (or (H, W, 3)) uint8 BGR device tensor -> list of N complete baseline JPEG files as ``bytes``"""
    frames = _check_frames(frames)
    head = header(int(frames.shape[1]), int(frames.shape[2]), int(quality))
    return [head + s for s in encode_scans(frames, quality)]


def main(argv=None):
    import argparse

    import torch
    ap = argparse.ArgumentParser(description="encode a saved frame array to JPEG files on the GPU")
    ap.add_argument("frames", help=".npy file: (N, H, W, 3) or (H, W, 3) uint8")
    ap.add_argument("out_prefix", help="files are written as OUT_PREFIX%%06d.jpg")
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--rgb", action="store_true", help="the array is RGB (default: BGR, the renderer's order)")
    a = ap.parse_args(argv)
    x = np.load(a.frames)
    if x.dtype != np.uint8 or x.ndim not in (3, 4) or x.shape[-1] != 3:
        raise SystemExit("expected a uint8 array of shape (N, H, W, 3) or (H, W, 3), got %s %s" % (x.dtype, x.shape))
    if x.ndim == 3:
        x = x[None]
    if a.rgb:
        x = x[..., ::-1]
    files = encode_frames(torch.from_numpy(np.ascontiguousarray(x)).cuda(), a.quality)
    for i, data in enumerate(files):
        with open("%s%06d.jpg" % (a.out_prefix, i), "wb") as f:
            f.write(data)
    print("wrote %d files, %d bytes" % (len(files), sum(len(d) for d in files)))


if __name__ == "__main__":
    main()
