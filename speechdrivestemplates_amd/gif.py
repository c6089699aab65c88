"""Animated GIF files from device frames (csrc/gif.hip): the renderer's (T, H, W, 3) uint8 BGR tensors are
shrunk by 0.4 (the reference's ``F.interpolate(scale_factor=0.4, mode='area')`` of its TensorBoard route), quantised to one 256-colour
palette and LZW-coded on the GPU; only the compressed bytes cross to the host, which adds the container.

The contract is integer only (include/sdt_hip.h) and the ``model_*`` functions below are its numpy statement: the GPU path returns
their bytes exactly.  They are also the host route of numpy frames (video.py uses ``model_downscale``) and the reference of the tests.

    python -m speechdrivestemplates_amd.gif IN.npy OUT.gif [--fps 15] [--no-downscale] [--rgb]
        IN.npy: (T, H, W, 3) or (H, W, 3) uint8 frames, BGR unless --rgb
"""
import ctypes as C
import struct

import numpy as np

ERR_RANGE = 1  # SDT_GIF_ERR_RANGE
ERR_COUNT = 2  # SDT_GIF_ERR_COUNT
MAX_SEGMENT = 3838  # 4096 - 258: the code table cannot fill inside a segment
CLEAR, EOI, FIRST_FREE = 256, 257, 258


# -- the contract in numpy ----------------------------------------------------------------------------------------------------------
def out_size(H, W, downscale=True):
    return ((2 * H) // 5, (2 * W) // 5) if downscale else (H, W)


def _windows(n_in, n_out):
    i = np.arange(n_out, dtype=np.int64)
    return (i * n_in) // n_out, ((i + 1) * n_in + n_out - 1) // n_out


def model_downscale(frames, downscale=True):
    """(T, H, W, 3) uint8 BGR -> (T, h, w, 3) uint8 RGB: the mean over source rows [floor(i H / h), ceil((i + 1) H / h)) and the same
    range of columns, as (sum + n // 2) // n"""
    x = np.asarray(frames)
    T, H, W, _ = x.shape
    h, w = out_size(H, W, downscale)
    if h < 1 or w < 1:
        raise ValueError("frames of %d x %d are too small to shrink by 0.4" % (H, W))
    r0, r1 = _windows(H, h)
    c0, c1 = _windows(W, w)
    n = ((r1 - r0)[:, None] * (c1 - c0)[None, :])[:, :, None]
    out = np.empty((T, h, w, 3), np.uint8)
    s = np.zeros((H + 1, W + 1, 3), np.int64)  # inclusive prefix sums along both axes behind a zero row / column
    for t in range(T):
        s[1:, 1:] = x[t, :, :, ::-1].astype(np.int64).cumsum(0).cumsum(1)
        tot = s[r1][:, c1] - s[r0][:, c1] - s[r1][:, c0] + s[r0][:, c0]
        out[t] = (tot + n // 2) // n
    return out


def model_bins(rgb):
    r = np.asarray(rgb).astype(np.uint16) >> 3
    return (r[..., 0] << 10) | (r[..., 1] << 5) | r[..., 2]


def model_palette(hist):
    """32768 counts -> (palette bins ascending, (256, 3) uint8 palette, (32768,) uint8 bin -> palette index)"""
    hist = np.asarray(hist, np.int64)
    occupied = np.nonzero(hist)[0]
    if len(occupied) > 256:
        order = np.lexsort((occupied, -hist[occupied]))  # most populated first, the lower bin first among equals
        occupied = np.sort(occupied[order[:256]])
    c5 = np.stack([occupied >> 10, (occupied >> 5) & 31, occupied & 31], 1).astype(np.int32)
    palette = np.zeros((256, 3), np.uint8)
    palette[:len(occupied)] = (c5 << 3) | (c5 >> 2)
    b = np.arange(32768, dtype=np.int32)
    d = sum((((b >> sh) & 31)[:, None] - c5[None, :, k]) ** 2 for k, sh in enumerate((10, 5, 0)))
    return occupied.astype(np.uint16), palette, d.argmin(1).astype(np.uint8)  # argmin: the first of equals


def model_quantise(frames, downscale=True):
    """-> (rgb (T, h, w, 3), indices (T, h, w) uint8, palette (256, 3) uint8)"""
    rgb = model_downscale(frames, downscale)
    bins = model_bins(rgb)
    _, palette, table = model_palette(np.bincount(bins.ravel(), minlength=32768))
    return rgb, table[bins], palette


def segments(w):
    """the (start, length) pieces one output row is coded in"""
    parts = -(-w // MAX_SEGMENT)
    step = -(-w // parts)
    return [(s, min(step, w - s)) for s in range(0, w, step)]


def width_after(k):
    """the code width after k codes of a segment"""
    return 9 + (k >= 255) + (k >= 767) + (k >= 1791)


def model_lzw_segment(pixels):
    """one segment's codes from an empty table (without the Clear around them)"""
    table = {}
    codes = []
    cur = int(pixels[0])
    for b in pixels[1:]:
        key = (cur << 8) | int(b)
        hit = table.get(key)
        if hit is not None:
            cur = hit
        else:
            codes.append(cur)
            table[key] = FIRST_FREE + len(table)
            cur = int(b)
    codes.append(cur)
    return codes


def model_frame_codes(indices):
    """(h, w) uint8 -> (codes, widths) of the frame's stream: Clear, then per segment its codes and a Clear (after the last one: EOI)
    at the width the segment ended in"""
    codes, widths = [CLEAR], [9]
    for row in np.asarray(indices):
        for s, n in segments(len(row)):
            width, next_code = 9, FIRST_FREE
            for code in model_lzw_segment(row[s:s + n].tolist()):
                codes.append(code)
                widths.append(width)
                next_code += 1
                if next_code > (1 << width) and width < 12:
                    width += 1
            codes.append(CLEAR)
            widths.append(width)
    codes[-1] = EOI
    return np.asarray(codes, np.int64), np.asarray(widths, np.int64)


def model_frame_stream(indices):
    """(h, w) uint8 -> the frame's LZW stream as bytes, codes packed LSB first, the last byte padded with 0-bits"""
    codes, widths = model_frame_codes(indices)
    start = np.cumsum(widths) - widths
    bits = np.zeros(int(widths.sum()), np.uint8)
    for j in range(12):
        m = widths > j
        bits[start[m] + j] = (codes[m] >> j) & 1
    return np.packbits(bits, bitorder="little").tobytes()


def container(streams, h, w, palette, fps):
    """the GIF89a file around the frames' LZW streams"""
    delay = int(round(100.0 / fps))
    out = [b"GIF89a", struct.pack("<HHBBB", w, h, 0xF7, 0, 0), np.asarray(palette, np.uint8).reshape(256, 3).tobytes(),
           b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00"]
    for stream in streams:
        out.append(b"\x21\xf9\x04\x00" + struct.pack("<H", delay) + b"\x00\x00")
        out.append(b"\x2c" + struct.pack("<HHHHB", 0, 0, w, h, 0) + b"\x08")
        data = np.frombuffer(stream, np.uint8)
        full = len(data) // 255
        blocks = np.empty((full, 256), np.uint8)
        blocks[:, 0] = 255
        blocks[:, 1:] = data[:full * 255].reshape(full, 255)
        out.append(blocks.tobytes())
        rest = data[full * 255:]
        if len(rest):
            out.append(bytes([len(rest)]) + rest.tobytes())
        out.append(b"\x00")
    out.append(b"\x3b")
    return b"".join(out)


def model_encode_gif(frames, fps, downscale=True):
    _, indices, palette = model_quantise(frames, downscale)
    return container([model_frame_stream(f) for f in indices], indices.shape[1], indices.shape[2], palette, fps)


# -- the GPU path -------------------------------------------------------------------------------------------------------------------
def _p(t):
    return C.c_void_p(t.data_ptr())


def _check_frames(frames, downscale):
    import torch
    if not torch.is_tensor(frames):
        raise TypeError("frames must be a torch tensor on the GPU")
    if frames.dtype != torch.uint8:
        raise ValueError("frames must be uint8, got %s" % frames.dtype)
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    if frames.dim() != 4 or frames.shape[-1] != 3 or min(frames.shape) < 1:
        raise ValueError("frames must be (T, H, W, 3) or (H, W, 3) with T, H, W >= 1, got %s" % (tuple(frames.shape),))
    if not frames.is_contiguous():
        raise ValueError("frames must be contiguous (the renderer's layout); call .contiguous() first")
    T, H, W, _ = (int(v) for v in frames.shape)
    h, w = out_size(H, W, downscale)
    if h < 1 or w < 1:
        raise ValueError("frames of %d x %d are too small to shrink by 0.4" % (H, W))
    if max(h, w) > 65535 or T > 65535:
        raise ValueError("GIF dimensions and frame count must be at most 65535, got %d frames of %d x %d" % (T, h, w))
    if T * H * W * 3 >= 1 << 40:
        raise ValueError("clip too large")
    return frames, (T, H, W, h, w)


def _quantise(frames, downscale, want_rgb):
    import torch

    from . import _lib
    from .ops import _req_cuda, _stream
    frames, (T, H, W, h, w) = _check_frames(frames, downscale)
    _req_cuda(frames)
    lib = _lib.load()
    dev = frames.device
    ws_bytes = lib.sdt_gif_workspace_bytes(T, h, w)
    if ws_bytes <= 0:
        raise ValueError("unsupported clip size: %d frames of %d x %d" % (T, h, w))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rgb = torch.empty((T, h, w, 3), dtype=torch.uint8, device=dev) if want_rgb else None
    indices = torch.empty((T, h, w), dtype=torch.uint8, device=dev)
    palette = torch.empty((256, 3), dtype=torch.uint8, device=dev)
    _lib.check(lib.sdt_gif_quantise(_p(frames), frames.numel(), T, H, W, h, w, None if rgb is None else _p(rgb),
                                    0 if rgb is None else rgb.numel(), _p(indices), indices.numel(), _p(palette), _p(ws), ws_bytes, _stream()))
    return rgb, indices, palette, ws, ws_bytes


def quantise(frames, downscale=True):
    """(T, H, W, 3) uint8 BGR device tensor -> (rgb (T, h, w, 3), indices (T, h, w), palette (256, 3)) uint8 device tensors"""
    return _quantise(frames, downscale, True)[:3]


def encode_gif(frames, fps, downscale=True):
    """(T, H, W, 3) uint8 BGR device tensor -> one animated GIF89a file as ``bytes``.  Quantise, measure, one readback of 16 bytes (the
    total and the error word), pack into a buffer of that size, one pinned copy, host framing."""
    import torch

    from . import _lib
    from .ops import _stream
    if not fps > 0:
        raise ValueError("fps must be positive, got %r" % (fps,))
    if torch.is_tensor(frames) and frames.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("GIF encoding cannot run inside a hipGraph capture (it reads the compressed size back)")
    _, indices, palette, ws, ws_bytes = _quantise(frames, downscale, False)
    lib = _lib.load()
    T, h, w = (int(v) for v in indices.shape)
    dev = indices.device
    st = _stream()
    n_off = T + 1 + T * h * len(segments(w))
    head = torch.empty(n_off + 1, dtype=torch.int64, device=dev)  # frame byte offsets, segment bit offsets, then the error word
    err = head[n_off:].view(torch.int32)
    _lib.check(lib.sdt_gif_measure(_p(indices), indices.numel(), T, h, w, _p(ws), ws_bytes, _p(head), n_off, _p(err), st))
    total, flags = (int(v) for v in head[[T, n_off]].cpu())  # the one readback before the payload
    if flags & 0xffffffff:
        raise RuntimeError("GIF encoder reported error word %d while measuring" % (flags & 0xffffffff))
    # | palette 768 | error word 8 | frame offsets 8 (T + 1) | payload, padded to whole words |
    lead = 768 + 8 + 8 * (T + 1)
    padded = (total + 3) & ~3
    packed = torch.empty(lead + padded, dtype=torch.uint8, device=dev)
    packed[:768].copy_(palette.view(-1))
    perr = packed[768:776].view(torch.int32)
    perr.zero_()
    packed[776:lead].view(torch.int64).copy_(head[:T + 1])
    payload = packed[lead:]
    _lib.check(lib.sdt_gif_pack(_p(ws), ws_bytes, T, h, w, _p(head), n_off, _p(payload), padded, _p(perr), st))
    host = torch.empty(packed.shape, dtype=torch.uint8, pin_memory=True)
    host.copy_(packed, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    buf = host.numpy()
    flags = int(buf[768:772].view(np.int32)[0])
    if flags:
        raise RuntimeError("GIF encoder reported error word %d (%s)" % (
            flags, ", ".join(s for b, s in ((ERR_RANGE, "a word position left its frame's range"),
                                            (ERR_COUNT, "a segment's code count exceeds its length")) if flags & b)))
    offs = buf[776:lead].view(np.int64)
    data = buf[lead:]
    return container([data[offs[i]:offs[i + 1]].tobytes() for i in range(T)], h, w, buf[:768], fps)


def main(argv=None):
    import argparse

    import torch
    ap = argparse.ArgumentParser(description="encode a saved frame array to an animated GIF on the GPU")
    ap.add_argument("frames", help=".npy file: (T, H, W, 3) or (H, W, 3) uint8")
    ap.add_argument("out", help="the GIF file to write")
    ap.add_argument("--fps", type=float, default=15)
    ap.add_argument("--no-downscale", action="store_true", help="keep the frame size (default: shrink by 0.4 like the reference)")
    ap.add_argument("--rgb", action="store_true", help="the array is RGB (default: BGR, the renderer's order)")
    a = ap.parse_args(argv)
    x = np.load(a.frames)
    if x.dtype != np.uint8 or x.ndim not in (3, 4) or x.shape[-1] != 3:
        raise SystemExit("expected a uint8 array of shape (T, H, W, 3) or (H, W, 3), got %s %s" % (x.dtype, x.shape))
    if x.ndim == 3:
        x = x[None]
    if a.rgb:
        x = x[..., ::-1]
    data = encode_gif(torch.from_numpy(np.ascontiguousarray(x)).cuda(), a.fps, not a.no_downscale)
    with open(a.out, "wb") as f:
        f.write(data)
    print("wrote %s: %d frames, %d bytes" % (a.out, x.shape[0], len(data)))


if __name__ == "__main__":
    main()
