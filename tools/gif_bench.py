#!/usr/bin/env python
"""GIF encoder timing (csrc/gif.hip).  Not bench.py: this measures the opt-in TensorBoard video route only.

The clips are the 64-frame pair clip the trainer saves, 720x1280 -> 288x512, and the same poses on a 720x2560 canvas -> 288x1024.
Reported per clip, one JSON line each:
  stages    HIP events around the three library calls (quantise = downscale + histogram, palette, map, index; measure = LZW + scan;
            pack), median and spread over the repeats after a warm-up.  Per-kernel times come from a kernel trace of this tool
            (rocprofv3 --kernel-trace --stats -- python tools/gif_bench.py --no-host).
  encode    gif.encode_gif end to end (host clock around a call that ends in a synchronise), the output size, and the PSNR of the
            quantised frames against the downscaled RGB.
  host      the same frames through the host route: numpy downscale + PIL quantize(256, dither=NONE) + save_all; its time and size; the
            PSNR of PIL's median-cut single palette over the stacked clip; and the byte ratio of our row-restart LZW to PIL's
            single-stream LZW on OUR indices (the cost of independent segments).

    python tools/gif_bench.py [--repeats 20] [--no-host] [--out profiles/r11_gif_bench.jsonl]
"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechdrivestemplates_amd import _lib, gif, render  # noqa: E402
from speechdrivestemplates_amd.ops import _stream  # noqa: E402


def poses(T, seed):
    rng = np.random.default_rng(seed)
    body = rng.uniform(-300.0, 300.0, size=(1, 2, 121))
    return torch.from_numpy(body + rng.normal(0.0, 12.0, size=(T, 2, 121))).cuda()


def spread(xs):
    xs = sorted(xs)
    return {"median": round(statistics.median(xs), 2), "min": round(xs[0], 2), "max": round(xs[-1], 2)}


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else round(10 * np.log10(255.0 ** 2 / mse), 2)


def stages(frames, repeats):
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    T, H, W, _ = (int(v) for v in frames.shape)
    h, w = gif.out_size(H, W)
    ws_bytes = lib.sdt_gif_workspace_bytes(T, h, w)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    indices = torch.empty((T, h, w), dtype=torch.uint8, device="cuda")
    palette = torch.empty((256, 3), dtype=torch.uint8, device="cuda")
    n_off = T + 1 + T * h * len(gif.segments(w))
    head = torch.empty(n_off + 1, dtype=torch.int64, device="cuda")
    err = head[n_off:].view(torch.int32)
    st = _stream()
    out = None
    times = {"quantise": [], "measure": [], "pack": []}
    for rep in range(repeats + 3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        _lib.check(lib.sdt_gif_quantise(p(frames), frames.numel(), T, H, W, h, w, None, 0, p(indices), indices.numel(), p(palette), p(ws),
                                        ws_bytes, st))
        ev[1].record()
        _lib.check(lib.sdt_gif_measure(p(indices), indices.numel(), T, h, w, p(ws), ws_bytes, p(head), n_off, p(err), st))
        ev[2].record()
        if out is None:
            out = torch.empty((int(head[T].item()) + 3) & ~3, dtype=torch.uint8, device="cuda")
            ev[2].record()
        _lib.check(lib.sdt_gif_pack(p(ws), ws_bytes, T, h, w, p(head), n_off, p(out), out.numel(), p(err), st))
        ev[3].record()
        ev[3].synchronize()
        if rep >= 3:  # (three warm-up rounds)
            for k, name in enumerate(("quantise", "measure", "pack")):
                times[name].append(ev[k].elapsed_time(ev[k + 1]) * 1e3)
    assert int(err[0].item()) == 0
    return {"case": "stages_us", "frames": T, "in": [H, W], "out": [h, w], "repeats": repeats, **{k: spread(v) for k, v in times.items()},
            "stream_bytes": int(head[T].item())}


def encode(frames, repeats):
    for _ in range(3):
        data = gif.encode_gif(frames, 15)
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data = gif.encode_gif(frames, 15)
        times.append((time.perf_counter() - t0) * 1e3)
    rgb, indices, palette = gif.quantise(frames)
    rgb, indices, palette = rgb.cpu().numpy(), indices.cpu().numpy(), palette.cpu().numpy()
    r = {"case": "encode_gif_ms", "repeats": repeats, **spread(times), "gif_bytes": len(data), "raw_bytes": frames.numel(),
         "occupied_bins": int(len(np.unique(gif.model_bins(rgb)))), "psnr_db": psnr(palette[indices], rgb)}
    return r, data, rgb, indices, palette


def host(frames_np, rgb, indices, palette, ours):
    from PIL import Image
    t0 = time.perf_counter()
    small = gif.model_downscale(frames_np)
    t1 = time.perf_counter()
    images = [Image.fromarray(f).quantize(256, dither=Image.Dither.NONE) for f in small]
    buf = io.BytesIO()
    images[0].save(buf, "GIF", save_all=True, append_images=images[1:], duration=70, loop=0)
    t2 = time.perf_counter()
    assert (small == rgb).all()
    T, h, w, _ = small.shape
    stacked = Image.fromarray(small.reshape(T * h, w, 3)).quantize(256, dither=Image.Dither.NONE)
    stacked_rgb = np.asarray(stacked.convert("RGB")).reshape(T, h, w, 3)
    # our indices and palette through PIL's single-stream LZW: what the row restarts cost in bytes
    pim = []
    for f in indices:
        im = Image.fromarray(f, "P")
        im.putpalette(palette.tobytes())
        pim.append(im)
    one = io.BytesIO()
    pim[0].save(one, "GIF", save_all=True, append_images=pim[1:], duration=70, loop=0, optimize=False, disposal=0)
    return {"case": "host_route", "downscale_ms": round((t1 - t0) * 1e3, 1), "pil_quantize_save_ms": round((t2 - t1) * 1e3, 1),
            "total_ms": round((t2 - t0) * 1e3, 1), "gif_bytes": len(buf.getvalue()), "psnr_db_pil_median_cut_single_palette": psnr(stacked_rgb, small),
            "pil_single_stream_bytes_on_our_indices": len(one.getvalue()), "row_restart_byte_ratio": round(len(ours) / len(one.getvalue()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    torch.cuda.init()
    lines = [{"device": torch.cuda.get_device_name(0)}]
    # the pair clip as the trainer draws it (both skeletons on one 720 x 1280 canvas), and the same poses on a canvas twice as wide
    for canvas in ((720, 1280), (720, 2560)):
        frames = render.render_pose_pair_clip(poses(64, 5), poses(64, 6), canvas, 0.85)
        lines.append(stages(frames, a.repeats))
        r, data, rgb, indices, palette = encode(frames, a.repeats)
        lines.append(r)
        if not a.no_host:
            lines.append(host(frames.cpu().numpy(), rgb, indices, palette, data))
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
