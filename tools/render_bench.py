#!/usr/bin/env python
"""Skeleton renderer timing (csrc/render.hip).  Not bench.py: this measures the opt-in video path only.

Four cases: 64 single-view frames at 720x1280, 64 pair frames, a T = 360 long image, a batch of 32 clips x 64 frames.  Every
shape is warmed up first; then the prepare + raster launches are timed with HIP events over enough repeats to fill ~1 s per case.
Reported: us per call, frames/s, frame bytes written per second and that rate as a fraction of the 8 TB/s HBM peak (frame bytes only:
the floor this kernel is bound by).  Also one end-to-end VideoWriter.save_video of the 64-frame pair clip split into render / D2H /
encode (JPEG frames; ffmpeg if it is on PATH), with SYS.DEVICE_JPEG off and on (on: the frames are encoded by csrc/jpeg.hip and
"d2h" is the GPU encode plus the compressed copy), and the JPEG encoder alone on the 64 pair frames and the long
image: HIP events around the three launches (transform + measure + scan, then pack), without the size readback and the copy.  One JSON
line per case.

    python tools/render_bench.py [--seconds 1.0] [--no-e2e] [--no-render]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechdrivestemplates_amd import render  # noqa: E402

HBM_PEAK = 8.0e12


def poses(n, T, seed):
    rng = np.random.default_rng(seed)
    body = rng.uniform(-300.0, 300.0, size=(n, 1, 2, 121))
    return torch.from_numpy(body + rng.normal(0.0, 12.0, size=(n, T, 2, 121))).cuda()


def case(name, x, inst_rows, n_images, n_inst, H, W, seconds):
    flat = x.reshape(-1, 2, 121).contiguous()
    out, ws, skipped, inst = render._launch(flat, inst_rows, n_images, n_inst, H, W)
    for _ in range(3):
        render._launch(flat, inst_rows, n_images, n_inst, H, W, out)
    torch.cuda.synchronize()
    lib = render._lib.load()
    p = render._p
    st = render._stream()

    def once():
        render._lib.check(lib.sdt_render_prepare_f64(p(flat), flat.shape[0], 121, p(inst), n_images, n_inst, H, W, p(ws), ws.numel(),
                                                     p(skipped), st))
        render._lib.check(lib.sdt_render_skeleton_u8(p(ws), ws.numel(), n_images, n_inst, 121, H, W, p(out), out.numel(), st))

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        once()
    e1.record()
    e1.synchronize()
    per = e0.elapsed_time(e1) / 5e3
    reps = max(10, int(seconds / max(per, 1e-6)))
    e0.record()
    for _ in range(reps):
        once()
    e1.record()
    e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    nbytes = out.numel()
    r = {"case": name, "images": n_images, "H": H, "W": W, "strokes_per_image": n_inst * lib.sdt_render_edges(121), "reps": reps,
         "us": round(us, 2), "frames_per_s": round(n_images / us * 1e6, 1), "frame_bytes": nbytes,
         "write_GB_per_s": round(nbytes / us * 1e-3, 1), "fraction_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)}
    print(json.dumps(r), flush=True)
    return r


def jpeg_case(name, frames, seconds, quality=95):
    """the encoder's launches alone, on frames that stay on the device"""
    import ctypes as C

    from speechdrivestemplates_amd import jpeg
    lib = render._lib.load()
    N, H, W, _ = (int(v) for v in frames.shape)
    files = jpeg.encode_frames(frames, quality)  # warm-up, and the sizes for the report
    tables = jpeg._tables_on(frames.device, quality)
    ws_bytes = lib.sdt_jpeg_workspace_bytes(N, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    n_off = int(lib.sdt_jpeg_intervals(N, H, W)) + 1
    head = torch.empty(n_off + 1, dtype=torch.int64, device="cuda")
    payload = sum(len(f) for f in files) - N * len(jpeg.header(H, W, quality))
    out = torch.empty(payload, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    st = render._stream()

    def once():
        render._lib.check(lib.sdt_jpeg_measure(p(frames), frames.numel(), N, H, W, p(tables), p(ws), ws_bytes, p(head), n_off,
                                               p(head[n_off:]), st))
        render._lib.check(lib.sdt_jpeg_pack(p(ws), ws_bytes, N, H, W, p(tables), p(head), n_off, p(out), payload, p(head[n_off:]), st))

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        once()
    e1.record()
    e1.synchronize()
    per = e0.elapsed_time(e1) / 3e3
    reps = max(5, int(seconds / max(per, 1e-6)))
    e0.record()
    for _ in range(reps):
        once()
    e1.record()
    e1.synchronize()
    assert int(head[n_off:].view(torch.int32)[0].item()) == 0
    us = e0.elapsed_time(e1) * 1e3 / reps
    t0 = time.perf_counter()
    jpeg.encode_frames(frames, quality)
    wall = time.perf_counter() - t0
    r = {"case": name, "images": N, "H": H, "W": W, "quality": quality, "reps": reps, "us": round(us, 1),
         "frames_per_s": round(N / us * 1e6, 1), "raw_bytes": frames.numel(), "jpeg_bytes": payload,
         "read_GB_per_s": round(frames.numel() / us * 1e-3, 1), "encode_frames_wall_ms": round(wall * 1e3, 2)}
    print(json.dumps(r), flush=True)
    return r


def e2e(seconds, device_jpeg=False):
    from speechdrivestemplates_amd.config import get_cfg_defaults
    from speechdrivestemplates_amd.video import VideoWriter
    cfg = get_cfg_defaults()
    cfg.merge_from_list(["SYS.VIDEO_FORMAT", ["mp4"], "SYS.DEVICE_JPEG", device_jpeg])
    cfg.freeze()
    p, g = poses(1, 64, 5)[0], poses(1, 64, 6)[0]
    render.render_pose_pair_clip(p, g)
    torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        frames = render.render_pose_pair_clip(p, g)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        w = VideoWriter(cfg)
        w.save_video(cfg, "TEST", frames, 1, 1, audio=np.zeros(16000 * 64 // 15, np.float32), base_path=d)
        t2 = time.perf_counter()
        r = {"case": "save_video_pair64_e2e" + ("_device_jpeg" if device_jpeg else ""), "render_ms": round((t1 - t0) * 1e3, 2), "d2h_ms": round(w.last_timing["d2h"] * 1e3, 2),
             "encode_ms": round(w.last_timing["encode"] * 1e3, 1), "total_ms": round((t2 - t0) * 1e3, 1),
             "encoder": "ffmpeg" if os.path.exists(os.path.join(d, "videos", "epoch1-TEST-step1.mp4")) else "jpeg frames only (no ffmpeg)"}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--no-render", action="store_true", help="skip the four renderer cases")
    a = ap.parse_args()
    torch.cuda.init()
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    s = a.seconds
    if not a.no_render:
        x = poses(1, 64, 1)
        case("single_64x720x1280", x, render.clip_instances(64, (720, 1280), 0.85), 64, 1, 720, 1280, s)
        both = torch.cat([x.reshape(64, 2, 121), poses(1, 64, 2).reshape(64, 2, 121)], 0)
        case("pair_64x720x1280", both, render.pair_instances(64, (720, 1280), 0.85), 64, 2, 720, 1280, s)
        width, n_win, rows = render.long_instances(1, 360)
        case("long_T360_720x%d" % width, poses(1, 360, 3), rows, 1, n_win, 720, width, s)
        case("batch_32x64x720x1280", poses(32, 64, 4), render.clip_instances(32 * 64, (720, 1280), 0.85), 32 * 64, 1, 720, 1280, s)
    jpeg_case("jpeg_pair_64x720x1280", render.render_pose_pair_clip(poses(1, 64, 5)[0], poses(1, 64, 6)[0]), s)
    jpeg_case("jpeg_long_T360", render.render_long_image(poses(1, 360, 3)[0])[None], s)
    if not a.no_e2e:
        e2e(s)
        e2e(s, device_jpeg=True)


if __name__ == "__main__":
    main()
