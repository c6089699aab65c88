"""Time the three launches of the audio strip (csrc/audio_strip.hip) on a 64-frame clip and on a 900-frame segment of
720 x 1280 frames with a band of 160 rows.  One JSON line per piece, HIP events around each launch, 3 warm-up calls, then the median and the
minimum of --reps calls:
    envelope / raster / compose   the launches of sdt_strip_envelope_f32, sdt_strip_raster_u8 and sdt_strip_compose_u8 (tables and outputs
                                  are uploaded and allocated before the timed window)
    render                        render.render_pose_clip of as many poses at the same canvas (it allocates its output inside the call)
    copy                          out[:, :H] = frames with torch slicing into a preallocated (n, H + S, W, 3) tensor: the frames' rows only,
                                  the floor of the compose pass
    compose_over_copy, compose_gbs, copy_gbs   compose moves n (H + (H + S)) W 3 bytes (frames read, out written; the band's rows are read from
                                  a few MB that stay in cache), the copy n 2 H W 3
Appends to profiles/r32_audio_strip_bench.jsonl.

    python tools/audio_strip_bench.py [--reps 20] [--out profiles/r32_audio_strip_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from speechdrivestemplates_amd import _lib  # noqa: E402
from speechdrivestemplates_amd import audio_strip as st  # noqa: E402
from speechdrivestemplates_amd import render  # noqa: E402
from speechdrivestemplates_amd.ops import _stream  # noqa: E402

H, W, S, WARMUP = 720, 1280, 160, 3


def event_ms(fn, reps):
    """-> (median, minimum) milliseconds between two events around fn, after WARMUP calls"""
    times = []
    for i in range(WARMUP + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= WARMUP:
            times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def bench(n, reps):
    rng = np.random.Generator(np.random.PCG64(n))
    L = n * st.SAMPLE_RATE // st.FPS
    audio = torch.from_numpy((rng.standard_normal(L) * 0.1).astype(np.float32)).cuda()
    mel = torch.from_numpy((rng.standard_normal((80, 1 + L // st.HOP)) ** 2).astype(np.float32)).cuda()
    marks = [np.arange(3, L * 300 // 16000, 150), np.arange(10, n * 20, 100), None]
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda")
    poses = torch.from_numpy(rng.standard_normal((n, 2, 121)).cumsum(0) * 4.0).cuda()
    bounds, c0, ph = st.clip_layout(n, W, L, 4.3)
    Nc = bounds.size - 1
    lib, p = _lib.load(), st._p
    b_dev = torch.from_numpy(bounds).cuda()
    ticks = [torch.from_numpy(t).cuda() for t in st._ticks(marks)]
    cmap, k_dev = torch.from_numpy(st.colormap()).cuda(), torch.from_numpy(st.factor_table(80.0)).cuda()
    env, flags = torch.empty((Nc, 2), dtype=torch.float32, device="cuda"), torch.empty(Nc, dtype=torch.int32, device="cuda")
    stats, work = torch.empty(2, dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda")
    band = torch.empty((S, Nc, 3), dtype=torch.uint8, device="cuda")
    tables = torch.from_numpy(np.stack([c0, ph])).cuda()
    out = torch.empty((n, H + S, W, 3), dtype=torch.uint8, device="cuda")
    colours, bg, head = st._bytes3((st.BACKGROUND, st.WAVE, st.WARNING) + st.MARKS), st._bytes3((st.BACKGROUND,)), st._bytes3((st.PLAYHEAD,))

    def envelope():
        _lib.check(lib.sdt_strip_envelope_f32(p(audio), L, p(b_dev), Nc, p(env), p(flags), p(stats), _stream()))

    def raster():
        _lib.check(lib.sdt_strip_raster_u8(p(env), p(flags), p(stats), p(b_dev), Nc, p(mel), mel.shape[0], mel.shape[1], p(cmap), p(k_dev),
                                           p(ticks[0]), ticks[0].numel(), p(ticks[1]), ticks[1].numel(), p(ticks[2]), ticks[2].numel(), colours, S,
                                           p(work), p(band), _stream()))

    def compose():
        _lib.check(lib.sdt_strip_compose_u8(p(frames), n, H, W, p(band), S, Nc, p(tables[0]), p(tables[1]), bg, head, p(out), out.numel(),
                                            _stream()))

    def copy():
        out[:, :H] = frames

    line = {"tool": "audio_strip_bench", "device": torch.cuda.get_device_name(0), "reps": reps, "warmup": WARMUP, "frames": n,
            "canvas": [H, W], "height": S, "samples": L, "columns": Nc, "scrolls": bool((c0 != 0).any()),
            "vectorised": int(lib.sdt_strip_compose_vectorised(p(frames), W, p(out)))}
    for name, fn in (("envelope", envelope), ("raster", raster), ("compose", compose), ("copy", copy),
                     ("render", lambda: render.render_pose_clip(poses, (H, W)))):
        line[name + "_ms"], line[name + "_min_ms"] = event_ms(fn, reps)
    want = st.compose_model(frames[:2].cpu().numpy(), band.cpu().numpy(), c0[:2], ph[:2])
    assert np.array_equal(out[:2].cpu().numpy(), want) and torch.equal(out[-1, :H], frames[-1])  # (what was timed is the feature's result)
    line["compose_over_copy"] = line["compose_ms"] / line["copy_ms"]
    line["compose_gbs"] = n * (2 * H + S) * W * 3 / line["compose_ms"] / 1e6
    line["copy_gbs"] = n * 2 * H * W * 3 / line["copy_ms"] / 1e6
    return line


def main(argv=None):
    ap = argparse.ArgumentParser(description="time the audio strip's three launches beside the renderer and a plain copy of the frames")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r32_audio_strip_bench.jsonl"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("the audio strip bench needs the GPU")
    for n in (64, 900):
        line = bench(n, a.reps)
        print(json.dumps(line))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
