"""Time the whole-recording demo (csrc/long_demo.hip) by HIP events.  JSON lines:
    kernels   ld.stitch, ld.smooth [2, 2], ld.report (with smoothed poses) and the three in a row at F = 4500, K = 121, W = 64, O = 16
              (N = 94 windows): median and minimum of --reps windows of 10 back-to-back calls, the four taking turns window by window.  Each call
              includes its output allocation from torch's caching allocator; report also uploads the 121-byte part table.
    gather    ld.gather_windows of 32 windows of 68266 samples out of the 4.8 M samples of that recording
    run       LongDemo.generate (gather + the forward passes in groups of DEMO.LONG_BATCH = 32 + final poses) and the whole LongDemo.run (that,
              then stitch + smooth + report and the report's copy to the host) of voice2pose_sdt_bp on a synthetic recording of 4500 frames:
              events around each, alternating, after one untimed call of each
Appends to profiles/r19_long_demo_bench.jsonl.

    python tools/long_demo_bench.py [--reps 20] [--out profiles/r19_long_demo_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from speechdrivestemplates_amd import long_demo as ld  # noqa: E402
from tools._timing import gpu_ms_alternating  # noqa: E402

INNER = 10
F, W, O, K, SMOOTH, BATCH = 4500, 64, 16, 121, (2, 2), 32


def bench_kernels(reps):
    rng = np.random.Generator(np.random.PCG64(3))
    starts, offsets = ld.window_layout(F, W, O)
    N = len(starts)
    base = rng.uniform(0.0, 400.0, (F, 2, K))
    win = torch.from_numpy(np.stack([base[s:s + W] + rng.standard_normal((W, 2, K)) for s in starts])).cuda()
    stitched = ld.stitch(win, O, F)
    smoothed = ld.smooth(stitched, SMOOTH)

    def all_three():
        s = ld.stitch(win, O, F)
        y = ld.smooth(s, SMOOTH)
        return ld.report(win, s, y, O)

    names = ("stitch", "smooth", "report", "stitch_smooth_report")
    res = gpu_ms_alternating([lambda: ld.stitch(win, O, F), lambda: ld.smooth(stitched, SMOOTH), lambda: ld.report(win, stitched, smoothed, O),
                              all_three], reps, INNER)
    pose_bytes = F * 2 * K * 8
    moved = {"stitch": N * W * 2 * K * 8 + pose_bytes, "smooth": 2 * pose_bytes}  # (report re-reads neighbouring frames: not stated)
    line = {"tool": "long_demo_bench", "case": "kernels", "device": torch.cuda.get_device_name(0), "reps": reps, "inner": INNER, "F": F, "W": W,
            "O": O, "K": K, "N": N, "smooth": list(SMOOTH)}
    for name, (ms, mn) in zip(names, res):
        line[name + "_ms"], line[name + "_min_ms"] = ms, mn
        if name in moved:
            line[name + "_bytes"] = moved[name]
    audio = torch.from_numpy(rng.standard_normal(F * 16000 // 15).astype(np.float32)).cuda()
    offs = torch.tensor(offsets[:BATCH], dtype=torch.int64, device="cuda")
    (g_ms, g_min), = gpu_ms_alternating([lambda: ld.gather_windows(audio, offs, 68266)], reps, INNER)
    gather = {"tool": "long_demo_bench", "case": "gather", "device": torch.cuda.get_device_name(0), "reps": reps, "inner": INNER, "windows": BATCH,
              "Lw": 68266, "L": int(audio.numel()), "gather_ms": g_ms, "gather_min_ms": g_min, "gather_bytes": 2 * BATCH * 68266 * 4}
    return [line, gather]


def bench_run(reps):
    from __graft_entry__ import make_pipeline
    from speechdrivestemplates_amd.core.datasets import gesture_dataset as gd
    pipe, cfg = make_pipeline("voice2pose_sdt_bp", 16)
    cfg.defrost()
    cfg.DEMO.LONG_FORM, cfg.DEMO.WINDOW_OVERLAP, cfg.DEMO.LONG_BATCH, cfg.DEMO.SMOOTH, cfg.DEMO.CODE_INDEX = True, O, BATCH, list(SMOOTH), 3
    cfg.freeze()
    pipe.test_dataset = gd.SyntheticGestureDataset(cfg=cfg, num_clips=16, split="val")
    pipe.model.eval()
    rng = np.random.Generator(np.random.PCG64(21))
    L = int(F * 16000 / 15)
    stat = {"scale_factor": torch.tensor([1.1]), "mean": torch.from_numpy(rng.standard_normal((1, 242)) * 20.0 + 300.0),
            "std": torch.from_numpy(rng.uniform(2.0, 30.0, (1, 242)))}
    batch = {"audio": torch.from_numpy((0.1 * rng.standard_normal((1, L))).astype(np.float32)), "speaker": ["synthetic"],
             "clip_index": torch.tensor([0]), "num_frames": torch.tensor([F]), "speaker_stat": stat}
    runner = ld.LongDemo(pipe)
    out = {}

    def run():
        out["res"] = runner.run(batch)

    with torch.no_grad():
        pipe.apply_knobs()
        (gen, gen_min), (whole, whole_min) = gpu_ms_alternating([lambda: runner.generate(batch), run], max(3, reps // 4), 1, warmup=1)
    res = out["res"]
    assert res["poses_pred_batch"].shape == (1, F, 2, K) and bool(torch.isfinite(res["poses_pred_batch"]).all())
    pipe.close()
    return {"tool": "long_demo_bench", "case": "run", "device": torch.cuda.get_device_name(0), "reps": max(3, reps // 4), "F": F, "W": W, "O": O,
            "N": int(res["poses_windows"].shape[0]), "long_batch": BATCH, "forward_passes": -(-int(res["poses_windows"].shape[0]) // BATCH),
            "smooth": list(SMOOTH), "generate_ms": gen, "generate_min_ms": gen_min, "run_ms": whole, "run_min_ms": whole_min,
            "run_minus_generate_ms": whole - gen, "report": ld.report_values(res["long_report"].numpy())}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r19_long_demo_bench.jsonl"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the bench needs the GPU"
    lines = bench_kernels(a.reps) + [bench_run(a.reps)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            text = json.dumps(line)
            f.write(text + "\n")
            print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
