"""Time the motion histograms (csrc/motion_dist.hip) by HIP events, each beside the clip metrics timed in the same
process at the same shapes (the yardstick, not this code).  JSON lines:
    add      one MotionDistAccumulator.add at R = 32, T = 64, K = 121 with m = 1 and with m = 4 (two launches each): median and minimum of
             --reps windows of 20 back-to-back calls, alternating window by window with ClipMetricsAccumulator.add (three launches, four
             with copies) on the same tensors, and their ratio; plus the bytes the add reads and writes, from the shapes
    result   one result() at N = 4096 clips, all seen (two launches and the device-to-host copy of the 64 words; host clock around the
             call, which ends in that copy), beside ClipMetricsAccumulator.result() at the same N
Appends to profiles/r27_motion_dist_bench.jsonl.

    python tools/motion_dist_bench.py [--reps 20] [--out profiles/r27_motion_dist_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from speechdrivestemplates_amd import clip_metrics as cm  # noqa: E402
from speechdrivestemplates_amd import motion_dist as md  # noqa: E402
from tools._timing import gpu_ms_alternating, host_ms  # noqa: E402

INNER = 20  # calls between two events: one call is tens of microseconds, a window of one measures the event pair
R, T, K, N_RESULT = 32, 64, 121, 4096


def add_bytes(m):
    """bytes one add moves, from the shapes: both pose tensors read once, the row records written and read, the clip records written"""
    return 2 * R * T * 2 * K * 8 + 2 * R * md.COLS * 8 + (R // m) * md.COLS * 8


def bench_add(reps):
    rng = np.random.Generator(np.random.PCG64(3))
    gt = 200.0 + np.cumsum(rng.standard_normal((R, T, 2, K)) * 3.0, axis=1)
    pred = gt + rng.standard_normal((R, T, 2, K)) * 2.0
    p64, g64 = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    lines = []
    for m in (1, 4):
        acc = md.MotionDistAccumulator(R // m, K, None, "cuda")
        ref = cm.ClipMetricsAccumulator(R // m, K, [0.1, 0.2], "cuda")
        idx = torch.arange(R // m, dtype=torch.int64, device="cuda")
        (ms, mn), (cms, cmn) = gpu_ms_alternating([lambda: acc.add(p64, g64, idx, m), lambda: ref.add(p64, g64, idx, m)], reps, INNER)
        lines.append({"tool": "motion_dist_bench", "case": "add", "device": torch.cuda.get_device_name(0), "reps": reps, "R": R, "T": T, "K": K,
                      "copies": m, "launches": 2, "add_ms": ms, "add_min_ms": mn, "clip_metrics_add_ms": cms, "clip_metrics_add_min_ms": cmn,
                      "add_over_clip_metrics_add": ms / cms, "bytes_moved": add_bytes(m), "gb_per_s": add_bytes(m) / ms / 1e6})
    return lines


def bench_result(reps):
    parts = [k % 3 for k in range(5)]
    rng = np.random.Generator(np.random.PCG64(4))
    gt = 200.0 + np.cumsum(rng.standard_normal((N_RESULT, 5, 2, 5)) * 3.0, axis=1)
    p, g = torch.from_numpy(gt + rng.standard_normal(gt.shape)).cuda(), torch.from_numpy(gt).cuda()
    idx = torch.arange(N_RESULT, dtype=torch.int64)
    acc = md.MotionDistAccumulator(N_RESULT, 5, None, "cuda", parts=parts)
    ref = cm.ClipMetricsAccumulator(N_RESULT, 5, [0.1, 0.2], "cuda", parts=parts)
    acc.add(p, g, idx, 1)
    ref.add(p, g, idx, 1)
    assert acc.result()["motion_clips_seen"] == N_RESULT and ref.result()["clips_seen"] == N_RESULT
    ms, mn = host_ms(acc.result, reps)
    cms, cmn = host_ms(ref.result, reps)
    return {"tool": "motion_dist_bench", "case": "result", "device": torch.cuda.get_device_name(0), "reps": max(reps, 5), "N": N_RESULT,
            "result_ms": ms, "result_min_ms": mn, "clip_metrics_result_ms": cms, "clip_metrics_result_min_ms": cmn,
            "result_over_clip_metrics_result": ms / cms, "table_bytes": N_RESULT * md.COLS * 8}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r27_motion_dist_bench.jsonl"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the bench needs the GPU"
    lines = bench_add(a.reps) + [bench_result(a.reps)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            text = json.dumps(line)
            f.write(text + "\n")
            print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
