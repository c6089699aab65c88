"""Time the speech-gesture synchrony metrics (csrc/sync_metrics.hip) by HIP events.  JSON lines:
    add        one SyncAccumulator.add at R = 32, T = 64, K = 121, L = 68266 with m = 1 and with m = 4 (seven launches: envelope, onsets,
               speeds and beats-and-matching for the prediction and again for the ground truth, commit): median and minimum of --reps windows
               of 20 back-to-back calls, alternating window by window with ClipMetricsAccumulator.add at the same shape, and their ratio
    recording  the whole-recording call at F = 4500 frames, L = 4 800 000 samples (four launches and the copy of the record), alternating with
               long_demo.report over 71 windows of 64 frames of the same poses
Appends to profiles/r20_sync_metrics_bench.jsonl.

    python tools/sync_metrics_bench.py [--reps 20] [--out profiles/r20_sync_metrics_bench.jsonl]
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
from speechdrivestemplates_amd import long_demo as ld  # noqa: E402
from speechdrivestemplates_amd import sync_metrics as sm  # noqa: E402
from tools._timing import gpu_ms_alternating  # noqa: E402

INNER = 20  # calls between two events: one call is tens of microseconds, a window of one measures the event pair
R, T, K, L, F, L_LONG, W, O = 32, 64, 121, 68266, 4500, 4800000, 64, 0


def speech(n, rng):
    x = rng.standard_normal(n) * 0.01
    for start in range(500, n, 2900):
        x[start:start + 600] += rng.standard_normal(len(x[start:start + 600])) * 0.5
    return x.astype(np.float32)


def bench_add(reps):
    rng = np.random.Generator(np.random.PCG64(3))
    gt = 200.0 + np.cumsum(rng.standard_normal((R, T, 2, K)) * 3.0, axis=1)
    pred = gt + rng.standard_normal((R, T, 2, K)) * 20.0
    p64, g64 = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    audio = torch.from_numpy(np.stack([speech(L, rng) for _ in range(R)])).cuda()
    sync = {m: sm.SyncAccumulator(R // m, K, 30, 0.1, "cuda") for m in (1, 4)}
    clip = {m: cm.ClipMetricsAccumulator(R // m, K, [0.1, 0.2], "cuda") for m in (1, 4)}
    idx = {m: torch.arange(R // m, dtype=torch.int64, device="cuda") for m in (1, 4)}
    res = gpu_ms_alternating([lambda: sync[1].add(p64, g64, audio, idx[1], 1), lambda: sync[4].add(p64, g64, audio[:R // 4], idx[4], 4),
                              lambda: clip[1].add(p64, g64, idx[1], 1), lambda: clip[4].add(p64, g64, idx[4], 4)], reps, INNER)
    onsets = int(sync[1].table()[:, sm.ONSETS].sum())
    return [{"tool": "sync_metrics_bench", "case": "add", "device": torch.cuda.get_device_name(0), "reps": reps, "R": R, "T": T, "K": K, "L": L,
             "copies": m, "launches": 7, "onsets_in_the_batch": onsets if m == 1 else None, "add_ms": res[i][0], "add_min_ms": res[i][1],
             "clip_metrics_add_ms": res[2 + i][0], "clip_metrics_add_min_ms": res[2 + i][1], "sync_over_clip_metrics": res[i][0] / res[2 + i][0]}
            for i, m in enumerate((1, 4))]


def bench_recording(reps):
    rng = np.random.Generator(np.random.PCG64(4))
    x = torch.from_numpy(200.0 + np.cumsum(rng.standard_normal((F, 2, K)) * 3.0, axis=0)).cuda()
    audio = torch.from_numpy(speech(L_LONG, rng)).cuda()
    n_win = len(ld.window_layout(F, W, O)[0])
    windows = torch.zeros((n_win, W, 2, K), dtype=torch.float64, device="cuda")
    flat = windows.view(-1, 2, K)
    flat[:F] = x  # (the last window is moved back in the layout; the report's cost does not depend on the values)
    (rec, rec_min), (rep, rep_min) = gpu_ms_alternating([lambda: sm.recording_report(x, audio, 30, 0.1), lambda: ld.report(windows, x, None, O)],
                                                        reps, inner=5)
    row = sm.recording_report(x, audio, 30, 0.1).cpu().numpy()
    return {"tool": "sync_metrics_bench", "case": "recording", "device": torch.cuda.get_device_name(0), "reps": reps, "F": F, "L": L_LONG, "K": K,
            "onsets": int(row[sm.ROW_ONSETS]), "beats_all": int(row[4]), "recording_report_ms": rec, "recording_report_min_ms": rec_min,
            "long_report_ms": rep, "long_report_min_ms": rep_min, "sync_over_long_report": rec / rep,
            "note": "both calls allocate their workspace and outputs; the sync call also builds its constant tables on the device"}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r20_sync_metrics_bench.jsonl"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the bench needs the GPU"
    lines = bench_add(a.reps) + [bench_recording(a.reps)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            text = json.dumps(line)
            f.write(text + "\n")
            print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
