"""Time the per-clip validation metrics (csrc/clip_metrics.hip) by HIP events and around one validate().  JSON lines:
    add           one ClipMetricsAccumulator.add at R = 32, T = 64, K = 121 with m = 1 (three launches) and with m = 4 (four): median and
                  minimum of --reps windows of 20 back-to-back calls, alternating window by window with
    final_metrics ops.final_metrics (sdt_final_metrics_f64) on fp32 poses of the same shape -- the sibling that makes the same pass, one
                  workgroup per (row, frame) and a reduction kernel -- and their ratio; plus the bytes the add reads and writes, from the shapes
    result        one result() at N = 4096 clips, all seen (two launches and the one device-to-host copy of 320 bytes; host clock around the
                  call, which ends in that copy)
    validate      one validate() of voice2pose_sdt_bp over 256 synthetic clips in batches of 32 with TEST.CLIP_METRICS off and on (host clock,
                  the loop ends in host reads of the metrics), for TEST.MULTIPLE 1 and 4, alternating
Appends to profiles/r18_clip_metrics_bench.jsonl.

    python tools/clip_metrics_bench.py [--reps 20] [--out profiles/r18_clip_metrics_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from speechdrivestemplates_amd import clip_metrics as cm  # noqa: E402
from speechdrivestemplates_amd import ops  # noqa: E402
from tools._timing import gpu_ms_alternating, host_ms  # noqa: E402

INNER = 20  # calls between two events: one call is tens of microseconds, a window of one measures the event pair
R, T, K, N_RESULT, N_VAL = 32, 64, 121, 4096, 256


def add_bytes(m):
    """bytes one add moves, from the shapes: the poses read once (the next frame's re-read and the copies' re-read by the diversity kernel
    counted), the per-frame partials written and read, the row records written and read, the clip records written"""
    poses = R * T * 2 * K * 8
    rows = 2 * 2 * poses + 2 * R * T * 32 * 8 + 2 * R * cm.COLS * 8
    div = poses + 2 * (R // m) * T * 4 * 8 if m > 1 else 0
    return rows + div + (R // m) * cm.COLS * 8


def bench_add(reps):
    rng = np.random.Generator(np.random.PCG64(3))
    gt = rng.uniform(0.0, 400.0, (R, T, 2, K))
    pred = gt + rng.standard_normal((R, T, 2, K)) * 20.0
    p64, g64 = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    p32, g32 = p64.float(), g64.float()
    mean, std, scale = (torch.zeros((R, 2 * K), dtype=torch.float64, device="cuda"), torch.ones((R, 2 * K), dtype=torch.float64, device="cuda"),
                        torch.ones(R, dtype=torch.float64, device="cuda"))
    accs = {m: cm.ClipMetricsAccumulator(R // m, K, [0.1, 0.2], "cuda") for m in (1, 4)}
    idx = {m: torch.arange(R // m, dtype=torch.int64, device="cuda") for m in (1, 4)}
    (a1, a1_min), (a4, a4_min), (fm, fm_min) = gpu_ms_alternating(
        [lambda: accs[1].add(p64, g64, idx[1], 1), lambda: accs[4].add(p64, g64, idx[4], 4),
         lambda: ops.final_metrics(p32, g32, mean, std, scale, False, True)], reps, INNER)
    return [{"tool": "clip_metrics_bench", "case": "add", "device": torch.cuda.get_device_name(0), "reps": reps, "R": R, "T": T, "K": K, "copies": m,
             "launches": 3 if m == 1 else 4, "add_ms": ms, "add_min_ms": mn, "final_metrics_ms": fm, "final_metrics_min_ms": fm_min,
             "add_over_final_metrics": ms / fm, "bytes_moved": add_bytes(m), "gb_per_s": add_bytes(m) / ms / 1e6}
            for m, ms, mn in ((1, a1, a1_min), (4, a4, a4_min))]


def bench_result(reps):
    acc = cm.ClipMetricsAccumulator(N_RESULT, 5, [0.1, 0.2], "cuda", parts=[k % 3 for k in range(5)])
    rng = np.random.Generator(np.random.PCG64(4))
    gt = rng.uniform(0.0, 400.0, (N_RESULT, 3, 2, 5))
    acc.add(torch.from_numpy(gt + rng.standard_normal(gt.shape)).cuda(), torch.from_numpy(gt).cuda(), torch.arange(N_RESULT, dtype=torch.int64), 1)
    ms, mn = host_ms(acc.result, reps)
    assert acc.result()["clips_seen"] == N_RESULT
    return {"tool": "clip_metrics_bench", "case": "result", "device": torch.cuda.get_device_name(0), "reps": max(reps, 5), "N": N_RESULT,
            "result_ms": ms, "result_min_ms": mn}


def bench_validate(reps):
    from __graft_entry__ import make_pipeline
    from speechdrivestemplates_amd.core.datasets import gesture_dataset as gd
    pipe, cfg = make_pipeline("voice2pose_sdt_bp", 16)
    ds = gd.SyntheticGestureDataset(cfg=cfg, num_clips=N_VAL, split="val")
    pipe.test_dataset = ds
    pipe.test_dataloader = torch.utils.data.DataLoader(ds, batch_size=cfg.TEST.BATCH_SIZE, shuffle=False)
    pipe.num_test_samples, pipe.num_test_batches = len(ds), len(pipe.test_dataloader)

    def run(on, m):
        cfg.defrost()
        cfg.TEST.CLIP_METRICS, cfg.TEST.MULTIPLE = on, m
        cfg.freeze()
        torch.manual_seed(5)
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = pipe.validate(pipe.test_dataloader, 1)
        vals = {k: float(v) for k, v in out.items()}  # (host reads: the loop's work has ended)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, vals

    lines = []
    for m in (1, 4):
        run(False, m), run(True, m)  # warm both
        off, on, vals = [], [], None
        for _ in range(max(3, reps // 4)):
            off.append(run(False, m)[0])
            ms, vals = run(True, m)
            on.append(ms)
        lines.append({"tool": "clip_metrics_bench", "case": "validate", "device": torch.cuda.get_device_name(0), "reps": len(on), "clips": N_VAL,
                      "batch": cfg.TEST.BATCH_SIZE, "copies": m, "validate_off_ms": float(np.median(off)), "validate_on_ms": float(np.median(on)),
                      "validate_off_min_ms": float(np.min(off)), "validate_on_min_ms": float(np.min(on)),
                      "on_over_off": float(np.median(on) / np.median(off)), "values": {k: v for k, v in vals.items() if not k.startswith("G_")}})
    cfg.defrost()
    cfg.TEST.CLIP_METRICS, cfg.TEST.MULTIPLE = False, 1
    cfg.freeze()
    pipe.close()
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r18_clip_metrics_bench.jsonl"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the bench needs the GPU"
    lines = bench_add(a.reps) + [bench_result(a.reps)] + bench_validate(a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            text = json.dumps(line)
            f.write(text + "\n")
            print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
