"""Time the bootstrap over the clip-metrics table (csrc/bootstrap.hip) at n = 512 and n = 4096 live clips with R = 1000
replicates.  One JSON line per n:
    stages     dense / sums / values / intervals: HIP events around the launches of each stage inside one clip_metric_intervals call; 3 warm-up
               calls, then the median and minimum of --reps calls (dense includes the host's read of n, the one wait before the end)
    call       the whole clip_metric_intervals call by the host clock (it ends in the copies of every stage to the host)
    result     ClipMetricsAccumulator.result() on the same table, by the host clock (it ends in its one copy)
    model      bootstrap.intervals_model in numpy on the host, median of 3
Appends to profiles/r31_bootstrap_bench.jsonl.

    python tools/bootstrap_bench.py [--reps 20] [--out profiles/r31_bootstrap_bench.jsonl]
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

from speechdrivestemplates_amd import bootstrap as bs  # noqa: E402
from speechdrivestemplates_amd import clip_metrics as cm  # noqa: E402
from tools._timing import host_ms  # noqa: E402

R, LEVEL, SEED, K, T = 1000, 0.95, 0, 5, 3
STAGES = ("dense", "sums", "values", "intervals")


def bench(n, reps):
    parts = [k % 3 for k in range(K)]
    acc = cm.ClipMetricsAccumulator(n, K, [0.1, 0.2], "cuda", parts=parts)
    rng = np.random.Generator(np.random.PCG64(n))
    gt = rng.uniform(0.0, 400.0, (n, T, 2, K))
    acc.add(torch.from_numpy(gt + rng.standard_normal(gt.shape) * 20.0).cuda(), torch.from_numpy(gt).cuda(), torch.arange(n, dtype=torch.int64), 1)
    sizes, alphas, rank = cm.part_sizes(parts), acc.alphas, bs.rank_of(R, LEVEL)
    per_stage = []
    for i in range(3 + reps):
        events = []
        st = bs.device_stages(acc, None, sizes, len(alphas), R, rank, SEED, events=events)
        torch.cuda.synchronize()
        assert st["n"] == n and len(events) == 5
        if i >= 3:
            per_stage.append([events[j].elapsed_time(events[j + 1]) for j in range(4)])
    per_stage = np.array(per_stage)
    call_ms, call_min = host_ms(lambda: bs.clip_metric_intervals(acc, replicates=R, level=LEVEL, seed=SEED), reps)
    result_ms, result_min = host_ms(acc.result, reps)
    table = acc.table().cpu().numpy()
    model = []
    for _ in range(3):
        t = time.perf_counter()
        want = bs.intervals_model(table, sizes, alphas, R, LEVEL, SEED)
        model.append((time.perf_counter() - t) * 1e3)
    assert want == bs.clip_metric_intervals(acc, replicates=R, level=LEVEL, seed=SEED)
    line = {"tool": "bootstrap_bench", "device": torch.cuda.get_device_name(0), "reps": reps, "warmup": 3, "n": n, "replicates": R,
            "call_ms": call_ms, "call_min_ms": call_min, "result_ms": result_ms, "result_min_ms": result_min,
            "model_ms": float(np.median(model)), "model_over_call": float(np.median(model) / call_ms)}
    for j, name in enumerate(STAGES):
        line[name + "_ms"], line[name + "_min_ms"] = float(np.median(per_stage[:, j])), float(per_stage[:, j].min())
    return line


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r31_bootstrap_bench.jsonl"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the bench needs the GPU"
    assert a.reps >= 20, "at least 20 timed calls"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for n in (512, 4096):
            text = json.dumps(bench(n, a.reps))
            f.write(text + "\n")
            print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
