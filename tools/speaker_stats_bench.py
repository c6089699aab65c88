#!/usr/bin/env python
"""Speaker statistics throughput (speaker_stats.compute_speaker_stats, csrc/speaker_stats.hip): writes a synthetic speaker of N clips
(tests/golden/synth_speaker_stats.py, float64, full-size audio) to a temporary directory, then times the whole computation with the
decoded clips resident on the device and with pass 2 re-reading the files.  One JSON line per run: kernel time per pass (HIP events
around the accumulate launches), end-to-end seconds and clips/s, and the share of the host's npz decoding.

    python tools/speaker_stats_bench.py [--clips 2000] [--chunks 10] [--out profiles/r07_speaker_stats_bench.jsonl]
"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=2000)
    ap.add_argument("--chunks", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import synth_speaker_stats as S
    from speechdrivestemplates_amd.speaker_stats import compute_speaker_stats
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        S.write_stats_speaker(tmp, "bench", n_train=a.clips, seed=1, dev_every=0)
        write_s = time.perf_counter() - t0
        compute_speaker_stats(tmp, "bench", num_chunks=a.chunks, scale_factor=1.0)  # warm-up: library, allocator, page cache
        for path, budget in (("resident", 8 << 30), ("reread", 0)):
            for r in range(a.repeats):
                st = compute_speaker_stats(tmp, "bench", num_chunks=a.chunks, scale_factor=1.0, device_budget_bytes=budget)
                t = st["timing"]
                n = st["clips_used"]
                lines.append({"tool": "speaker_stats_bench", "path": path, "repeat": r, "clips": n, "chunks": a.chunks, "frames": 64,
                              "dtype": st["dtype"], "kernel_ms_pass1": round(t["kernel_ms"][0], 4), "kernel_ms_pass2": round(t["kernel_ms"][1], 4),
                              "kernel_us_per_1k_clips_per_pass": round(1e3 * sum(t["kernel_ms"]) / 2 / (n / 1e3), 2),
                              "total_s": round(t["total_s"], 4), "read_s": round(t["read_s"], 4),
                              "read_share": round(t["read_s"] / t["total_s"], 3), "clips_per_s": round(n / t["total_s"], 1),
                              "write_fixture_s": round(write_s, 2), "device": torch.cuda.get_device_name(0)})
                print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
