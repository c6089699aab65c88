"""Time the per-tensor histogram snapshot (csrc/tensor_hist.hip) by HIP events on two buffers: the flat parameter
buffer of the voice2pose_sdt_bp generator (optimizerG: 7.08 M elements, its real segment table and its initial weights) and a
100 000 x 32 clip-code table (one segment, normal with std 0.5).  Per buffer one JSON line with
    snapshot_ms   one tensor_hist.flat_histograms call (two memsets, the segmented pass, the per-segment reduction; with its allocations);
                  median of --reps windows of 20 back-to-back calls, alternating with the windows of
    sumsq_ms      sdt_grad_sumsq_f64 on the same buffer: the sibling that makes the same single read pass and the same float64 tree
    host_ms       the route through the host: device-to-host copy of the buffer, then per tensor np.histogram over the 1549 edges, sum and
                  sum of squares in float64 (wall clock, once)
and the ratios snapshot / sumsq and host / snapshot.  Appends to profiles/r16_tensor_hist_bench.jsonl.

    python tools/tensor_hist_bench.py [--reps 20] [--skip-host] [--out profiles/r16_tensor_hist_bench.jsonl]
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

from speechdrivestemplates_amd import ops  # noqa: E402
from speechdrivestemplates_amd import tensor_hist as th  # noqa: E402
from tools._timing import gpu_ms_alternating  # noqa: E402


INNER = 20  # calls between two events: one call is tens of microseconds, a window of one measures the event pair


def host_route(flat, offsets, sizes):
    t = time.perf_counter()
    x = flat.cpu().numpy()
    out = []
    for off, n in zip(offsets, sizes):
        v = x[off:off + n].astype(np.float64)
        out.append((np.histogram(np.clip(v, th.BUCKET_EDGES[0], th.BUCKET_EDGES[-1]), bins=th.BUCKET_EDGES)[0], v.sum(), (v * v).sum()))
    return (time.perf_counter() - t) * 1e3, out


def bench(name, flat, offsets, sizes, reps, host):
    partial = torch.zeros(ops.grad_sumsq_partials(), device=flat.device, dtype=torch.float64)
    (snap, snap_min), (sumsq, sumsq_min) = gpu_ms_alternating([lambda: th.flat_histograms(flat, offsets, sizes),
                                                               lambda: ops.grad_sumsq(flat, partial)], reps, INNER)
    counts, tallies, stats = (t.cpu().numpy() for t in th.flat_histograms(flat, offsets, sizes))
    line = {"tool": "tensor_hist_bench", "case": name, "device": torch.cuda.get_device_name(0), "reps": reps, "elements": int(sum(sizes)),
            "segments": len(sizes), "chunks": int(sum(-(-n // th.HIST_CHUNK) for n in sizes)), "buffer_mb": flat.numel() * 4 / 1e6,
            "result_kb": (counts.nbytes + tallies.nbytes + stats.nbytes) / 1e3, "occupied_buckets_max": int((counts > 0).sum(1).max()),
            "snapshot_ms": snap, "snapshot_min_ms": snap_min, "sumsq_ms": sumsq, "sumsq_min_ms": sumsq_min,
            "snapshot_over_sumsq": snap / sumsq, "snapshot_gb_per_s": flat.numel() * 4 / snap / 1e6}
    if host:
        ms, ref = host_route(flat, offsets, sizes)
        line["host_ms"], line["host_over_snapshot"] = ms, ms / snap
        line["counts_equal_host"] = bool(all(np.array_equal(counts[i], ref[i][0]) for i in range(len(sizes))))
    return line


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r16_tensor_hist_bench.jsonl"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the bench needs the GPU"
    from __graft_entry__ import make_pipeline
    pipe, _ = make_pipeline("voice2pose_sdt_bp", 16)
    opt = pipe.optimizers["optimizerG"]
    lines = [bench("sdt_bp_generator", opt.flat_param.detach(), list(opt.offsets), [p.numel() for p in opt.params], a.reps, not a.skip_host)]
    table = torch.from_numpy((np.random.Generator(np.random.PCG64(7)).standard_normal(100000 * 32) * 0.5).astype(np.float32)).cuda()
    lines.append(bench("code_table_100000x32", table, [0], [table.numel()], a.reps, not a.skip_host))
    pipe.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            text = json.dumps(line)
            f.write(text + "\n")
            print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
