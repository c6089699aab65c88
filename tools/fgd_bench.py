#!/usr/bin/env python
"""Device-FGD timing (csrc/fgd.hip, SYS.DEVICE_FGD).  Not bench.py: this measures the opt-in validation metric only.

Kernels: HIP-event times of ``sdt_fgd_accumulate`` for one validation step (32 rows of mu ++ logvar, 32 + 32 columns) and of
``sdt_fgd_finalize`` on the 64-wide state for dim_used 32 (FGD_mu) and 64 (FGD_mu_logvar), after a warm-up, over enough back-to-back
calls to fill ``--seconds``, repeated ``--repeats`` times: min and median of the per-call means.
Loop: wall time of ``Trainer.validate`` (voice2pose_sdt_bp, ``--clips`` synthetic validation clips in batches of 32, the batches built
once and reused so that the dataset's own cost stays out of it) with the key off and on, in turn, one warm-up call then ``--repeats`` timed
ones each: min and median, and the two metrics of both routes.  ``--keys off`` measures the key-off loop alone (the form to run on
another commit for comparison).  One JSON line per measurement, appended to --out.

    python tools/fgd_bench.py [--seconds 0.2] [--repeats 5] [--clips 1024] [--keys off on] [--out profiles/r09_fgd_bench.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, seconds):
    """mean HIP-event us of fn() over enough back-to-back calls to fill ``seconds`` (3 warm-up calls first)"""
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        fn()
    e1.record()
    e1.synchronize()
    reps = max(10, min(20000, int(seconds * 1e3 / max(e0.elapsed_time(e1) / 5, 1e-3))))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, reps


def kernels(seconds, repeats):
    from speechdrivestemplates_amd import _lib, fgd
    lib = _lib.load()
    rng = np.random.Generator(np.random.PCG64(0))
    feats = [torch.from_numpy(rng.standard_normal((32, 32)).astype(np.float32)).cuda() for _ in range(4)]
    acc = fgd.FGDAccumulator(64, "cuda")
    for _ in range(32):  # a 1024-clip epoch's worth of rows, so that finalize sees full-rank covariances
        acc.add(*[torch.from_numpy(rng.standard_normal((32, 32)).astype(np.float32)).cuda() for _ in range(4)])
    raw = torch.cuda.current_stream().cuda_stream
    scratch = fgd.FGDAccumulator(64, "cuda")
    st = scratch.state_tensors()[0]

    def accumulate():
        _lib.check(lib.sdt_fgd_accumulate(C.c_void_p(feats[0].data_ptr()), 32, C.c_void_p(feats[1].data_ptr()), 32, 32,
                                          C.c_void_p(st.data_ptr()), scratch.state_bytes, 0, raw))

    out, err = torch.empty(16, dtype=torch.float64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    a, b = (C.c_void_p * 1)(acc.state_tensors()[0].data_ptr()), (C.c_void_p * 1)(acc.state_tensors()[1].data_ptr())

    def finalize(dim_used):
        _lib.check(lib.sdt_fgd_finalize(a, b, 1, 64, dim_used, fgd.MAX_SWEEPS, fgd.REL_TOL, C.c_void_p(out.data_ptr()), C.c_void_p(err.data_ptr()),
                                        raw))

    recs = []
    for name, fn in (("accumulate_32x64", accumulate), ("finalize_dim32_of_64", lambda: finalize(32)), ("finalize_dim64", lambda: finalize(64))):
        us = [timed(fn, seconds) for _ in range(repeats)]
        rec = {"tool": "fgd_bench", "kernel": name, "us_min": round(min(u for u, _ in us), 2),
               "us_median": round(statistics.median(u for u, _ in us), 2), "calls_per_repeat": us[0][1], "repeats": repeats}
        if name.startswith("finalize"):
            assert int(err.item()) == 0
            rec.update(sweeps=[int(out[7].item()), int(out[9].item())])
        recs.append(rec)
    return recs


def loop(key_on, clips, repeats):
    from __graft_entry__ import make_pipeline
    from speechdrivestemplates_amd.core.datasets import gesture_dataset as gd
    torch.manual_seed(0)
    pipe, cfg = make_pipeline("voice2pose_sdt_bp", 64, sys_opts={"DEVICE_FGD": True} if key_on else None)
    ds = gd.SyntheticGestureDataset(cfg=cfg, num_clips=clips, split="val")
    batches = list(torch.utils.data.DataLoader(ds, batch_size=32, shuffle=False))
    pipe.test_dataset, pipe.num_test_samples, pipe.num_test_batches = ds, clips, len(batches)
    times, out = [], None
    for i in range(repeats + 1):
        torch.manual_seed(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe.validate(batches, 1)
        torch.cuda.synchronize()
        if i:
            times.append(time.perf_counter() - t0)
    return {"tool": "fgd_bench", "loop": "validate", "config": "voice2pose_sdt_bp", "DEVICE_FGD": bool(key_on), "clips": clips, "batch": 32,
            "wall_ms_min": round(min(times) * 1e3, 2), "wall_ms_median": round(statistics.median(times) * 1e3, 2), "repeats": repeats,
            "FGD_mu": float(out["FGD_mu"]), "FGD_mu_logvar": float(out["FGD_mu_logvar"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.2, help="timed window per kernel and repeat")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--keys", nargs="+", choices=("off", "on"), default=("off", "on"))
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r09_fgd_bench.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fgd_bench needs the GPU"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        def emit(rec):
            rec["device"] = torch.cuda.get_device_name(0)
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
        if not a.no_kernels:
            for rec in kernels(a.seconds, a.repeats):
                emit(rec)
        for key in a.keys:
            emit(loop(key == "on", a.clips, a.repeats))


if __name__ == "__main__":
    main()
