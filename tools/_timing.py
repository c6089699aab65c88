"""The timing method of the bench tools: short calls in windows between two HIP events, the candidates taking turns; host-side calls by the
host clock between device synchronisations.  Every tool keeps its own window length, repetitions, field names and output file."""
import time

import numpy as np
import torch


def gpu_ms_alternating(fns, reps, inner, warmup=3):
    """per function the median and the minimum time of one call in ms: ``reps`` windows of ``inner`` back-to-back calls each, timed by HIP
    events, the functions taking turns window by window (after ``warmup`` untimed calls of each).  One call is tens of microseconds: a
    window of one measures the event pair."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, out in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) / inner)
    return [(float(np.median(t)), float(np.min(t))) for t in times]


def host_ms(fn, reps):
    """the median and the minimum host time in ms of ``max(reps, 5)`` calls of a function that waits for the device itself (after one
    untimed call)"""
    fn()
    times = []
    for _ in range(max(reps, 5)):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times)), float(np.min(times))
