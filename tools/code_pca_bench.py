#!/usr/bin/env python
"""Clip-code figure timing (csrc/code_pca.hip).  Not bench.py: this measures the opt-in per-epoch figure only.

For N = 4096, 30000 and 100000 rows of D = 32 (and 512 rows of D = 64, the largest eigenproblem): HIP-event times of the four stages
(moments, eigh, project, raster; the ABI calls of code_pca.fit_project / render_scatter, buffers allocated once) after a warm-up,
averaged over enough repeats to fill ``--seconds`` per stage; the wall time of the whole ``clip_code_figure`` call (allocations, the
host's reads of the error words and limits) and of ``save_png``; the table bytes over the stage time for the two stages that read the
table.  Where scikit-learn and matplotlib import, also the wall time of the reference's host route on the same table (device -> host
copy, PCA.fit + transform, Agg scatter to a PNG), for comparison.  One JSON line per size, appended to --out.

    python tools/code_pca_bench.py [--seconds 0.3] [--out profiles/r08_code_pca_bench.jsonl]
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechdrivestemplates_amd import _lib, code_pca  # noqa: E402

SIZES = ((4096, 32), (30000, 32), (100000, 32), (512, 64))


def table(n, d, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((n, d)) * np.linspace(2.0, 0.2, d)
    return torch.from_numpy((x @ (np.eye(d) + 0.1 * rng.standard_normal((d, d)))).astype(np.float32)).cuda()


def timed(fn, seconds):
    """mean HIP-event ms of fn() over enough back-to-back calls to fill ``seconds`` (3 warm-up calls first)"""
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
    return e0.elapsed_time(e1) / reps, reps


def stages(x, seconds, canvas, marker_px):
    lib = _lib.load()
    p = code_pca._p
    n, d = x.shape
    dev = x.device
    raw = torch.cuda.current_stream(dev).cuda_stream
    f64 = dict(dtype=torch.float64, device=dev)
    ws_bytes = lib.sdt_code_pca_workspace_bytes(n, d)
    ws, mean, cov = torch.empty(ws_bytes // 8, **f64), torch.empty(d, **f64), torch.empty((d, d), **f64)
    bad, err = torch.empty(1, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    evals, comps, info = torch.empty(d, **f64), torch.empty((2, d), **f64), torch.empty(4, **f64)
    X, limits = torch.empty((n, 2), **f64), torch.empty(8, **f64)
    h, w = canvas
    ph, pw = code_pca.plot_rectangle(canvas)
    tab = code_pca.colour_table()
    tab_d = torch.from_numpy(tab).to(dev)
    counts, out = torch.zeros((ph, pw), dtype=torch.int32, device=dev), torch.empty((h, w, 3), dtype=torch.uint8, device=dev)

    def moments():
        _lib.check(lib.sdt_code_pca_moments(p(x), n, d, p(ws), ws_bytes, p(mean), p(cov), p(bad), raw))

    def eigh():
        _lib.check(lib.sdt_code_pca_eigh(p(cov), d, code_pca.MAX_SWEEPS, code_pca.REL_TOL, p(evals), p(comps), p(info), p(err), raw))

    def project():
        _lib.check(lib.sdt_code_pca_project(p(x), n, d, p(mean), p(comps), p(X), p(ws), ws_bytes, p(limits), raw))

    def raster():  # with the caller's zeroing of the counters, as render_scatter does it
        counts.zero_()
        _lib.check(lib.sdt_code_pca_raster(p(X), n, C.c_void_p(limits.data_ptr() + 32), p(tab_d), tab.shape[0], h, w, code_pca.MARGIN_PX,
                                           marker_px, p(counts), counts.numel(), p(out), out.numel(), raw))

    res = {}
    for name, fn in (("moments", moments), ("eigh", eigh), ("project", project), ("raster", raster)):
        ms, reps = timed(fn, seconds)
        res[name + "_us"] = round(ms * 1e3, 2)
        res[name + "_reps"] = reps
    assert int(err.item()) == 0 and int(bad.item()) == 0
    res["sweeps"] = int(info[0].item())
    table_bytes = n * d * 4
    res["moments_table_GBps"] = round(2 * table_bytes / (res["moments_us"] * 1e-6) / 1e9, 1)  # two passes over the table
    res["project_table_GBps"] = round(table_bytes / (res["project_us"] * 1e-6) / 1e9, 1)
    return res


def whole_call(x, canvas, marker_px, repeats=5):
    code_pca.clip_code_figure(x, canvas=canvas, marker_px=marker_px)
    torch.cuda.synchronize()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        img = code_pca.clip_code_figure(x, canvas=canvas, marker_px=marker_px)
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        code_pca.save_png(os.path.join(d, "f.png"), img, {"n": 1})
        png = time.perf_counter() - t0
    return {"figure_wall_ms_median": round(sorted(t)[len(t) // 2] * 1e3, 3), "figure_wall_ms_min": round(min(t) * 1e3, 3),
            "save_png_ms": round(png * 1e3, 2)}


def host_route(x, repeats=3):
    """the reference's draw_figure_epoch (core/pipelines/voice2pose.py:479-510) on the same table, figure written to a PNG in memory"""
    try:
        import matplotlib as mpl
        mpl.use("Agg")
        import matplotlib.pyplot as plt
        from sklearn import decomposition
    except ImportError as e:
        return {"host_route": "not measured (%s)" % e}
    t = []
    for _ in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        code = x.detach().cpu().numpy()
        fig = plt.figure()
        pca = decomposition.PCA(n_components=2)
        pca.fit(code)
        X = pca.transform(code)
        plt.scatter(X[:, 0], X[:, 1], alpha=0.2, edgecolors="none", s=1)
        fig.tight_layout()
        fig.savefig(io.BytesIO(), format="png")
        plt.close()
        t.append(time.perf_counter() - t0)
    t = t[1:]  # the first call imports and builds font caches
    return {"host_route_wall_ms_median": round(sorted(t)[len(t) // 2] * 1e3, 2), "host_route_wall_ms_min": round(min(t) * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3, help="timed window per stage")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r08_code_pca_bench.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "code_pca_bench needs the GPU"
    canvas, marker_px = code_pca.DEFAULT_CANVAS, 2
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for n, d in SIZES:
            x = table(n, d)
            rec = {"tool": "code_pca_bench", "rows": n, "dim": d, "canvas": list(canvas), "marker_px": marker_px}
            rec.update(stages(x, a.seconds, canvas, marker_px))
            rec.update(whole_call(x, canvas, marker_px))
            rec.update(host_route(x))
            rec["device"] = torch.cuda.get_device_name(0)
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
