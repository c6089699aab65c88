"""Time the stages of the template axes (csrc/code_axes.hip) by HIP events on two synthetic tables, 100 000 x 32 and
1 000 000 x 64, and the numpy contract models of code_axes.py on the host for the same tables.  Appends one JSON line to
profiles/r13_code_axes_bench.jsonl.  No speed claim rests on it; if one is made, it is against the host models of the same line.

    python tools/code_axes_bench.py [--reps 5] [--skip-host] [--out profiles/r13_code_axes_bench.jsonl]
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
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import synth_code_tables as S  # noqa: E402

from speechdrivestemplates_amd import _lib  # noqa: E402
from speechdrivestemplates_amd import code_axes as CA  # noqa: E402

TABLES = ((100000, 32), (1000000, 64))
AXES, STEPS = 4, 7


def gpu_ms(fn, reps):
    """median of ``reps`` HIP-event timings of fn() after one untimed call"""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def host_ms(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def bench_table(n, d, reps, host):
    lib = _lib.load()
    table = S.make_table((n, d), 50 + d)
    x = torch.from_numpy(table).cuda()
    p = CA._p
    raw = torch.cuda.current_stream().cuda_stream
    f64 = dict(dtype=torch.float64, device="cuda")
    ws_bytes = lib.sdt_code_pca_workspace_bytes(n, d)
    ws = torch.empty(ws_bytes // 8, **f64)
    mean, cov, bad = torch.empty(d, **f64), torch.empty((d, d), **f64), torch.empty(1, dtype=torch.int64, device="cuda")
    evals, comps, info = torch.empty(d, **f64), torch.empty((d, d), **f64), torch.empty(4, **f64)
    err = torch.empty(1, dtype=torch.int32, device="cuda")
    P = torch.empty((n, d), **f64)
    ranks = CA.quantile_ranks(CA.FILE_QUANTILES, n)
    ranks_d = torch.tensor(ranks, dtype=torch.int64, device="cuda")
    qws_bytes = lib.sdt_code_axes_quantiles_workspace_bytes(n, d, len(ranks))
    qws, qout = torch.empty(qws_bytes // 8, dtype=torch.int64, device="cuda"), torch.empty((d, len(ranks)), **f64)
    gpu = {}
    gpu["moments_ms"] = gpu_ms(lambda: _lib.check(lib.sdt_code_pca_moments(p(x), n, d, p(ws), ws_bytes, p(mean), p(cov), p(bad), raw)), reps)
    gpu["eigh_ms"] = gpu_ms(lambda: _lib.check(lib.sdt_code_axes_eigh(p(cov), d, CA.MAX_SWEEPS, CA.REL_TOL, p(evals), p(comps), p(info), p(err), raw)), reps)
    gpu["project_ms"] = gpu_ms(lambda: _lib.check(lib.sdt_code_axes_project(p(x), n, d, p(mean), p(comps), p(P), raw)), reps)
    gpu["quantiles_ms"] = gpu_ms(lambda: _lib.check(lib.sdt_code_axes_quantiles(p(P), n, d, p(ranks_d), len(ranks), p(qout), p(qws), qws_bytes, raw)), reps)
    fit = {"mean": mean, "components": comps, "projections": P, "dim": d}
    points = CA.traversal(fit, AXES, STEPS)["points"].reshape(-1, d).contiguous()
    nq = points.shape[0]
    nws_bytes = lib.sdt_code_axes_nearest_workspace_bytes(n, d, nq)
    nws = torch.empty(nws_bytes // 8, **f64)
    index, dist2 = torch.empty(nq, dtype=torch.int64, device="cuda"), torch.empty(nq, **f64)
    gpu["nearest_ms"] = gpu_ms(lambda: _lib.check(lib.sdt_code_axes_nearest(p(x), n, d, p(points), nq, p(index), p(dist2), p(bad), p(nws), nws_bytes, raw)), reps)
    out = {"rows": n, "dim": d, "queries": nq, "ranks": len(ranks), "sweeps": int(info[0].item()), "gpu": gpu}
    if host:
        m, c, Pn = mean.cpu().numpy(), comps.cpu().numpy(), P.cpu().numpy()
        h = {}
        h["components_ms"], (lam, mc, _, _) = host_ms(lambda: CA.model_components(cov.cpu().numpy()))
        h["project_ms"], mp = host_ms(lambda: CA.model_project(table, m, c))
        h["quantiles_ms"], mq = host_ms(lambda: CA.model_quantiles(Pn, ranks))
        h["nearest_ms"], (mi, md) = host_ms(lambda: CA.model_nearest(table, points.cpu().numpy()))
        out["host_models"] = h
        out["equal_bits"] = bool(np.array_equal(mc, c) and np.array_equal(mp, Pn) and (mq == qout.cpu().numpy()).all()
                                 and np.array_equal(mi, index.cpu().numpy()) and np.array_equal(md, dist2.cpu().numpy()))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r13_code_axes_bench.jsonl"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the bench needs the GPU"
    line = {"tool": "code_axes_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps,
            "tables": [bench_table(n, d, a.reps, not a.skip_host) for n, d in TABLES]}
    text = json.dumps(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
