"""Time the feature-set metrics (csrc/prdc.hip), each beside the device FGD timed in the same process on the same rows
(the yardstick, not this code) and beside the host route a user would otherwise take.  JSON lines:
    add      one FeatureSetAccumulator.add of 32 rows of 32 + 32 columns with m = 1 and m = 4 (one launch): median and minimum of --reps
             windows of 20 back-to-back calls by HIP events, alternating window by window with FGDAccumulator.add (two launches)
    result   one result() at N = 512, 4096 and 16384 clips with 1 and 4 copies, D = 64, k = 5 (both passes, 24 launches and the copy of the 32
             words; host clock around the call, which ends in that copy), beside FGDAccumulator.result() on the same rows, and, up to
             --host-clips clips, the host route: the table copied out, then scipy's cdist (squared Euclidean, in row blocks) with
             np.partition; its four values are compared with the device's (they agree to rounding, not to the bit: cdist sums in another order)
    kernels  the two all-pairs kernels alone at the largest case by HIP events: the radii of the generated set and the cross pass generated x
             real, with the float64 operations per second they reach (3 D per pair: subtract, multiply, add)
Appends to profiles/r30_prdc_bench.jsonl.

    python tools/prdc_bench.py [--reps 10] [--host-clips 4096] [--out profiles/r30_prdc_bench.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from speechdrivestemplates_amd import _lib, fgd, prdc  # noqa: E402
from tools._timing import gpu_ms_alternating, host_ms  # noqa: E402

INNER = 20  # calls between two events: one add is a few microseconds, a window of one measures the event pair
DH, K = 32, 5


def features(rng, rows):
    """mu_pred, logvar_pred, mu_gt, logvar_gt: the prediction a shifted, narrower cloud"""
    return [torch.from_numpy((s * rng.standard_normal((rows, DH)) + o).astype(np.float32)).cuda() for s, o in ((0.8, 0.3), (0.8, 0.0), (1, 0), (1, 0))]


def bench_add(reps):
    rng, lines = np.random.Generator(np.random.PCG64(3)), []
    x = features(rng, 32)
    for m in (1, 4):
        acc, ref = prdc.FeatureSetAccumulator(32 // m, 2 * DH, m, K), fgd.FGDAccumulator(2 * DH)
        idx = torch.arange(32 // m, dtype=torch.int64, device="cuda")
        (ms, mn), (fms, fmn) = gpu_ms_alternating([lambda: acc.add(*x, idx), lambda: ref.add(x[0], x[2], x[1], x[3])], reps, INNER)
        lines.append({"tool": "prdc_bench", "case": "add", "rows": 32, "columns": 2 * DH, "copies": m, "launches": 1, "add_ms": ms,
                      "add_min_ms": mn, "fgd_add_ms": fms, "fgd_add_min_ms": fmn, "add_over_fgd_add": ms / fms})
    return lines


def host_route(acc):
    """what a user without this module does: the features to the host, all pairs with cdist in blocks of rows -> the four values"""
    from scipy.spatial.distance import cdist
    g = prdc.gather_model([acc.state().cpu().numpy()], acc.dim, acc.copies)
    real, gen, k = g['real'], g['gen'], acc.k

    def radii(x):
        out = np.empty(len(x))
        for lo in range(0, len(x), 2048):
            d = cdist(x[lo:lo + 2048], x, 'sqeuclidean')
            d[np.arange(d.shape[0]), lo + np.arange(d.shape[0])] = np.inf
            out[lo:lo + 2048] = np.partition(d, k - 1, axis=1)[:, k - 1]
        return out
    ra, rb = radii(real), radii(gen)
    balls, recalled, nearest = np.zeros(len(gen), dtype=np.int64), np.zeros(len(real), dtype=bool), np.full(len(real), np.inf)
    for lo in range(0, len(gen), 2048):
        d = cdist(gen[lo:lo + 2048], real, 'sqeuclidean')
        balls[lo:lo + 2048] = (d <= ra[None, :]).sum(axis=1)
        recalled |= (d <= rb[lo:lo + 2048, None]).any(axis=0)
        nearest = np.minimum(nearest, d.min(axis=0))
    return {'precision': (balls > 0).mean(), 'recall': recalled.mean(), 'density': balls.sum() / (k * len(gen)), 'coverage': (nearest <= ra).mean()}


def bench_result(N, m, reps, host_clips):
    rng = np.random.Generator(np.random.PCG64(N + m))
    acc, ref = prdc.FeatureSetAccumulator(N, 2 * DH, m, K), fgd.FGDAccumulator(2 * DH)
    for lo in range(0, N, 512):
        B = min(512, N - lo)
        x = features(rng, m * B)
        acc.add(*x, torch.arange(lo, lo + B, dtype=torch.int64))
        ref.add(x[0], x[2], x[1], x[3])
    res = acc.result()
    assert res['rows_real'] == N and res['rows_gen'] == N * m and res['err'] == 0
    ms, mn = host_ms(acc.result, reps)
    fms, fmn = host_ms(lambda: ref.result(strict=False), reps)
    line = {"tool": "prdc_bench", "case": "result", "clips": N, "copies": m, "D": 2 * DH, "k": K, "reps": max(reps, 5), "result_ms": ms,
            "result_min_ms": mn, "fgd_result_ms": fms, "fgd_result_min_ms": fmn, "result_over_fgd_result": ms / fms,
            "values": {v: res[v] for v in prdc.VALUES}, "floor": {v: res[v + '_floor'] for v in prdc.VALUES}}
    line["pairs_per_result"] = N * N + (N * m) ** 2 + 2 * N * N * m + 2 * ((N + 1) // 2) ** 2 + 2 * ((N + 1) // 2) * (N // 2)  # (both passes)
    if N <= host_clips:
        t = time.perf_counter()
        host = host_route(acc)
        line.update(host_ms=(time.perf_counter() - t) * 1e3, host_calls=1, host_over_result=(time.perf_counter() - t) * 1e3 / ms,
                    host_values=host, host_max_abs_difference=max(abs(float(host[v]) - res[v]) for v in prdc.VALUES))
    return line, acc


def bench_kernels(acc, reps):
    """the two all-pairs launches (with their merges) on the sets the last result() left on the device"""
    st, lib, p = acc._sets, _lib.load(), lambda t: C.c_void_p(t.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    n_real, n_gen = p(st.counts), C.c_void_p(st.counts.data_ptr() + 8)
    nr, ng = acc._last
    s_knn, s_cross = int(lib.sdt_prdc_slices(st.gen_cap, st.gen_cap)), int(lib.sdt_prdc_slices(st.gen_cap, st.real_cap))
    part = torch.empty(max(s_knn * st.gen_cap * 16, s_cross * st.gen_cap * 3), dtype=torch.int64, device="cuda")
    scratch = [torch.empty(st.gen_cap, dtype=torch.int64, device="cuda") for _ in range(3)]

    def knn():
        _lib.check(lib.sdt_prdc_knn(p(st.gen), n_gen, st.gen_cap, acc.dim, acc.k, s_knn, p(part), part.numel(), p(scratch[0]), stream))

    def cross():
        _lib.check(lib.sdt_prdc_cross(p(st.gen), n_gen, st.gen_cap, p(st.real), n_real, st.real_cap, p(st.rows['real_radius']), acc.dim, s_cross,
                                      p(part), part.numel(), p(scratch[0]), p(scratch[1]), p(scratch[2]), stream))
    (kms, kmn), (cms, cmn) = gpu_ms_alternating([knn, cross], max(reps, 5), 1, warmup=1)
    ops = 3 * acc.dim
    return {"tool": "prdc_bench", "case": "kernels", "rows_real": nr, "rows_gen": ng, "D": acc.dim, "k": acc.k, "knn_gen_ms": kms,
            "knn_gen_min_ms": kmn, "knn_slices": s_knn, "knn_f64_ops_per_s": ng * ng * ops / (kmn * 1e-3), "cross_gen_real_ms": cms,
            "cross_gen_real_min_ms": cmn, "cross_slices": s_cross, "cross_f64_ops_per_s": ng * nr * ops / (cmn * 1e-3)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-clips", type=int, default=4096, help="the host route is timed up to this many clips (it takes seconds beyond)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r30_prdc_bench.jsonl"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the bench needs the GPU"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        def emit(line):
            line["device"] = torch.cuda.get_device_name(0)
            text = json.dumps(line)
            f.write(text + "\n")
            f.flush()
            print(text, flush=True)
        for line in bench_add(a.reps):
            emit(line)
        acc = None
        for N in (512, 4096, 16384):
            for m in (1, 4):
                line, acc = bench_result(N, m, a.reps, a.host_clips)
                emit(line)
        emit(bench_kernels(acc, a.reps))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
