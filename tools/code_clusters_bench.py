"""Time the stages of the code clusters (csrc/code_clusters.hip) by HIP events on two synthetic tables, 30 000 x 32 with
k = 8 and 1 000 000 x 64 with k = 64, and the numpy contract models of code_clusters.py on the host for the same tables.  Each stage is one
ABI call (one seed update, one k-means++ pick, one assignment, one centre update, the final pass), not a whole fit: a fit is k seeds and
as many iterations as the table needs.  Appends one JSON line to profiles/r15_code_clusters_bench.jsonl.  No speed claim rests on it; if
one is made, it is against the host models of the same line.

    python tools/code_clusters_bench.py [--reps 5] [--skip-host] [--out profiles/r15_code_clusters_bench.jsonl]
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
from speechdrivestemplates_amd import code_clusters as CC  # noqa: E402

TABLES = ((30000, 32, 8), (1000000, 64, 64))


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


def bench_table(n, d, k, reps, host):
    lib = _lib.load()
    table = S.make_table((n, d), 70 + d)
    x = torch.from_numpy(table).cuda()
    p, check = CC._p, CC._check
    raw = torch.cuda.current_stream().cuda_stream
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    i64 = dict(dtype=torch.int64, device="cuda")
    u = CC.draw_uniforms(0, k)
    # the state after k - 1 seeds: what the last pick and the last update of a fit see
    seeds, m, _ = CC.choose_seeds(x, k - 1, seed=0)
    seeds = torch.cat([seeds, torch.zeros(1, **i64)])
    m_before = m.clone()
    sws_bytes = lib.sdt_code_clusters_seed_workspace_bytes(n, d)
    sws, info = torch.empty(sws_bytes // 8, **i64), torch.empty(4, **f64)
    # (the workspace holds the chunk sums of m_before: one more update of the last seed leaves m as it is and writes them)
    check(lib.sdt_code_clusters_seed_update(p(x), n, d, p(seeds), k - 2, 0, p(m), p(sws), sws_bytes, raw))
    assert torch.equal(m, m_before)
    gpu = {}
    gpu["seed_pick_ms"] = gpu_ms(lambda: check(lib.sdt_code_clusters_seed_pick(p(m), n, 0, float(u[k - 1]), p(seeds), k - 1, p(info), p(sws), sws_bytes, raw)), reps)
    gpu["seed_update_ms"] = gpu_ms(lambda: check(lib.sdt_code_clusters_seed_update(p(x), n, d, p(seeds), k - 1, 0, p(m), p(sws), sws_bytes, raw)), reps)
    centers0 = x[seeds].double()
    labels, changed = torch.empty(n, **i32), torch.empty(1, **i64)
    gpu["assign_ms"] = gpu_ms(lambda: check(lib.sdt_code_clusters_assign(p(x), n, d, p(centers0), k, p(labels), 1, p(changed), raw)), reps)
    uws_bytes = lib.sdt_code_clusters_update_workspace_bytes(n, d, k)
    uws, counts = torch.empty(uws_bytes // 8, **i64), torch.empty(k, **i32)
    centers1 = centers0.clone()

    def update():  # (from the seed centres every time: the call rewrites its centres in place)
        centers1.copy_(centers0)
        check(lib.sdt_code_clusters_update(p(x), n, d, p(labels), k, p(centers1), p(counts), p(uws), uws_bytes, raw))
    gpu["update_ms"] = gpu_ms(update, reps)
    gpu["centers_copy_ms"] = gpu_ms(lambda: centers1.copy_(centers0), reps)  # (inside update_ms)
    final = {}

    def final_pass():
        final.update(CC.final_pass(x, centers1))
    gpu["final_ms"] = gpu_ms(final_pass, reps)  # (with its workspace and output allocations)
    out = {"rows": n, "dim": d, "k": k, "update_workspace_bytes": int(uws_bytes), "gpu": gpu}
    if host:
        x64 = table.astype(np.float64)
        mb, sd = m_before.cpu().numpy(), seeds.cpu().numpy()
        h = {}
        h["seed_pick_ms"], (row, _) = host_ms(lambda: CC.model_seed_pick(mb, "kmeans++", u[k - 1], sd[:k - 1]))
        h["seed_update_ms"], mm = host_ms(lambda: np.minimum(mb, CC.model_d2(x64, x64[row])))
        c0 = x64[sd]
        h["assign_ms"], (ml, _) = host_ms(lambda: CC.model_assign(x64, c0))
        h["update_ms"], (mc, mcnt) = host_ms(lambda: CC.model_update(x64, ml, c0))
        h["final_ms"], mf = host_ms(lambda: CC.model_final(x64, mc))
        out["host_models"] = h
        equal = [row == int(sd[k - 1]), np.array_equal(mm, m.cpu().numpy()), np.array_equal(ml, labels.cpu().numpy()),
                 int(changed.item()) == n, np.array_equal(mc, centers1.cpu().numpy()), np.array_equal(mcnt, counts.cpu().numpy())]
        equal += [np.array_equal(mf[key], final[key].cpu().numpy()) for key in ("labels", "centers", "counts", "within_ss", "inertia", "code_index",
                                                                             "code_dist2", "order")]
        out["equal_bits"] = bool(all(equal))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r15_code_clusters_bench.jsonl"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the bench needs the GPU"
    line = {"tool": "code_clusters_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps,
            "tables": [bench_table(n, d, k, a.reps, not a.skip_host) for n, d, k in TABLES]}
    text = json.dumps(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
