"""Time the optimiser step of the generator step group at its real sizes (7 075 122 generator parameters and a 4096 x 32 clip-code
table, two flat buffers) by HIP events, three ways, alternating them in one process:
    plain    sdt_adam_step_f32 per buffer (the step with the safeguard keys at their defaults)
    guarded  sum of squares per buffer + guard record + sdt_adam_step_guarded_f32 per buffer (TRAIN.GRAD_CLIP_NORM / SKIP_NONFINITE_STEP)
    ema      the same with the EMA written in the guarded pass (+ TRAIN.EMA_DECAY)
Each sample is one event pair around ``--iters`` back-to-back steps; ``--rounds`` samples per variant, taken in turn.  The yardstick
is the plain step of the same run: by bytes moved the guarded step costs 8/7 of it and 10/7 with the EMA.
Appends one JSON line to profiles/r14_optim_guard_bench.jsonl.

    python tools/optim_guard_bench.py [--iters 50] [--rounds 7] [--out profiles/r14_optim_guard_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from speechdrivestemplates_amd import ops  # noqa: E402

SIZES = (4096 * 32, 7075122)  # optimizerClipCode, optimizerG: the order optimizer_updates steps them in
STREAMS = {"plain": 7, "guarded": 8, "ema": 10}  # fp32 HBM streams per element: p, g, m, v read + p, m, v written; + g for the norm; + ema read and written


class Buffers:
    def __init__(self, n, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.p = torch.randn(n, device="cuda", generator=g)
        self.g = torch.randn(n, device="cuda", generator=g) * 1e-2
        self.m, self.v, self.ema = torch.zeros_like(self.p), torch.zeros_like(self.p), self.p.clone()
        self.state = torch.zeros(2, dtype=torch.int64, device="cuda")
        self.partial = torch.zeros(ops.grad_sumsq_partials(), dtype=torch.float64, device="cuda")


def make_variants(bufs):
    lr = torch.full((1,), 1e-4, device="cuda")
    record = torch.zeros(ops.GUARD_WORDS, dtype=torch.int64, device="cuda")

    def plain():
        for b in bufs:
            ops.adam_step(b.p, b.g, b.m, b.v, lr, b.state)

    def guarded(ema):
        for b in bufs:
            ops.grad_sumsq(b.g, b.partial)
        ops.optim_guard_prep([b.partial for b in bufs], record, 1.0, 1.0, True)
        for b in bufs:
            ops.adam_step_guarded(b.p, b.g, b.m, b.v, lr, b.state, record, ema=b.ema if ema else None, ema_decay=0.999 if ema else 0.0)

    return {"plain": plain, "guarded": lambda: guarded(False), "ema": lambda: guarded(True)}, record


def sample_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r14_optim_guard_bench.jsonl"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the bench needs the GPU"
    bufs = [Buffers(n, 7 + i) for i, n in enumerate(SIZES)]
    variants, record = make_variants(bufs)
    for fn in variants.values():  # warm up every launch shape
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            samples[k].append(sample_ms(fn, a.iters))
    assert int(record[2].item()) == 0 and bool(torch.isfinite(bufs[1].p).all()), "the timed steps must be applied steps"
    elems = sum(SIZES)
    res = {}
    for k, xs in samples.items():
        med = float(np.median(xs))
        res[k] = {"ms_median": med, "ms_min": float(min(xs)), "ms_max": float(max(xs)), "bytes": 4 * STREAMS[k] * elems,
                  "tb_per_s": 4 * STREAMS[k] * elems / (med * 1e-3) / 1e12}
    base = res["plain"]
    line = {"tool": "optim_guard_bench", "device": torch.cuda.get_device_name(0), "sizes": list(SIZES), "iters": a.iters, "rounds": a.rounds,
            "variants": res,
            "plain_spread": (base["ms_max"] - base["ms_min"]) / base["ms_median"],
            "ratio_guarded": res["guarded"]["ms_median"] / base["ms_median"], "byte_ratio_guarded": 8 / 7,
            "ratio_ema": res["ema"]["ms_median"] / base["ms_median"], "byte_ratio_ema": 10 / 7}
    text = json.dumps(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
