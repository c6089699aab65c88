"""Time the fused regression loss (ops.RegLossFn, csrc/reg_loss.hip) by HIP events at the training shape
B=32, T=64, C=242 with every option on (mask at 0.3 on uniform scores, part weights [1, 0.5, 2], velocity term), against what it replaces.
One JSON line per case, forward + backward of one call each:
    fused      RegLossFn.apply + (reg + vel).backward(): two launches forward, one backward
    l1         L1LossFn.apply + backward on the same pred / gt: the default step's loss (two launches forward, one backward)
    composed   the same terms from the existing ops: pred * (mask * weights), TimeDiffFn on both operands, L1LossFn on positions and on
               differences (gt is masked outside the timed region; the divisors are element counts, not live counts -- a cost model of
               the composition, not the same number)
and per case
    ms / min_ms        median / minimum over --reps windows of 20 back-to-back calls through autograd, the cases taking turns window by window
    raw_ms             (fused, l1) the three C entry-point launches alone, no autograd and no allocation: what the GPU needs
plus the ratios fused / l1 and fused / composed.  Appends to profiles/r17_reg_loss_bench.jsonl.

    python tools/reg_loss_bench.py [--reps 20] [--out profiles/r17_reg_loss_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from speechdrivestemplates_amd import _lib, ops  # noqa: E402
from speechdrivestemplates_amd.core.datasets.gesture_dataset import PoseTransforms  # noqa: E402
from tools._timing import gpu_ms_alternating  # noqa: E402

INNER = 20  # calls between two events: one call is tens of microseconds, a window of one measures the event pair
B, T, K = 32, 64, 121
LAM_REG, LAM_VEL, MIN_CONF, PARTS = 1.0, 0.5, 0.3, (1.0, 0.5, 2.0)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r17_reg_loss_bench.jsonl"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the bench needs the GPU"
    dev = torch.device("cuda", 0)
    rng = np.random.Generator(np.random.PCG64(17))
    pred = torch.from_numpy(rng.standard_normal((B, T, 2, K)).astype(np.float32)).to(dev).requires_grad_(True)
    gt = torch.from_numpy(rng.standard_normal((B, T, 2, K)).astype(np.float32)).to(dev)
    score = torch.from_numpy(np.repeat(rng.uniform(0, 1, (B, T, 1, K)).astype(np.float32), 2, axis=2)).to(dev)
    chan_w = torch.tensor([PARTS[p] for p in PoseTransforms.part_table()] * 2, dtype=torch.float32, device=dev)
    mw = (score > MIN_CONF).float() * chan_w.reshape(2, K)
    gt_m = gt * mw

    def fused():
        pred.grad = None
        reg, vel = ops.RegLossFn.apply(pred, gt, score, chan_w, LAM_REG, LAM_VEL, MIN_CONF)
        (reg + vel).backward()

    def l1():
        pred.grad = None
        ops.L1LossFn.apply(pred, gt, LAM_REG).backward()

    def composed():
        pred.grad = None
        pm = pred * mw
        reg = ops.L1LossFn.apply(pm, gt_m, LAM_REG)
        vel = ops.L1LossFn.apply(ops.TimeDiffFn.apply(pm.reshape(B, T, -1)), ops.TimeDiffFn.apply(gt_m.reshape(B, T, -1)), LAM_VEL)
        (reg + vel).backward()

    lib, n, C = _lib.load(), pred.numel(), 2 * K
    p_, g_, s_, w_ = (t.data_ptr() for t in (pred.detach(), gt, score, chan_w))
    partial = torch.empty(512, device=dev, dtype=torch.float64)
    counts = torch.empty(512, device=dev, dtype=torch.int64)
    losses, denom = torch.empty(2, device=dev), torch.empty(2, device=dev, dtype=torch.float64)
    one, dp = torch.ones(1, device=dev), torch.empty_like(gt)

    def fused_raw():
        st = ops._stream()
        _lib.check(lib.sdt_reg_loss_fwd_f32(p_, g_, s_, w_, B, T, C, LAM_REG, LAM_VEL, MIN_CONF, partial.data_ptr(), counts.data_ptr(),
                                            losses.data_ptr(), denom.data_ptr(), st))
        _lib.check(lib.sdt_reg_loss_bwd_f32(p_, g_, s_, w_, one.data_ptr(), one.data_ptr(), denom.data_ptr(), B, T, C, LAM_REG, LAM_VEL,
                                            MIN_CONF, dp.data_ptr(), st))

    def l1_raw():
        st = ops._stream()
        _lib.check(lib.sdt_l1_loss_fwd_f32(p_, g_, n, LAM_REG, partial.data_ptr(), losses.data_ptr(), st))
        _lib.check(lib.sdt_l1_loss_bwd_f32(p_, g_, one.data_ptr(), n, LAM_REG, dp.data_ptr(), st))

    names = ["fused", "l1", "composed", "fused_raw", "l1_raw"]
    res = dict(zip(names, gpu_ms_alternating([fused, l1, composed, fused_raw, l1_raw], a.reps, INNER)))
    common = {"tool": "reg_loss_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": INNER, "B": B, "T": T, "C": C,
              "elements": n, "traffic_mb": 4 * n * 4 / 1e6}  # forward reads pred, gt, score; backward reads them again and writes dpred
    lines = []
    for name in ("fused", "l1", "composed"):
        line = dict(common, case=name, ms=res[name][0], min_ms=res[name][1])
        if name + "_raw" in res:
            line["raw_ms"], line["raw_min_ms"] = res[name + "_raw"]
        lines.append(line)
    lines[0].update(fused_over_l1=res["fused"][0] / res["l1"][0], fused_over_composed=res["fused"][0] / res["composed"][0],
                    raw_fused_over_l1=res["fused_raw"][0] / res["l1_raw"][0])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            text = json.dumps(line)
            f.write(text + "\n")
            print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
