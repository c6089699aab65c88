"""Time the fused limb loss (ops.BoneLossFn, csrc/bone_loss.hip) by HIP events at the training shape B=32, T=64,
K=121 on the 108 limbs of the skeleton with both terms, the mask (0.3 on uniform scores) and the part weights [1, 0.5, 2] on, next to the
two regression losses on the same tensors.  One JSON line per case, forward + backward of one call each:
    bone       BoneLossFn.apply + (bone + bone_dir).backward(): two launches forward, one backward
    reg        RegLossFn.apply (mask, weights, velocity) + backward: two launches forward, one backward
    l1         L1LossFn.apply + backward: the default step's loss
and per case
    ms / min_ms        median / minimum over --reps windows of 20 back-to-back calls through autograd, the cases taking turns window by window
    raw_ms             the three C entry-point launches alone, no autograd and no allocation: what the GPU needs
plus the ratios bone / reg through autograd and as bare calls.  Appends to profiles/r23_bone_loss_bench.jsonl.

    python tools/bone_loss_bench.py [--reps 20] [--out profiles/r23_bone_loss_bench.jsonl]
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
LAM_BONE, LAM_DIR, MIN_LEN, MIN_CONF, PARTS = 1.0, 0.5, 1.0, 0.3, (1.0, 0.5, 2.0)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r23_bone_loss_bench.jsonl"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the bench needs the GPU"
    dev = torch.device("cuda", 0)
    rng = np.random.Generator(np.random.PCG64(23))
    pred = torch.from_numpy(rng.standard_normal((B, T, 2, K)).astype(np.float32)).to(dev).requires_grad_(True)
    gt = torch.from_numpy(rng.standard_normal((B, T, 2, K)).astype(np.float32)).to(dev)
    score = torch.from_numpy(np.repeat(rng.uniform(0, 1, (B, T, 1, K)).astype(np.float32), 2, axis=2)).to(dev)
    mean = torch.from_numpy(rng.standard_normal((B, 2 * K)) * 20.0).to(dev)
    std = torch.from_numpy(rng.uniform(2.0, 30.0, (B, 2 * K))).to(dev)
    parts = PoseTransforms.part_table()
    chan_w = torch.tensor([PARTS[p] for p in parts] * 2, dtype=torch.float32, device=dev)
    edges = PoseTransforms.skeleton_edges()
    table = ops.BoneTable(edges, PoseTransforms.part_roots(True), [PARTS[parts[e[0]]] for e in edges])
    E = table.E

    def bone():
        pred.grad = None
        x, y = ops.BoneLossFn.apply(pred, gt, mean, std, score, table, LAM_BONE, LAM_DIR, MIN_CONF, MIN_LEN)
        (x + y).backward()

    def reg():
        pred.grad = None
        x, y = ops.RegLossFn.apply(pred, gt, score, chan_w, 1.0, 0.5, MIN_CONF)
        (x + y).backward()

    def l1():
        pred.grad = None
        ops.L1LossFn.apply(pred, gt, 1.0).backward()

    lib, n, C = _lib.load(), pred.numel(), 2 * K
    p_, g_, s_, w_, m_, sd_ = (t.data_ptr() for t in (pred.detach(), gt, score, chan_w, mean, std))
    tabs = [None if t is None else t.data_ptr() for t in table.on(dev)]
    psum = torch.empty(2 * B * T, device=dev, dtype=torch.float64)
    pcnt = torch.empty(2 * B * T, device=dev, dtype=torch.int64)
    losses, denom = torch.empty(2, device=dev), torch.empty(2, device=dev, dtype=torch.float64)
    one, dp = torch.ones(1, device=dev), torch.empty_like(gt)

    def bone_raw():
        st = ops._stream()
        _lib.check(lib.sdt_bone_loss_fwd_f32(p_, g_, s_, m_, sd_, tabs[0], tabs[1], tabs[2], B, T, K, E, LAM_BONE, LAM_DIR, MIN_CONF, MIN_LEN,
                                             psum.data_ptr(), pcnt.data_ptr(), losses.data_ptr(), denom.data_ptr(), st))
        _lib.check(lib.sdt_bone_loss_bwd_f32(p_, g_, s_, m_, sd_, *tabs, one.data_ptr(), one.data_ptr(), denom.data_ptr(), B, T, K, E,
                                             LAM_BONE, LAM_DIR, MIN_CONF, MIN_LEN, dp.data_ptr(), st))

    def reg_raw():
        st = ops._stream()
        _lib.check(lib.sdt_reg_loss_fwd_f32(p_, g_, s_, w_, B, T, C, 1.0, 0.5, MIN_CONF, psum.data_ptr(), pcnt.data_ptr(), losses.data_ptr(),
                                            denom.data_ptr(), st))
        _lib.check(lib.sdt_reg_loss_bwd_f32(p_, g_, s_, w_, one.data_ptr(), one.data_ptr(), denom.data_ptr(), B, T, C, 1.0, 0.5, MIN_CONF,
                                            dp.data_ptr(), st))

    def l1_raw():
        st = ops._stream()
        _lib.check(lib.sdt_l1_loss_fwd_f32(p_, g_, n, 1.0, psum.data_ptr(), losses.data_ptr(), st))
        _lib.check(lib.sdt_l1_loss_bwd_f32(p_, g_, one.data_ptr(), n, 1.0, dp.data_ptr(), st))

    names = ["bone", "reg", "l1", "bone_raw", "reg_raw", "l1_raw"]
    res = dict(zip(names, gpu_ms_alternating([bone, reg, l1, bone_raw, reg_raw, l1_raw], a.reps, INNER)))
    common = {"tool": "bone_loss_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": INNER, "B": B, "T": T, "K": K,
              "E": E, "frames": B * T, "traffic_mb": 7 * n * 4 / 1e6}  # forward reads pred, gt, score; backward again, and writes dpred
    lines = []
    for name in ("bone", "reg", "l1"):
        line = dict(common, case=name, ms=res[name][0], min_ms=res[name][1])
        line["raw_ms"], line["raw_min_ms"] = res[name + "_raw"]
        lines.append(line)
    lines[0].update(bone_over_reg=res["bone"][0] / res["reg"][0], bone_over_l1=res["bone"][0] / res["l1"][0],
                    raw_bone_over_reg=res["bone_raw"][0] / res["reg_raw"][0], raw_bone_over_l1=res["bone_raw"][0] / res["l1_raw"][0])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            text = json.dumps(line)
            f.write(text + "\n")
            print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
