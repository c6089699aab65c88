"""Time the pose augmentation (csrc/pose_augment.hip) by HIP events.  One JSON line:
    kernels   at B = 32, T = 64, K = 121 with the confidences: pose_augment.augment_poses with every augmentation on (the parameter launch and
              the element pass, into buffers given by the caller), with the mirror alone, with identity options (the pass copies bits),
              without the confidences, the whole PoseAugmenter call (which allocates its outputs), and a device-to-device copy_ of the same
              (32, 64, 2, 121) float32 tensor -- the yardstick.  Median and minimum of --reps windows of 10 back-to-back calls, the cases taking
              turns window by window.  augment_over_copy = augment_ms / copy_ms.  The tensor is 1.98 MB: at this size every case is a few
              microseconds of launch overhead, not bandwidth, so the ratio says how many launches a call is, not how fast its loads are.
Appends to profiles/r26_pose_augment_bench.jsonl.

    python tools/pose_augment_bench.py [--reps 20] [--out profiles/r26_pose_augment_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from speechdrivestemplates_amd import pose_augment as PA  # noqa: E402
from tools._timing import gpu_ms_alternating  # noqa: E402
from tools.augment_bench import INNER  # noqa: E402

B, T, K = 32, 64, 121
OPTS = dict(seed=1234, mirror_prob=0.5, scale_pct=10.0, rot_deg=15.0)


def bench_kernels(reps):
    rng = np.random.Generator(np.random.PCG64(3))
    dev = torch.device("cuda", torch.cuda.current_device())
    poses = torch.from_numpy(rng.standard_normal((B, T, 2, K)).astype(np.float32)).to(dev)
    score = torch.from_numpy(rng.uniform(0, 1, (B, T, 2, K)).astype(np.float32)).to(dev)
    mean = torch.from_numpy(rng.standard_normal((B, 2 * K)) * 20.0).to(dev)
    std = torch.from_numpy(rng.uniform(2.0, 30.0, (B, 2 * K))).to(dev)
    clips = torch.arange(B, dtype=torch.int64, device=dev)
    step = torch.tensor([7], dtype=torch.int64, device=dev)
    cases = {"augment": PA.options(**OPTS), "mirror_only": PA.options(seed=1234, mirror_prob=1.0), "identity": PA.options(seed=1234)}
    tables = {k: PA.device_tables(o, dev) for k, o in cases.items()}
    perm = PA.perm_array(PA.default_perm(K))
    out, sout, dst = torch.empty_like(poses), torch.empty_like(score), torch.empty_like(poses)
    rec = torch.zeros((B, PA.REC_COLS), dtype=torch.int64, device=dev)
    aug = PA.PoseAugmenter(cases["augment"], dev, 4096)

    def call(name, with_score=True):
        return lambda: PA.augment_poses(poses, score if with_score else None, mean, std, clips, step, cases[name], 4096, perm, tables[name], rec,
                                        out, sout if with_score else None)

    names = ("augment", "mirror_only", "identity", "augment_no_score", "augmenter", "copy")
    res = gpu_ms_alternating([call("augment"), call("mirror_only"), call("identity"), call("augment", False),
                              lambda: aug(poses, score, mean, std, clips, step), lambda: dst.copy_(poses)], reps, INNER)
    line = {"tool": "pose_augment_bench", "case": "kernels", "device": torch.cuda.get_device_name(0), "reps": reps, "inner": INNER, "B": B, "T": T,
            "K": K, "options": OPTS, "pose_bytes": 2 * B * T * 2 * K * 4, "launches": {"augment": 2, "augmenter": 2, "copy": 1}}
    for name, (ms, mn) in zip(names, res):
        line[name + "_ms"], line[name + "_min_ms"] = ms, mn
    line["augment_over_copy"] = line["augment_ms"] / line["copy_ms"]
    line["augment_no_score_over_copy"] = line["augment_no_score_ms"] / line["copy_ms"]
    return line


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r26_pose_augment_bench.jsonl"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the bench needs the GPU"
    line = bench_kernels(a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        text = json.dumps(line)
        f.write(text + "\n")
        print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
