"""Time the audio augmentation (csrc/augment.hip) by HIP events.  JSON lines:
    kernels   at B = 32, L = 68266, every augmentation on (noise on every clip): augment.sumsq, augment.augment_audio (given the sums: the
              parameter kernel and the audio pass), the same with the noise off (no Philox per sample), the same at L = 68272 (a multiple of
              4: every row starts on a 16-byte boundary) with and without the shift, augment.mel_mask on (32, 80, 427), the
              whole Augmenter.audio, and a device-to-device copy_ of the same (32, 68266) float32 tensor -- the yardstick: the audio pass moves
              the same bytes.  Median and minimum of --reps windows of 10 back-to-back calls, the functions taking turns window by window.
              audio_over_copy = audio_ms / copy_ms.
    step      Voice2Pose train steps (forward_backward + optimizer_updates, as train_step runs them) of voice2pose_sdt_bp at 32 clips with the key
              off and with everything enabled, two pipelines taking turns step by step after --warmup steps of each: median ms per step.
Appends to profiles/r21_augment_bench.jsonl.

    python tools/augment_bench.py [--reps 20] [--steps 40] [--warmup 10] [--out profiles/r21_augment_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from speechdrivestemplates_amd import augment as A  # noqa: E402
from tools._timing import gpu_ms_alternating  # noqa: E402

INNER = 10
B, L, M, F = 32, 68266, 80, 427
OPTS = dict(seed=1234, gain_db=6.0, snr=(5.0, 30.0), noise_prob=1.0, shift_ms=50.0, shift=800, polarity=True, freq_masks=(2, 15),
            time_masks=(2, 40))
KEYS_ON = ["TRAIN.AUGMENT.ENABLE", True, "TRAIN.AUGMENT.SEED", 1234, "TRAIN.AUGMENT.GAIN_DB", 6.0, "TRAIN.AUGMENT.NOISE_SNR_DB", [5.0, 30.0],
           "TRAIN.AUGMENT.SHIFT_MS", 50.0, "TRAIN.AUGMENT.POLARITY", True, "TRAIN.AUGMENT.MEL_FREQ_MASKS", [2, 15],
           "TRAIN.AUGMENT.MEL_TIME_MASKS", [2, 40]]


def bench_kernels(reps):
    rng = np.random.Generator(np.random.PCG64(3))
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.from_numpy((0.1 * rng.standard_normal((B, L))).astype(np.float32)).to(dev)
    mel = torch.from_numpy(rng.uniform(0.5, 2.0, (B, M, F)).astype(np.float32)).to(dev)
    clips = torch.arange(B, dtype=torch.int64, device=dev)
    step = torch.tensor([7], dtype=torch.int64, device=dev)
    on, quiet = A.options(**OPTS), A.options(**dict(OPTS, snr=None))
    tables, tables_q = A.device_tables(on, dev), A.device_tables(quiet, dev)
    aug = A.Augmenter(on, dev)
    ss = A.sumsq(x)
    work = torch.empty(B * (-(-L // A.CHUNK)), dtype=torch.float64, device=dev)
    y, rec, dst = torch.empty_like(x), torch.zeros((B, A.REC_COLS), dtype=torch.int64, device=dev), torch.empty_like(x)
    La = 68272  # rows of 16-byte alignment, for what the unaligned rows of L = 68266 cost
    xa = torch.from_numpy((0.1 * rng.standard_normal((B, La))).astype(np.float32)).to(dev)
    ssa, ya, still = A.sumsq(xa), torch.empty_like(xa), A.options(**dict(OPTS, shift=0, shift_ms=0.0))
    names = ("sumsq", "audio", "audio_noise_off", "audio_aligned", "audio_aligned_no_shift", "mel_mask", "augmenter_audio", "copy")
    res = gpu_ms_alternating([lambda: A.sumsq(x, work, ss), lambda: A.augment_audio(x, clips, step, on, tables, ss, rec, y),
                              lambda: A.augment_audio(x, clips, step, quiet, tables_q, ss, rec, y),
                              lambda: A.augment_audio(xa, clips, step, on, tables, ssa, rec, ya),
                              lambda: A.augment_audio(xa, clips, step, still, tables, ssa, rec, ya), lambda: A.mel_mask(mel, clips, step, on, rec),
                              lambda: aug.audio(x, clips, step), lambda: dst.copy_(x)], reps, INNER)
    line = {"tool": "augment_bench", "case": "kernels", "device": torch.cuda.get_device_name(0), "reps": reps, "inner": INNER, "B": B, "L": L,
            "mel": [B, M, F], "options": {k: (list(v) if isinstance(v, tuple) else v) for k, v in OPTS.items()},
            "audio_bytes": 2 * B * L * 4, "launches": {"sumsq": 2, "audio": 2, "mel_mask": 2, "augmenter_audio": 4, "copy": 1}}
    for name, (ms, mn) in zip(names, res):
        line[name + "_ms"], line[name + "_min_ms"] = ms, mn
    line["audio_over_copy"] = line["audio_ms"] / line["copy_ms"]
    line["audio_noise_off_over_copy"] = line["audio_noise_off_ms"] / line["copy_ms"]
    line["copy_GBps"] = line["audio_bytes"] / line["copy_ms"] * 1e-6
    line["audio_GBps"] = line["audio_bytes"] / line["audio_ms"] * 1e-6
    return line


def bench_step(steps, warmup):
    from __graft_entry__ import make_pipeline
    from oracle import sdt_oracle as O
    n_clips = 256
    pipes = {}
    for name, keys in (("off", []), ("on", KEYS_ON)):
        pipe, cfg = make_pipeline("voice2pose_sdt_bp", n_clips, batch_global=B)
        if keys:  # (make_pipeline has no hook for TRAIN keys: rebuild the model's options from a config with them set)
            from speechdrivestemplates_amd.config import check_augment
            cfg = cfg.clone()
            cfg.defrost()
            cfg.merge_from_list(keys)
            cfg.freeze()
            pipe.model.aug_opts = check_augment(cfg)
        pipes[name] = pipe
    dev = torch.device("cuda", torch.cuda.current_device())

    def to_dev(b):
        b = {k: (v.to(dev) if torch.is_tensor(v) and k != "num_frames" else v) for k, v in b.items()}
        b["speaker_stat"] = {k: v.to(dev) for k, v in b["speaker_stat"].items()}
        return b

    batches = [to_dev(O.make_batch(B, n_clips, step=i, seed=1)) for i in range(2)]
    times = {name: [] for name in pipes}
    last = {}
    for i in range(warmup + steps):
        for name, pipe in pipes.items():
            batch = dict(batches[i % 2])
            if name == "on":
                batch["aug_step"] = torch.tensor([i + 1], dtype=torch.int64, device=dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            losses, _ = pipe.forward_backward(batch)
            pipe.optimizer_updates(losses)
            b.record()
            b.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b))
            last[name] = float(losses["G_loss"].detach())
    line = {"tool": "augment_bench", "case": "step", "device": torch.cuda.get_device_name(0), "config": "voice2pose_sdt_bp", "batch": B,
            "steps": steps, "warmup": warmup, "keys_on": KEYS_ON}
    for name in pipes:
        line["step_%s_median_ms" % name], line["step_%s_min_ms" % name] = float(np.median(times[name])), float(np.min(times[name]))
        line["final_G_loss_%s" % name] = last[name]
        pipes[name].close()
    line["on_minus_off_ms"] = line["step_on_median_ms"] - line["step_off_median_ms"]
    return line


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r21_augment_bench.jsonl"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the bench needs the GPU"
    lines = [bench_kernels(a.reps), bench_step(a.steps, a.warmup)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            text = json.dumps(line)
            f.write(text + "\n")
            print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
