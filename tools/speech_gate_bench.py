#!/usr/bin/env python
"""Time of the audio activity gate (clip_builder.device_speech_gate, csrc/speech_gate.hip) on the 20-minute
synthetic track of tools/clip_builder_bench.py (48 kHz stereo int16 noise), next to ``device_resample`` on the same track: the sibling
kernel to read the gate against.  Per stage: HIP-event time of --iters back-to-back calls after --warmup calls, the median and the
spread over --repeats such measurements (allocation of the stage's outputs included: it is what build_clips pays).  One JSON line per
run, appended to --out.

    python tools/speech_gate_bench.py [--frames 18000] [--out profiles/r22_speech_gate_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(torch, fn, warmup, iters, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=18000, help="video length in 15 fps frames (18000 = 20 minutes)")
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r22_speech_gate_bench.jsonl"))
    import torch
    from speechdrivestemplates_amd import clip_builder as cb
    cb.add_speech_gate_options(ap)
    a = ap.parse_args()
    gate = cb.speech_gate_option(a) or cb.speech_gate_params({'min_permille': 500})
    margin, abs_floor = cb.gate_constants(gate)
    g = np.random.Generator(np.random.PCG64(1))
    samples = a.frames * a.rate // 15
    pcm = np.round(g.uniform(-0.9, 0.9, (samples, 2)) * 32767).astype(np.int16)
    pcm[samples // 3:samples // 2] //= 4096  # a quiet third, so that the mask and the smoothing have something to decide
    start, frames = 80, 64
    mono = cb.device_pcm_to_mono(pcm, cb.source_cut(start, a.rate), 'cuda')
    audio = cb.device_resample(mono, a.rate)
    starts = np.arange(start, a.frames - frames, cb.STEP)
    offs = [cb.audio_offsets(int(s), start, frames) for s in starts]
    starts_dev = torch.from_numpy(starts.astype(np.int32)).cuda()
    e, flag = cb.device_hop_energy(audio)
    raw, stats = cb.device_speech_mask(e, gate['floor_pct'], margin, abs_floor)
    active = cb.device_speech_smooth(raw, gate['min_run_hops'], gate['hang_hops'])
    win = cb.device_speech_windows(active, audio.numel(), starts_dev, offs, gate['min_permille'])
    t = (a.warmup, a.iters, a.repeats)
    stages = {
        "resample": timed(torch, lambda: cb.device_resample(mono, a.rate), *t),
        "gate_energy": timed(torch, lambda: cb.device_hop_energy(audio), *t),
        "gate_mask": timed(torch, lambda: cb.device_speech_mask(e, gate['floor_pct'], margin, abs_floor), *t),
        "gate_smooth": timed(torch, lambda: cb.device_speech_smooth(raw, gate['min_run_hops'], gate['hang_hops']), *t),
        "gate_windows": timed(torch, lambda: cb.device_speech_windows(active, audio.numel(), starts_dev, offs, gate['min_permille']), *t),
    }
    gate_ms = sum(v["median_ms"] for k, v in stages.items() if k.startswith("gate_"))
    line = {"tool": "speech_gate_bench", "frames": a.frames, "sample_rate": a.rate, "samples_16k": int(audio.numel()), "hops": int(e.numel()),
            "windows": len(offs), "kept": int(win['n_kept'].item()), "active_raw": int(raw.sum().item()), "active": int(active.sum().item()),
            "flag": int(flag.item()), "floor": float(stats[0].item()), "thr": float(stats[1].item()), "gate": gate,
            "warmup": a.warmup, "iters": a.iters, "repeats": a.repeats, "stages": stages, "gate_ms": round(gate_ms, 5),
            "gate_over_resample": round(gate_ms / stages["resample"]["median_ms"], 4), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
