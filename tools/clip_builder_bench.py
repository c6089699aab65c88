#!/usr/bin/env python
"""Clip building time (clip_builder.build_clips, csrc/clip_builder.hip): writes one synthetic video (default 18000 frames = 20 minutes
at 15 fps, float32 keypoints, 48 kHz stereo int16 audio, an outlier every 997 frames) to a temporary directory, builds its clips, and
times the same stages of the numpy contract models on the host.  One JSON line per run, appended to --out: kernel time per stage (HIP
events), keypoint-file reading and npz writing seconds and their share of the wall time, and the host models' seconds per stage.

    python tools/clip_builder_bench.py [--frames 18000] [--no-write] [--out profiles/r12_clip_builder_bench.jsonl]

With --repair-max-gap G [--despike H KAPPA [FLOOR_PX]] the video also loses one finger joint for one frame every 131 frames, the repair
stage of DESIGN.md section 26 runs, and the line (its ``repair`` kernel time next to ``flags`` of the same run, and the stage's counts)
goes to profiles/r20_clip_repair_bench.jsonl instead.

With --source-fps P[/Q] [--retime nearest|linear|smooth] the synthetic video is written at that rate (--frames source frames, the audio as
long as they last), the retime stage of DESIGN.md section 27 runs in front of everything else, and the line (its ``retime`` kernel time
next to ``flags`` of the same run, and the stage's counts) goes to profiles/r21_clip_retime_bench.jsonl instead.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def write_video(root, speaker, video, n, rate=48000, dropouts=False, fps=(15, 1)):
    from scipy.io import wavfile
    g = np.random.Generator(np.random.PCG64(1))
    d = os.path.join(root, speaker, 'tmp', 'raw_pose_2d', video)
    os.makedirs(d)
    os.makedirs(os.path.join(root, speaker, 'audio_full'))
    base = g.uniform(200.0, 900.0, (3, 137))
    base[0, 2], base[0, 5] = 400.0, 640.0
    for f in range(n):
        a = (base + g.normal(0.0, 6.0, (3, 137))).astype(np.float32)
        if f % 997 == 500:
            a[:2, 30] = 0.0
        if dropouts and f % 131 == 65:
            a[:, 100] = 0.0  # OpenPose's (0, 0, 0) for a joint it did not detect
        np.save(os.path.join(d, '%s_%06d.npy' % (video, f)), a)
    samples = n * fps[1] * rate // fps[0]
    wavfile.write(os.path.join(root, speaker, 'audio_full', video + '.wav'), rate,
                  np.round(g.uniform(-0.9, 0.9, (samples, 2)) * 32767).astype(np.int16))


def host_models(root, speaker, video, start=80, frames=64):
    """the contract models of the same stages, timed one by one"""
    from scipy.io import wavfile
    from speechdrivestemplates_amd import clip_builder as cb
    plan = cb.plan_clips(root, speaker)[0]
    t = {}
    t0 = time.perf_counter()
    src = np.zeros((plan['n_frames'], 3, 137), np.float32)
    present = np.zeros(plan['n_frames'], bool)
    for i, p in plan['frames'].items():
        src[i] = np.load(p)
        present[i] = True
    t['read_s'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    keep, dist = cb.model_frame_flags(src, present)
    t['flags_s'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    means, _ = cb.model_shoulder_means(dist[keep], 1)
    scalar = cb.model_scalar(means)
    t['shoulder_s'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    starts = cb.model_clip_starts(keep, start, frames)
    t['windows_s'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    scaled = cb.model_scale(src, scalar, True)
    poses = np.stack([scaled[s:s + frames] for s in starts])
    t['gather_poses_s'] = time.perf_counter() - t0
    rate, pcm = wavfile.read(plan['wav'])
    t0 = time.perf_counter()
    mono = cb.model_pcm_to_mono(pcm)[cb.source_cut(start, rate):]
    t['pcm_s'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    track = cb.model_resample(mono, rate)
    t['resample_s'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    audio = [track[slice(*cb.audio_offsets(s, start, frames))] for s in starts]
    t['gather_audio_s'] = time.perf_counter() - t0
    return {k: round(v, 4) for k, v in t.items()}, len(poses), len(audio)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=18000)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None, help="default: profiles/r12_clip_builder_bench.jsonl, with the repair stage "
                                                "profiles/r20_clip_repair_bench.jsonl, with --source-fps profiles/r21_clip_retime_bench.jsonl")
    import torch
    from speechdrivestemplates_amd import clip_builder as cb
    cb.add_repair_options(ap)
    cb.add_retime_options(ap)
    a = ap.parse_args()
    rep = dict(repair_max_gap=a.repair_max_gap, despike=cb.despike_option(ap, a.despike))
    fps = (15, 1)
    if a.source_fps is not None:
        fps = cb.parse_fps(a.source_fps, "--source-fps")
        rep.update(source_fps=fps, retime=a.retime, retime_min_support=a.retime_min_support)
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "r21_clip_retime_bench.jsonl" if a.source_fps is not None else
                             "r20_clip_repair_bench.jsonl" if a.repair_max_gap else "r12_clip_builder_bench.jsonl")
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        write_video(tmp, "bench", "vid", a.frames, dropouts=bool(a.repair_max_gap) or a.source_fps is not None, fps=fps)
        fixture_s = time.perf_counter() - t0
        cb.build_clips(tmp, "bench", write=False, **rep)  # warm-up: library, allocator, page cache
        t0 = time.perf_counter()
        res = cb.build_clips(tmp, "bench", write=not a.no_write, **rep)
        total = time.perf_counter() - t0
        v = res['videos']['vid']
        k = v['timing']
        line = {"tool": "clip_builder_bench", "frames": v['frames'], "dtype": res['dtype'], "sample_rate": v['sample_rate'], "channels": 2,
                "kept": v['kept'], "clips": len(res['table']), "write": not a.no_write,
                "kernel_ms": {s: round(ms, 4) for s, ms in k['kernel_ms'].items()}, "kernel_ms_total": round(sum(k['kernel_ms'].values()), 4),
                "read_s": round(k['read_s'], 4), "write_s": round(k['write_s'], 4), "total_s": round(total, 4),
                "file_io_share": round((k['read_s'] + k['write_s']) / total, 3), "write_fixture_s": round(fixture_s, 2),
                "device": torch.cuda.get_device_name(0)}
        if a.repair_max_gap:
            line["repair_max_gap"], line["despike"], line["repair"] = a.repair_max_gap, rep["despike"], v["repair"]
        if a.source_fps is not None:
            line["source_fps"], line["retime_mode"], line["retime"] = "%d/%d" % fps, a.retime, v.get("retime")
        if not a.skip_host and not a.repair_max_gap and a.source_fps is None:  # (the host models below time the plain 15 fps stages)
            line["host_model"], n_p, n_a = host_models(tmp, "bench", "vid")
            assert n_p == n_a == len(res['table'])
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
