"""Seeded synthetic speakers for the speaker-statistics tests (speechdrivestemplates_amd/speaker_stats.py), in the on-disk layout of
synth_clips.py (processed_137.csv + one npz per clip with pose (frames, 3, 137) in pixels and raw audio).

Everything the statistics must survive is planted at fixed training rows (positions among the csv's 'train' rows):
  * scattered undetected keypoints, (0, 0, 0), in every clip; every lower-body column (8..14, 19..24) undetected throughout;
  * keypoint ONE_CHUNK_KP undetected in training rows [0, 2) only, i.e. in the first chunk of 10 (23 rows: stride 2);
  * an undetected root (keypoint 1) in frames [0, 10) of row ROOT_ROW;
  * at row EDGE_ROW, frame EDGE_FRAME: an integral root and coordinates at exactly 5.0 (kept: the test is a strict <) and just
    below it (skipped);
  * clips of 64, 70, 80 and 66 frames (only the first NUM_FRAMES count), 'dev' rows in between (ignored);
  * optionally a keypoint that is never detected (its std is 0), a NaN coordinate, a clip that is too short.
"""
import os

import numpy as np
import pandas as pd

ONE_CHUNK_KP = 3
ROOT_ROW = 4
EDGE_ROW, EDGE_FRAME = 5, 3
LOWER_BODY = list(range(8, 15)) + list(range(19, 25))
FRAMES = (64, 70, 64, 80, 66)

# (speaker, training rows, seed, dtype, never-detected keypoint) -> the fixture's cases add num_chunks
SPEAKERS = {
    "synth_f64": dict(n_train=23, seed=101, dtype="float64", never_detected=None),
    "synth_f32": dict(n_train=23, seed=202, dtype="float32", never_detected=None),
    "synth_zero": dict(n_train=12, seed=303, dtype="float64", never_detected=15),
}
CASES = {  # case -> (speaker, num_chunks)
    "f64_c10": ("synth_f64", 10), "f64_c3": ("synth_f64", 3), "f64_c1": ("synth_f64", 1),
    "f32_c10": ("synth_f32", 10), "f32_c3": ("synth_f32", 3), "f32_c1": ("synth_f32", 1),
    "zero_c3": ("synth_zero", 3),
}


def write_stats_speaker(root, speaker, n_train=23, seed=101, dtype="float64", never_detected=None, features=True, nan_at=None,
                        short_row=None, csv="processed_137.csv", audio_len=68266, dev_every=4, frames=FRAMES):
    """-> the speaker directory.  nan_at = (training row, frame, keypoint) gets a NaN x; short_row gets 40 frames.
    Every ``dev_every``-th csv row is a 'dev' clip (not part of the statistics)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    d = os.path.join(root, speaker)
    os.makedirs(os.path.join(d, "clips"), exist_ok=True)
    rows, t, i = [], 0, 0
    while t < n_train:
        is_dev = dev_every and i % dev_every == dev_every - 1
        T = 40 if (not is_dev and t == short_row) else frames[i % len(frames)]
        pose = np.empty((T, 3, 137), dtype=np.float64)
        pose[:, 0] = 640 + 150 * rng.standard_normal((T, 137))
        pose[:, 1] = 360 + 120 * rng.standard_normal((T, 137))
        pose[:, 2] = rng.uniform(0, 1, (T, 137))
        if features:
            fz, kz = np.nonzero(rng.uniform(0, 1, (T, 137)) < 0.02)
            pose[fz, :, kz] = 0.0  # scattered undetected keypoints: (0, 0, 0)
            pose[:, :, LOWER_BODY] = 0.0
            if not is_dev:
                if t < 2:
                    pose[:, :, ONE_CHUNK_KP] = 0.0
                if t == ROOT_ROW:
                    pose[:10, :, 1] = 0.0
                if t == EDGE_ROW:
                    f = EDGE_FRAME
                    pose[f, :2, 1] = (640.0, 360.0)
                    pose[f, :2, 0] = (5.0, 5.0)        # kept: 5 < 5 is false
                    pose[f, :2, 2] = (4.9999, 4.0)     # skipped
                    pose[f, :2, 5] = (5.0, 4.0)        # kept
                    pose[f, :2, 6] = (-4.9999, -4.9999)  # skipped
                    pose[f, :2, 15] = (4.999999, 5.0)  # kept
        if never_detected is not None:
            pose[:, :, never_detected] = 0.0
        if nan_at is not None and not is_dev and t == nan_at[0]:
            pose[nan_at[1], 0, nan_at[2]] = np.nan
        audio = (0.1 * rng.standard_normal(audio_len)).astype(np.float32)
        fn = "clips/%05d.npz" % i
        np.savez(os.path.join(d, fn), pose=pose.astype(dtype), audio=audio)
        rows.append({"dataset": "dev" if is_dev else "train", "start": i * 4.0, "end": i * 4.0 + 4.27, "interval_id": "iv%d" % i,
                     "pose_fn": fn, "audio_fn": "a%d.wav" % i, "video_fn": "v.mp4", "speaker": speaker})
        t += 0 if is_dev else 1
        i += 1
    pd.DataFrame(rows).to_csv(os.path.join(d, csv), index=False)
    return d


def write_named(root, speaker, **kw):
    """one of SPEAKERS, regenerated from its seed"""
    return write_stats_speaker(root, speaker, **dict(SPEAKERS[speaker], **kw))
