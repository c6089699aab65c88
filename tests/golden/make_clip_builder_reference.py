#!/usr/bin/env python
"""Record the reference's clip preparation of the synthetic videos of synth_keypoint_videos.py into
tests/golden/clip_builder_reference.npz (outputs only; the tests regenerate the inputs from their seeds).

The reference's data_preprocess/2_2_remove_outlier.py, 2_3_rescale_shoulder_width.py and 3_1_generate_clips.py are loaded from their
files (they parse sys.argv and create directories at import, so both point into a temporary tree; librosa / tqdm get stand-in modules
when missing) and 3_2_split_train_val_test.py is run as the script it is.  Recorded per speaker and video:
  keep            not check_is_pose_outlier(file), False for a missing file
  means<C>/scalar<C>   cal_mean_shoulder_distance_single_process per chunk of the kept files, C = 1 and 3, and 331.085.../np.average
  starts          the window loop of gen_data_samples (3_1:168-215), its pose half: a start survives iff no get_pose_np raises
  times, a0, a1   frame_idx_to_time(f) and int(audio_start), int(audio_end) (3_1:172-175) for every start index of the fixture
  split           3_2's clips.csv rows: dataset, interval_id, start

Usage:  python tests/golden/make_clip_builder_reference.py REFERENCE_CHECKOUT
"""
import importlib.util
import os
import runpy
import shutil
import sys
import tempfile
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import synth_keypoint_videos as S  # noqa: E402

OUT = os.path.join(HERE, "clip_builder_reference.npz")
RECORDED = ['kp_f64', 'kp_f32']


def stand_ins():
    for name in ("librosa", "tqdm"):
        try:
            importlib.import_module(name)
        except ImportError:
            m = types.ModuleType(name)
            m.tqdm = lambda it=None, **kw: it
            sys.modules[name] = m


def load(ref_root, script, tmp, speaker):
    argv = sys.argv
    sys.argv = [script, "-b", tmp, "-s", speaker]
    try:
        spec = importlib.util.spec_from_file_location("_ref_" + script[:3], os.path.join(ref_root, "data_preprocess", script))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.argv = argv
    return mod


def main(ref_root):
    stand_ins()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for sp in RECORDED:
            base = S.write_speaker(tmp, sp)
            for d in ("frames", "videos"):
                os.makedirs(os.path.join(base, d), exist_ok=True)
            raw = os.path.join(base, "tmp", "raw_pose_2d")
            rescaled = os.path.join(base, "tmp", "rescaled_pose_2d")
            os.makedirs(rescaled)
            r22, r23 = load(ref_root, "2_2_remove_outlier.py", tmp, sp), load(ref_root, "2_3_rescale_shoulder_width.py", tmp, sp)
            r31 = load(ref_root, "3_1_generate_clips.py", tmp, sp)
            csv_dir = os.path.join(base, "tmp", "intermediate_csv")
            for video in S.SPEAKERS[sp][1]:
                n = S.VIDEOS[video]['n']
                keep = np.zeros(n, bool)
                os.makedirs(os.path.join(rescaled, video))
                kept_files = []
                for fn in sorted(os.listdir(os.path.join(raw, video))):
                    path = os.path.join(raw, video, fn)
                    if not r22.check_is_pose_outlier(path):
                        keep[int(os.path.splitext(fn)[0].rpartition('_')[2])] = True
                        shutil.copy(path, os.path.join(rescaled, video, fn))
                        kept_files.append(os.path.join(rescaled, video, fn))
                key = "%s/%s/" % (sp, video)
                out[key + "keep"] = keep
                for C in (1, 3):
                    stride = len(kept_files) // C
                    ans = np.array([r23.cal_mean_shoulder_distance_single_process((kept_files[i * stride:(i + 1) * stride], i)) for i in range(C)])
                    out[key + "means%d" % C] = ans.astype(np.float64)
                    out[key + "means%d_dtype" % C] = np.array(str(ans.dtype))
                    out[key + "scalar%d" % C] = np.float64(331.0850066245443 * 1.0 / np.average(ans, axis=0))
                starts, cand = [], list(range(S.START, n - S.FRAMES, S.STEP))
                for f in cand:
                    try:
                        np.array([r31.get_pose_np(r31.get_pose_path(f + i, video)) for i in range(S.FRAMES)])
                        starts.append(f)
                    except Exception:
                        continue
                out[key + "starts"] = np.array(starts, np.int64)
                t0 = pd.to_timedelta(r31.frame_idx_to_time(S.START))
                out[key + "cand"] = np.array(cand, np.int64)
                out[key + "times"] = np.array([r31.frame_idx_to_time(f) for f in cand] + [r31.frame_idx_to_time(f + S.FRAMES) for f in cand])
                out[key + "a0"] = np.array([int((pd.to_timedelta(r31.frame_idx_to_time(f)) - t0).total_seconds() * r31.SR) for f in cand], np.int64)
                out[key + "a1"] = np.array([int((pd.to_timedelta(r31.frame_idx_to_time(f + S.FRAMES)) - t0).total_seconds() * r31.SR)
                                            for f in cand], np.int64)
                pd.DataFrame({'dataset': ['train'] * len(starts), 'start': starts, 'end': [s + S.FRAMES for s in starts],
                              'interval_id': [video] * len(starts), 'pose_fn': ['x'] * len(starts), 'audio_fn': ['x'] * len(starts),
                              'video_fn': [video] * len(starts), 'speaker': [sp] * len(starts)}).to_csv(
                    os.path.join(csv_dir, "tmp_%s.csv" % video), index=False)
            argv = sys.argv
            sys.argv = ["3_2", "-b", tmp, "-s", sp]
            try:
                runpy.run_path(os.path.join(ref_root, "data_preprocess", "3_2_split_train_val_test.py"), run_name="__main__")
            finally:
                sys.argv = argv
            df = pd.read_csv(os.path.join(base, "clips.csv"))
            out[sp + "/split_columns"] = np.array(list(df.columns))
            out[sp + "/split_dataset"] = np.array(list(df['dataset']))
            out[sp + "/split_video"] = np.array(list(df['interval_id']))
            out[sp + "/split_start"] = np.array(list(df['start']), np.int64)
    np.savez(OUT, **out)
    print("wrote", OUT, len(out), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: make_clip_builder_reference.py REFERENCE_CHECKOUT")
    main(sys.argv[1])
