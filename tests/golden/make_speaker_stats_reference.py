#!/usr/bin/env python
"""Record the reference's speaker statistics of the synthetic speakers of synth_speaker_stats.py into
tests/golden/speaker_stats_reference.npz (outputs only; the tests regenerate the clips from their seeds).

Per case (synth_speaker_stats.CASES): the reference's own cal_mean_parted, cal_std_parted and cal_std_global
(data_preprocess/4_1_calculate_mean_std.py, loaded from its file) run chunk by chunk on the training rows of processed_137.csv,
combined with cal_mean_std's np.average lines (:193-225) and reduced 137 -> 121 with 4_2_parse_mean_std_npz.py's delete_idx.
The reference's cal_mean_global raises on the first clip (:26-27 compares a scalar with a 2-vector): that is recorded, and the
global mean comes from global_mean_restated below, cal_mean_global with the component-wise test of cal_std_global.

Usage:  python tests/golden/make_speaker_stats_reference.py REFERENCE_CHECKOUT   (a checkout of the reference project)
"""
import importlib.util
import os
import sys
import tempfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import synth_speaker_stats as S  # noqa: E402

OUT = os.path.join(HERE, "speaker_stats_reference.npz")
DELETE_137 = [1] + list(range(8, 15)) + list(range(17, 25))


def load_4_1(ref_root):
    spec = importlib.util.spec_from_file_location("_ref_4_1", os.path.join(ref_root, "data_preprocess", "4_1_calculate_mean_std.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def global_mean_restated(paths):
    """the running mean of cal_mean_global for one chunk, with the skip test written per component"""
    num = np.zeros((64, 137))
    avg = np.zeros((64, 2, 137))
    for fn in paths:
        pose = np.load(fn)["pose"]
        for i in range(64):
            root = pose[i, :2, 1]
            pose[i, :2, 0:1] -= pose[i, :2, 1, None]
            pose[i, :2, 2:] -= pose[i, :2, 1, None]
            for k in range(137):
                if abs(pose[i, 0, k] + root[0]) < 5 and abs(pose[i, 1, k] + root[1]) < 5:
                    continue
                w = num[i, k] / (num[i, k] + 1)
                avg[i, :, k] = avg[i, :, k] * w + (1 - w) * (pose[i, :2, k])
                num[i, k] += 1
    return avg


def combine(per_chunk):
    """cal_mean_std :204-205 / :224-225"""
    return np.expand_dims(np.average(np.average(np.array(per_chunk), axis=0), axis=0), axis=0)


def main(ref_root):
    ref = load_4_1(ref_root)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for sp in S.SPEAKERS:
            S.write_named(tmp, sp)
        for case, (sp, C) in S.CASES.items():
            df = pd.read_csv(os.path.join(tmp, sp, "processed_137.csv"))
            paths = [os.path.join(tmp, sp, f) for f in df[df["dataset"] == "train"]["pose_fn"]]
            stride = len(paths) // C
            chunks = [paths[c * stride:(c + 1) * stride] for c in range(C)]
            try:
                ref.cal_mean_global((chunks[0], 0))
                raises = False
            except ValueError:
                raises = True
            assert raises, "the reference's cal_mean_global no longer raises: record its global mean instead"
            mp = combine([ref.cal_mean_parted((ch, c)) for c, ch in enumerate(chunks)])
            mg = combine([global_mean_restated(ch) for ch in chunks])
            ap = np.array([mp.squeeze() for _ in range(64)])
            ag = np.array([mg.squeeze() for _ in range(64)])
            sp_ = combine([ref.cal_std_parted((ap, ch, c)) for c, ch in enumerate(chunks)])
            sg = combine([ref.cal_std_global((ag, ch, c)) for c, ch in enumerate(chunks)])
            for name, a in (("parted_mean", mp), ("parted_std", sp_), ("global_mean", mg), ("global_std", sg)):
                out["%s/%s137" % (case, name)] = a[0]
                out["%s/%s" % (case, name)] = np.delete(a, DELETE_137, axis=2).reshape(-1)  # 4_2:16-23, (1, 2, 121) -> 242
            out["%s/num_chunks" % case] = np.int64(C)
            out["%s/clips_used" % case] = np.int64(stride * C)
            out["%s/clips_dropped" % case] = np.int64(len(paths) - stride * C)
    out["global_mean_reference_raises"] = np.bool_(True)
    np.savez(OUT, **out)
    print("wrote", OUT, len(out), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: make_speaker_stats_reference.py REFERENCE_CHECKOUT")
    main(sys.argv[1])
