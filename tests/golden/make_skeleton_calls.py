#!/usr/bin/env python
"""Record every cv2.line call the REFERENCE's drawing code makes, so that the renderer's tests need no reference sources and no OpenCV:

    tests/golden/skeleton_calls_reference.npz

For each case the file holds the input poses (``<case>/poses``, and ``<case>/gt`` for the pair view) and the calls in call order:
``<case>/calls`` int32 (n, 10) = [image, x_off, view_h, view_w, x0, y0, x1, y1, thickness, line_type] and ``<case>/colour`` float64 (n, 3),
the colour argument exactly as passed (the renderer converts it the way cv2 converts a Scalar to uint8).  ``image`` is the frame number
(clips) or 0 (long image); ``x_off`` is the column of the drawn-into view inside its canvas (long-image windows are numpy views);
(view_h, view_w) is the shape of the view, i.e. the clip window of the stroke.  ``<case>/canvas`` is the canvas (H, W) the call returned.

Cases: realistic +-300 px poses at VISUALIZATION_SCALING 0.85 with a few keypoints far off the canvas and a few whose endpoints are
negative fractions (truncation toward zero), on 720x1280 and on the odd 721x1279 canvas; the pair view; long images of T = 36, 64 and
360 (frames the long image does not draw are zero, which keeps the file small).
Run where the reference sources are:  python tests/golden/make_skeleton_calls.py <reference checkout>
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
K = 121


class _Recorder:
    def __init__(self):
        self.calls, self.colours, self.bases = [], [], {}

    def line(self, img, p0, p1, color, thickness, line_type=None):
        base = img.base if img.base is not None else img
        image = self.bases.setdefault(id(base), len(self.bases))
        x_off = (img.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // img.strides[1]
        for v in (*p0, *p1):
            assert isinstance(v, int), "the reference passes Python ints"
        self.calls.append([image, x_off, img.shape[0], img.shape[1], p0[0], p0[1], p1[0], p1[1], thickness, line_type])
        self.colours.append([float(c) for c in color])
        return img


def _install_stubs(rec):
    cv2 = types.ModuleType("cv2")
    cv2.LINE_AA = 16
    cv2.line = rec.line
    sys.modules["cv2"] = cv2
    tqdm = types.ModuleType("tqdm")
    tqdm.tqdm = lambda it, *a, **k: it
    sys.modules["tqdm"] = tqdm


def _poses(rng, T, off_canvas=True):
    """(T, 2, K) relative poses: a +-300 px body with per-frame jitter; some keypoints far away, some at negative fractions."""
    body = rng.uniform(-300.0, 300.0, size=(1, 2, K))
    p = body + rng.normal(0.0, 12.0, size=(T, 2, K))
    if off_canvas:
        p[0, 0, 10] = 2600.3   # face keypoint far right of the canvas
        p[1, 1, 90] = -1500.7  # a hand keypoint far above it
        p[2 % T, :, 3] = 40000.0  # pose keypoint far outside both axes
        # endpoints that land on negative fractions after p*0.85 + centre: int() must truncate toward zero
        p[0, 0, 100] = (-0.305 - 640.0) / 0.85
        p[0, 1, 100] = (-0.75 - 360.0) / 0.85
        p[1 % T, 0, 20] = (-1.4 - 640.0) / 0.85
    return p


def main(ref):
    sys.path.insert(0, os.path.abspath(ref))
    rec = _Recorder()
    _install_stubs(rec)
    from core.utils import keypoint_visualization as kv  # the reference's own drawing code, driving the recording stub

    rng = np.random.default_rng(20261016)
    out = {}

    def run(case, fn, *args, **arrays):
        rec.calls, rec.colours, rec.bases = [], [], {}
        res = fn(*args)
        out[case + "/calls"] = np.asarray(rec.calls, dtype=np.int32)
        out[case + "/colour"] = np.asarray(rec.colours, dtype=np.float64)
        out[case + "/canvas"] = np.asarray(res.shape[-3:-1], dtype=np.int32)
        for k, v in arrays.items():
            out[case + "/" + k] = v

    s = 0.85
    p = _poses(rng, 8)
    run("clip", kv.vis_relative_pose_clip, p * s, (720, 1280), poses=p)
    p = _poses(rng, 4)
    run("clip_odd", kv.vis_relative_pose_clip, p * s, (721, 1279), poses=p)
    p, g = _poses(rng, 6), _poses(rng, 6, off_canvas=False)
    run("pair", kv.vis_relative_pose_pair_clip, p * s, g * s, (720, 1280), poses=p, gt=g)
    for T in (36, 64, 360):
        p = _poses(rng, T, off_canvas=T == 36) * 1.2
        keep = np.zeros(T, bool)
        keep[::8] = True
        p[~keep] = 0.0
        run("long%d" % T, kv.draw_pose_frames_in_long_img, p.transpose(0, 2, 1), poses=p)
    out["scaling"] = np.asarray(s)
    path = os.path.join(HERE, "skeleton_calls_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items() if k.endswith("/calls")})


if __name__ == "__main__":
    main(sys.argv[1])
