"""Pose videos and long images drawn on the GPU (csrc/render.hip): the reference's vis_relative_pose_clip,
vis_relative_pose_pair_clip and draw_pose_frames_in_long_img (core/utils/keypoint_visualization.py:96-110,177-207).

The geometry, colours and draw order are the reference's; the anti-aliasing profile is this engine's own (DESIGN.md
section 10).  Results are (frames, H, W, 3) uint8 device tensors in BGR channel order, like the reference's arrays.
Poses are (T, 2, K) or batched (B, T, 2, K), float64 or float32 (widened to float64 first), on the GPU.

Deliberate difference: the reference raises on a non-finite keypoint (int(nan)), which would end a validation epoch;
here an edge with a non-finite endpoint or one beyond 2^24 px is not drawn, counted, and reported with one warning.
"""
import ctypes as C
import warnings

import numpy as np
import torch

from . import _lib
from .ops import _req_cuda, _stream

LONG_H = 720
LONG_W = LONG_H // 3 * 4     # window width w of draw_pose_frames_in_long_img
LONG_STEP = LONG_H * 0.7     # pose_step: 503.99999999999994 in float64, so windows start at int(j * LONG_STEP) = 0, 503, 1007, ...
LONG_INTERVAL = 8

INSTANCE = np.dtype([("pose", "<i8"), ("off_x", "<f8"), ("off_y", "<f8"), ("scale", "<f8"), ("shift_x", "<i4"),
                     ("clip_x0", "<i4"), ("clip_x1", "<i4"), ("reserved", "<i4")])  # sdt_render_instance (include/sdt_hip.h)
assert INSTANCE.itemsize == 48

_warned = [False]
last_skipped = 0  # edges left out by the last public call (non-finite or > 2^24 px endpoints)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _poses(x):
    """-> ((N, T, 2, K) float64 contiguous device tensor, batched?)"""
    if not torch.is_tensor(x):
        raise TypeError("poses must be a torch tensor on the GPU")
    _req_cuda(x)
    if x.dim() not in (3, 4) or x.shape[-2] != 2:
        raise ValueError("poses must be (T, 2, K) or (B, T, 2, K), got %s" % (tuple(x.shape),))
    batched = x.dim() == 4
    x = x if batched else x.unsqueeze(0)
    return x.to(torch.float64).contiguous(), batched


def _refuse_capture():
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("rendering cannot run inside a hipGraph capture (it reads a count back and allocates its output)")


def _table(rows, dev):
    a = np.zeros(len(rows), INSTANCE)
    for i, r in enumerate(rows):
        a[i] = r
    return torch.from_numpy(a.view(np.uint8)).to(dev)


def _launch(poses, inst_rows, n_images, n_inst, H, W, out=None):
    """poses (N, 2, K) float64; inst_rows: n_images * n_inst instance tuples -> (frames (n_images, H, W, 3) uint8, workspace, skipped word)"""
    lib = _lib.load()
    dev = poses.device
    K = int(poses.shape[-1])
    if lib.sdt_render_edges(K) == 0:
        raise ValueError("unsupported number of keypoints: %d (draw_body_parts knows 121, 135 and 137)" % K)
    inst = _table(inst_rows, dev)
    ws_bytes = lib.sdt_render_workspace_bytes(n_images, n_inst, K)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    skipped = torch.empty(1, dtype=torch.int32, device=dev)
    if out is None:
        out = torch.empty((n_images, H, W, 3), dtype=torch.uint8, device=dev)
    st = _stream()
    _lib.check(lib.sdt_render_prepare_f64(_p(poses), poses.shape[0], K, _p(inst), n_images, n_inst, H, W, _p(ws), ws_bytes, _p(skipped), st))
    _lib.check(lib.sdt_render_skeleton_u8(_p(ws), ws_bytes, n_images, n_inst, K, H, W, _p(out), out.numel(), st))
    return out, ws, skipped, inst


def _report(skipped):
    global last_skipped
    last_skipped = int(skipped.item())
    if last_skipped and not _warned[0]:
        _warned[0] = True
        warnings.warn("render: %d skeleton edge(s) with non-finite or out-of-range (> 2^24 px) endpoints were not drawn "
                      "(the reference would raise here); further occurrences are counted in render.last_skipped" % last_skipped)
    return last_skipped


# -- instance layouts of the reference's three drawing functions --------------------------------------------------------------
def clip_instances(n, canvas_size, scaling):
    """vis_relative_pose_clip: pose i on image i, centre (W//2, H//2)."""
    H, W = canvas_size
    return [(i, float(W // 2), float(H // 2), float(scaling), 0, 0, W, 0) for i in range(n)]


def pair_instances(n, canvas_size, scaling):
    """vis_relative_pose_pair_clip: prediction (poses 0..n-1) at int(W*0.33), then ground truth (poses n..2n-1) at int(W*0.67)."""
    H, W = canvas_size
    rows = []
    for i in range(n):
        rows.append((i, float(int(W * 0.33)), float(H // 2), float(scaling), 0, 0, W, 0))
        rows.append((n + i, float(int(W * 0.67)), float(H // 2), float(scaling), 0, 0, W, 0))
    return rows


def long_image_layout(T):
    """draw_pose_frames_in_long_img's arithmetic -> (canvas width, [(pose index, window column x0)] in draw order)."""
    kept = min(T, T - T % LONG_INTERVAL + 1)
    N = kept // LONG_INTERVAL + 1
    width = LONG_W + int((N - 1) * LONG_STEP)
    windows = [(i, int(i // LONG_INTERVAL * LONG_STEP)) for i in range(kept) if i % LONG_INTERVAL == 0]
    return width, windows


def long_instances(B, T):
    width, windows = long_image_layout(T)
    rows = []
    for b in range(B):
        for i, x0 in windows:  # each window's strokes are clipped to the window (cv2 draws into a numpy view of the canvas)
            rows.append((b * T + i, float(LONG_W // 2), float(LONG_H // 2), 1.0, x0, x0, x0 + LONG_W, 0))
    return width, len(windows), rows


# -- public API ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def render_pose_clip(poses, canvas_size=(720, 1280), scaling=0.85):
    """(T, 2, K) -> (T, H, W, 3) uint8 BGR; (B, T, 2, K) -> (B, T, H, W, 3), all frames in one launch."""
    _refuse_capture()
    x, batched = _poses(poses)
    B, T, _, K = x.shape
    H, W = int(canvas_size[0]), int(canvas_size[1])
    out, _, skipped, _ = _launch(x.reshape(B * T, 2, K), clip_instances(B * T, (H, W), scaling), B * T, 1, H, W)
    _report(skipped)
    out = out.reshape(B, T, H, W, 3)
    return out if batched else out[0]


@torch.no_grad()
def render_pose_pair_clip(pred, gt, canvas_size=(720, 1280), scaling=0.85):
    """prediction and ground truth side by side: (T, 2, K) x 2 -> (T, H, W, 3) uint8 BGR (batched like render_pose_clip)."""
    _refuse_capture()
    p, batched = _poses(pred)
    g, _ = _poses(gt)
    if p.shape != g.shape:
        raise ValueError("pred %s and gt %s differ in shape" % (tuple(pred.shape), tuple(gt.shape)))
    B, T, _, K = p.shape
    H, W = int(canvas_size[0]), int(canvas_size[1])
    both = torch.cat([p.reshape(B * T, 2, K), g.reshape(B * T, 2, K)], 0)
    out, _, skipped, _ = _launch(both, pair_instances(B * T, (H, W), scaling), B * T, 2, H, W)
    _report(skipped)
    out = out.reshape(B, T, H, W, 3)
    return out if batched else out[0]


@torch.no_grad()
def render_long_image(poses):
    """draw_pose_frames_in_long_img: every eighth pose of (T, 2, K) in its own 960-px window -> (720, width, 3) uint8 BGR
    ((B, T, 2, K) -> (B, 720, width, 3))."""
    _refuse_capture()
    x, batched = _poses(poses)
    B, T, _, K = x.shape
    width, n_win, rows = long_instances(B, T)
    out, _, skipped, _ = _launch(x.reshape(B * T, 2, K), rows, B, n_win, LONG_H, width)
    _report(skipped)
    return out if batched else out[0]


@torch.no_grad()
def stroke_table(view, poses, gt=None, canvas_size=(720, 1280), scaling=0.85):
    """The prepare pass's stroke records for ``view`` in {'clip', 'pair', 'long'} (poses as for the render functions), in draw
    order, as numpy arrays: image (n,), endpoints (n, 4) = x0 y0 x1 y1, colour (n, 3) BGR, thickness (n,), clip (n, 2) = the
    window [x0, x1) in canvas columns, drawn (n,) bool, bbox (n, 4); plus 'canvas' (H, W)."""
    _refuse_capture()
    x, _ = _poses(poses)
    B, T, _, K = x.shape
    if view == "clip":
        H, W = canvas_size
        flat, rows, n_img, n_inst = x.reshape(B * T, 2, K), clip_instances(B * T, canvas_size, scaling), B * T, 1
    elif view == "pair":
        H, W = canvas_size
        g, _ = _poses(gt)
        flat = torch.cat([x.reshape(B * T, 2, K), g.reshape(B * T, 2, K)], 0)
        rows, n_img, n_inst = pair_instances(B * T, canvas_size, scaling), B * T, 2
    elif view == "long":
        H = LONG_H
        W, n_inst, rows = long_instances(B, T)
        flat, n_img = x.reshape(B * T, 2, K), B
    else:
        raise ValueError("view must be 'clip', 'pair' or 'long'")
    lib = _lib.load()
    if lib.sdt_render_edges(int(K)) == 0:
        raise ValueError("unsupported number of keypoints: %d" % K)
    inst = _table(rows, x.device)
    ws_bytes = lib.sdt_render_workspace_bytes(n_img, n_inst, int(K))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    skipped = torch.empty(1, dtype=torch.int32, device=x.device)
    _lib.check(lib.sdt_render_prepare_f64(_p(flat), flat.shape[0], int(K), _p(inst), n_img, n_inst, int(H), int(W), _p(ws), ws_bytes,
                                          _p(skipped), _stream()))
    rec = ws.view(torch.int32).reshape(-1, 16).cpu().numpy()
    n = rec.shape[0]
    cw = rec[:, 12]
    return {"image": np.arange(n) // (n // n_img), "endpoints": rec[:, 0:4].copy(), "bbox": rec[:, 4:8].copy(),
            "colour": np.stack([cw & 0xff, (cw >> 8) & 0xff, (cw >> 16) & 0xff], 1), "thickness": (cw >> 24) & 0xff,
            "clip": rec[:, 13:15].copy(), "drawn": rec[:, 15] != 0, "skipped": int(skipped.item()), "canvas": (int(H), int(W))}
