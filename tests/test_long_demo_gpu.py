"""The whole-recording demo on the GPU (csrc/long_demo.hip, speechdrivestemplates_amd/long_demo.py, DEMO.LONG_FORM) against
the numpy contract models.

Bars.  The gather is float32 copies: bit-equal to numpy slicing with zero fill.  The blend and the smoother run the models' operations in the
models' order and have no square root: bit-identical.  The report's counts and its flag are equal; its float sums are bit-identical where this
device's float64 square root is correctly rounded on the test's own arguments (the ``sqrt_is_exact`` pattern of tests/test_clip_metrics_gpu.py),
otherwise held to (n + 2) 2^-52 relative, n the number of terms.  Every comparison prints how many values were bit-identical before it asserts.
"""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest
import torch

from conftest import REPO
from speechdrivestemplates_amd import _lib
from speechdrivestemplates_amd import clip_metrics as cm
from speechdrivestemplates_amd import long_demo as ld
from test_long_demo_host import LW, SHAPES, ULP, part_table, window_poses

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMOOTHS = [(1, 0), (2, 2), (8, 3)]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def same_bits(name, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    same = int((bits(got) == bits(want)).sum())
    print("  %-44s %d of %d values bit-identical" % (name, same, got.size))
    assert same == got.size, "%s: %d of %d values differ in bits" % (name, got.size - same, got.size)


@functools.lru_cache(maxsize=None)
def windows_of(shape):
    return window_poses(*shape)


@functools.lru_cache(maxsize=None)
def stitched_model_of(shape):
    F, W, O, K = shape
    return ld.stitch_model(windows_of(shape), O, F)


# -- gather ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [LW, LW + 1, 3 * LW - 5], ids=["Lw", "Lw+1", "3Lw-5"])
def test_gather_is_slicing_with_zero_fill(L):
    rng = np.random.Generator(np.random.PCG64(L))
    audio = rng.standard_normal(L).astype(np.float32)
    F = max(64, L * 15 // 16000)
    _, offsets = ld.window_layout(F, 64, 16)
    offsets = sorted(set(offsets + [0, 1, L - LW, max(0, L - LW) + 7, L - 1]))  # windows that end at, and run past, the end
    offsets = [o for o in offsets if o >= 0]
    want = np.zeros((len(offsets), LW), dtype=np.float32)
    for i, a in enumerate(offsets):
        n = max(0, min(LW, L - a))
        want[i, :n] = audio[a:a + n]
    got = ld.gather_windows(dev(audio), offsets, LW).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    got = ld.gather_windows(dev(audio), torch.tensor(offsets[-2:], dtype=torch.int64, device=DEV), LW).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want[-2:].view(np.int32))
    if L == LW:  # one window that is the recording itself, and a short window length
        assert np.array_equal(ld.gather_windows(dev(audio), [0], LW).cpu().numpy()[0].view(np.int32), audio.view(np.int32))
        assert np.array_equal(ld.gather_windows(dev(audio), [L - 3], 5).cpu().numpy()[0], np.concatenate([audio[-3:], [0.0, 0.0]]).astype(np.float32))


# -- stitch and smooth ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stitch_and_smooth_equal_the_models_bit_for_bit(shape):
    F, W, O, K = shape
    win = windows_of(shape)
    want = stitched_model_of(shape)
    got = ld.stitch(dev(win), O, F)
    same_bits("stitch F=%d W=%d O=%d K=%d" % shape, got.cpu().numpy(), want)
    for m, d in SMOOTHS:
        y = ld.smooth(got, (m, d))
        assert y.data_ptr() != got.data_ptr()
        same_bits("smooth [%d, %d]" % (m, d), y.cpu().numpy(), ld.smooth_model(want, (m, d)))
    same_bits("stitch again (the smoother wrote elsewhere)", got.cpu().numpy(), want)


def test_smooth_clamps_at_both_ends():
    for F, K in ((8, 5), (64, 121), (2, 1), (1, 3)):  # m = 8 reaches past both ends of F = 8 at every frame
        x = windows_of((max(F, 8), max(F, 8), 0, K))[0][:F]
        same_bits("smooth [8, 3] F=%d K=%d" % (F, K), ld.smooth(dev(x), (8, 3)).cpu().numpy(), ld.smooth_model(x, (8, 3)))
    table = np.arange(1.0, 6.0) / 7.0  # an explicit table that is no Savitzky-Golay filter
    x = windows_of((64, 64, 0, 121))[0]
    same_bits("smooth with a given table", ld.smooth(dev(x), table).cpu().numpy(), ld.smooth_model(x, table))


@pytest.mark.parametrize("shape", [(17, 8, 3, 5), (113, 64, 32, 121)], ids=lambda s: "x".join(map(str, s)))
def test_a_nan_stays_in_the_frames_its_window_covers(shape):
    F, W, O, K = shape
    win = windows_of(shape).copy()
    starts, _ = ld.window_layout(F, W, O)
    clean = ld.stitch(dev(win), O, F)
    clean_s = ld.smooth(clean, (2, 2))
    i, local = len(starts) - 2, W - 2  # a frame in the overlap with the last window
    win[i, local] = np.nan
    t = starts[i] + local
    got = ld.stitch(dev(win), O, F)
    got_s = ld.smooth(got, (2, 2))
    g, c = got.cpu().numpy(), clean.cpu().numpy()
    assert np.isnan(g[t]).all()
    others = np.arange(F) != t
    assert np.array_equal(bits(g[others]), bits(c[others]))
    gs, cs = got_s.cpu().numpy(), clean_s.cpu().numpy()
    near = np.abs(np.arange(F) - t) <= 2
    assert np.isnan(gs[near]).all() and np.array_equal(bits(gs[~near]), bits(cs[~near]))
    same_bits("stitch with a NaN frame", g, ld.stitch_model(win, O, F))


# -- report --------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sqrt_is_exact():
    rng = np.random.Generator(np.random.PCG64(11))
    x = np.concatenate([rng.uniform(0, 4, 100000), np.exp(rng.uniform(-30, 30, 100000)), [0.0, 1.0, 2.0, 4.0, 2.0 ** -1040]])
    same = np.array_equal(cm.device_sqrt(dev(x)).cpu().numpy(), np.sqrt(x))
    print("  device sqrt(float64) equals numpy's on %d values: %s" % (x.size, same))
    return same


def sqrt_arguments(win, O, poses):
    """every argument of a square root the report takes on these inputs"""
    out = []
    for x in poses:
        v = x[1:] - x[:-1]
        out.append(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1])
        if x.shape[0] > 3:
            d = ((x[3:] - 3.0 * x[2:-1]) + 3.0 * x[1:-2]) - x[:-3]
            out.append(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    N, W = win.shape[:2]
    F = poses[0].shape[0]
    starts, _ = ld.window_layout(F, W, O)
    for t in range(F):
        idx = ld.covering(t, starts, W)
        for a in range(len(idx)):
            for b in range(a + 1, len(idx)):
                d = win[idx[a], t - starts[idx[a]]] - win[idx[b], t - starts[idx[b]]]
                out.append(d[0] * d[0] + d[1] * d[1])
    x = np.concatenate([o.ravel() for o in out]) if out else np.zeros(0)
    return x[np.isfinite(x)]


def held(name, got, want, exact):
    assert np.array_equal(got[20:], want[20:]), "%s: counts or flags differ: %s vs %s" % (name, got[20:], want[20:])
    same = int((got[:20] == want[:20]).sum())
    print("  %-44s %d of 20 float values bit-identical (sqrt exact on these inputs: %s)" % (name, same, exact))
    if exact:
        assert same == 20, "%s: %d of 20 float values differ in bits" % (name, 20 - same)
        return
    gf, wf = got[:20].view(np.float64), want[:20].view(np.float64)
    n = np.array([want[ld.N_SEAM + p] if g == 4 else want[(ld.N_JERK if g & 1 else ld.N_SPEED) + p] for g in range(5) for p in range(4)])
    assert (np.abs(gf - wf) <= (n + 2) * ULP * np.abs(wf)).all(), "%s: %s" % (name, np.abs(gf - wf) / np.maximum(np.abs(wf), 1e-300))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_report_equals_the_model(shape):
    F, W, O, K = shape
    win, stitched = windows_of(shape), stitched_model_of(shape)
    smoothed = ld.smooth_model(stitched, (2, 2))
    parts = part_table(K)
    for name, sm in (("plain", None), ("smoothed", smoothed)):
        poses = [stitched] + ([] if sm is None else [sm])
        x = sqrt_arguments(win, O, poses)
        exact = sqrt_is_exact() and (x.size == 0 or np.array_equal(cm.device_sqrt(dev(x)).cpu().numpy(), np.sqrt(x)))
        got = ld.report(dev(win), dev(stitched), None if sm is None else dev(sm), O, parts).cpu().numpy()
        held("report %s F=%d W=%d O=%d K=%d" % ((name,) + shape), got, ld.report_model(win, stitched, sm, O, parts), exact)


def test_report_of_identical_windows_and_of_a_nan():
    F, W, O, K = 113, 64, 32, 121
    rng = np.random.Generator(np.random.PCG64(9))
    g = rng.uniform(1.0, 500.0, (F, 2, K))
    starts, _ = ld.window_layout(F, W, O)
    win = np.stack([g[s:s + W] for s in starts])
    stitched = ld.stitch(dev(win), O, F)
    words = ld.report(dev(win), stitched, None, O).cpu().numpy()
    assert words[ld.PAIR_FRAMES] > 0 and words[ld.NONFINITE] == 0 and not words[16:20].any()  # seam is exactly +0.0
    win[1, 5, 0, 100] = np.nan
    stitched = ld.stitch(dev(win), O, F)
    words = ld.report(dev(win), stitched, None, O).cpu().numpy()
    want = ld.report_model(win, stitched.cpu().numpy(), None, O)
    assert words[ld.NONFINITE] == 1 and np.array_equal(words[20:], want[20:])
    f = words[:20].view(np.float64)
    assert np.isnan(f[0]) and np.isnan(f[3]) and np.isfinite(f[1]) and np.isfinite(f[2])


# -- size checks ---------------------------------------------------------------------------------------------------------------------------------
def test_sizes_outside_the_contract_are_refused_before_any_launch():
    lib = _lib.load()
    x = torch.zeros(4 * 8 * 2 * 129, dtype=torch.float64, device=DEV)
    out = torch.zeros(64 * 2 * 129, dtype=torch.float64, device=DEV)
    work = torch.zeros(int(lib.sdt_long_report_workspace_bytes(64)) // 8, dtype=torch.int64, device=DEV)
    parts = torch.zeros(129, dtype=torch.uint8, device=DEV)
    sizes = (C.c_int64 * 4)(1, 1, 0, 0)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    ERR_ARG = -1
    # (N, W, O, F, K): K = 129, O > W / 2, F < W, W < 2, an N that does not match, K = 0
    for N, W, O, F, K in ((1, 8, 0, 8, 129), (1, 8, 5, 8, 1), (1, 8, 0, 7, 1), (1, 1, 0, 1, 1), (3, 8, 0, 16, 1), (1, 8, 0, 8, 0), (1, 8, -1, 8, 1)):
        assert lib.sdt_long_stitch_f64(p(x), N, W, O, F, K, p(out), s) == ERR_ARG, (N, W, O, F, K)
        assert lib.sdt_long_report_f64(p(x), p(out), None, p(parts), sizes, N, W, O, F, K, p(work), p(out), s) == ERR_ARG, (N, W, O, F, K)
    coeffs = (C.c_double * 17)(*([1.0 / 17] * 17))
    for F, K, m in ((8, 129, 1), (8, 0, 1), (0, 1, 1), (8, 1, 0), (8, 1, 9)):
        assert lib.sdt_long_smooth_f64(p(x), F, K, coeffs, m, p(out), s) == ERR_ARG, (F, K, m)
    assert lib.sdt_long_smooth_f64(p(x), 8, 1, coeffs, 1, p(x), s) == ERR_ARG  # in place
    offs = torch.zeros(1, dtype=torch.int64, device=DEV)
    a = torch.zeros(16, dtype=torch.float32, device=DEV)
    for L, n, Lw in ((0, 1, 4), (16, 0, 4), (16, 65536, 4), (16, 1, 0)):
        assert lib.sdt_long_windows_gather_f32(p(a), L, p(offs), n, Lw, p(a), s) == ERR_ARG, (L, n, Lw)
    assert lib.sdt_long_report_workspace_bytes(0) == -1 and lib.sdt_long_report_workspace_bytes(64) == (64 + 1) * 24 * 8
    torch.cuda.synchronize()
    assert not out.any() and not x.any()  # nothing was launched
    # the same sizes from Python
    with pytest.raises(ValueError, match="K = 129"):
        ld.stitch(torch.zeros(1, 8, 2, 129, dtype=torch.float64, device=DEV), 0)
    with pytest.raises(ValueError, match="overlap"):
        ld.stitch(torch.zeros(1, 8, 2, 1, dtype=torch.float64, device=DEV), 5)
    with pytest.raises(ValueError, match="F = 7"):
        ld.stitch(torch.zeros(1, 8, 2, 1, dtype=torch.float64, device=DEV), 0, 7)
    with pytest.raises(ValueError):
        ld.smooth(torch.zeros(8, 2, 129, dtype=torch.float64, device=DEV), (1, 0))
    with pytest.raises(ValueError, match="K = 129"):
        ld.report(torch.zeros(1, 8, 2, 129, dtype=torch.float64, device=DEV), torch.zeros(8, 2, 129, dtype=torch.float64, device=DEV), None, 0,
                  [0] * 129)
    with pytest.raises(TypeError):
        ld.stitch(torch.zeros(1, 8, 2, 1, dtype=torch.float32, device=DEV), 0)


def test_device_functions_refuse_a_capture():
    x = torch.zeros(1, 8, 2, 1, dtype=torch.float64, device=DEV)
    real = torch.cuda.is_current_stream_capturing
    torch.cuda.is_current_stream_capturing = lambda: True  # (no real capture is opened for a call that must refuse before any launch)
    try:
        for call in (lambda: ld.stitch(x, 0), lambda: ld.smooth(x[0], (1, 0)), lambda: ld.report(x, x[0], None, 0, [0]),
                     lambda: ld.gather_windows(torch.zeros(8, device=DEV), [0], 4)):
            with pytest.raises(RuntimeError, match="capture"):
                call()
    finally:
        torch.cuda.is_current_stream_capturing = real


def test_command_line_writes_the_npz(tmp_path, capsys):
    shape = (113, 64, 32, 121)
    win = windows_of(shape)
    np.save(str(tmp_path / "w.npy"), win)
    assert ld.main([str(tmp_path / "w.npy"), str(tmp_path / "out.npz"), "--overlap", "32", "--frames", "113", "--smooth", "2", "2"]) == 0
    assert "113 frames from 3 windows" in capsys.readouterr().out
    with np.load(str(tmp_path / "out.npz")) as z:
        assert set(z.files) == set(ld.OUT_KEYS)
        same_bits("command line: poses_stitched", z["poses_stitched"][0], stitched_model_of(shape))
        same_bits("command line: poses_pred_batch", z["poses_pred_batch"][0], ld.smooth_model(stitched_model_of(shape), (2, 2)))
        assert z["window_starts"].tolist() == ld.window_layout(113, 64, 32)[0] and z["long_report"].shape == (40,)


# -- pipeline ------------------------------------------------------------------------------------------------------------------------------------
PARENT_KEYS = {"poses_pred_batch", "condition_code"}
NEW_KEYS = {"poses_windows", "window_starts", "poses_stitched", "long_report"}


def _pipeline(base_path, *opts):
    """the synthetic voice2pose_sdt_bp set-up of __graft_entry__.make_pipeline, with DEMO / TEST / SYS keys of the test's own, in eval mode"""
    from speechdrivestemplates_amd.config import get_cfg_defaults
    from speechdrivestemplates_amd.core.datasets import gesture_dataset as gd
    from speechdrivestemplates_amd.core.pipelines import get_pipeline
    n_clips = 8
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(REPO, "configs", "voice2pose_sdt_bp.yaml"))
    cfg.merge_from_list(["DATASET.NAME", "SyntheticGestureDataset", "DATASET.SYNTHETIC_CLIPS", n_clips, "SYS.LOG_INTERVAL", 10 ** 9,
                         "DEMO.CODE_INDEX", 3, "TEST.SAVE_NPZ", True, "TEST.SAVE_VIDEO", True, "SYS.VIDEO_FORMAT", ["mp4", "img"]] + list(opts))
    cfg.freeze()
    pipe = get_pipeline(cfg.PIPELINE_TYPE)(cfg)
    pipe.num_train_samples = n_clips
    pipe.test_dataset = gd.SyntheticGestureDataset(cfg=cfg, num_clips=n_clips, split="val")
    torch.manual_seed(5)
    pipe.setup_model(cfg, state_dict=None)
    with torch.no_grad():
        pipe.model.clips_code.normal_(0.0, 0.5)
    pipe.base_path = None if base_path is None else str(base_path)
    return pipe


def _batch(tmp_path, F):
    """a synthetic wav of F frames, read back as the demo dataset reads it"""
    from scipy.io import wavfile
    L = int(F * 16000 / 15)
    rng = np.random.Generator(np.random.PCG64(21 + F))
    path = str(tmp_path / ("speech%d.wav" % F))
    wavfile.write(path, 16000, (rng.standard_normal(L) * 3000).astype(np.int16))
    sr, a = wavfile.read(path)
    assert sr == 16000 and a.shape == (L,)
    audio = torch.from_numpy(a.astype(np.float32) / 32768.0).reshape(1, L)
    stat = {"scale_factor": torch.tensor([1.1]), "mean": torch.from_numpy(rng.standard_normal((1, 242)) * 20.0 + 300.0),
            "std": torch.from_numpy(rng.uniform(2.0, 30.0, (1, 242)))}
    return {"audio": audio, "speaker": ["synthetic"], "clip_index": torch.tensor([0]), "num_frames": torch.tensor([F]), "speaker_stat": stat}


def test_pipeline_with_the_key_off_is_the_single_pass(tmp_path):
    pipe = _pipeline(None)
    res = pipe.demo_step(_batch(tmp_path, 150), 1)
    assert set(res) == PARENT_KEYS
    assert res["poses_pred_batch"].shape == (1, 150, 2, 121) and res["poses_pred_batch"].dtype == torch.float64
    assert res["condition_code"].shape[0] == 1
    assert getattr(pipe, "_long_demo", None) is None and not hasattr(pipe, "_clip")
    pipe.close()


@pytest.fixture(scope="module")
def long_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("long_demo")
    pipe = _pipeline(tmp, "DEMO.LONG_FORM", True, "DEMO.LONG_BATCH", 2, "DEMO.SMOOTH", [2, 2], "DEMO.SEGMENT_FRAMES", 100, "SYS.RENDER_VIDEO", True)
    short = pipe.demo_step(_batch(tmp, 40), 2)  # F = 40 < W: the single pass
    had_runner = getattr(pipe, "_long_demo", None) is not None
    res = pipe.demo_step(_batch(tmp, 150), 1)
    pipe.close()  # (the writer's files are complete)
    return {"pipe": pipe, "res": res, "short": short, "had_runner": had_runner, "base": str(tmp)}


def test_pipeline_long_form_equals_the_models(long_run):
    res = long_run["res"]
    assert set(res) == PARENT_KEYS | NEW_KEYS
    p = res["poses_pred_batch"]
    assert p.shape == (1, 150, 2, 121) and p.dtype == torch.float64 and torch.isfinite(p).all()
    starts, _ = ld.window_layout(150, 64, 16)
    assert res["window_starts"].tolist() == starts == [0, 48, 86]
    win = res["poses_windows"].cpu().numpy()
    assert win.shape == (3, 64, 2, 121) and win.dtype == np.float64
    stitched = ld.stitch_model(win, 16, 150)
    same_bits("pipeline: poses_stitched", res["poses_stitched"].cpu().numpy()[0], stitched)
    same_bits("pipeline: poses_pred_batch", p.cpu().numpy()[0], ld.smooth_model(stitched, (2, 2)))
    words = res["long_report"].numpy()
    want = ld.report_model(win, stitched, ld.smooth_model(stitched, (2, 2)), 16)
    assert np.array_equal(words[20:], want[20:]) and words[ld.NONFINITE] == 0 and words[ld.SMOOTHED] == 1
    assert np.allclose(words[:20].view(np.float64), want[:20].view(np.float64), rtol=1e-12, atol=0)
    code = res["condition_code"]  # one code for the whole recording: row DEMO.CODE_INDEX of the table
    assert code.shape[0] == 1 and torch.equal(code[0], long_run["pipe"].model.clips_code.detach()[3])
    # windows of one recording differ (different audio), and overlap frames of neighbours are close to neither being copied from the other
    assert not np.array_equal(win[0, 48:], win[1, :16])


def test_pipeline_short_input_takes_the_single_pass(long_run):
    assert set(long_run["short"]) == PARENT_KEYS and long_run["short"]["poses_pred_batch"].shape == (1, 40, 2, 121)
    assert not long_run["had_runner"]  # the runner is made by the first long input


def test_pipeline_long_form_writes_the_npz_and_two_video_segments(long_run):
    base = long_run["base"]
    with np.load(os.path.join(base, "results", "epoch0-DEMO-step1.npz")) as z:
        assert NEW_KEYS | PARENT_KEYS <= set(z.files)
        assert z["poses_pred_batch"].shape == (1, 150, 2, 121) and z["poses_windows"].shape == (3, 64, 2, 121)
        assert z["window_starts"].tolist() == [0, 48, 86] and z["long_report"].shape == (40,) and z["poses_stitched"].shape == (1, 150, 2, 121)
    with np.load(os.path.join(base, "results", "epoch0-DEMO-step2.npz")) as z:
        assert not NEW_KEYS & set(z.files)
    vids, imgs = os.path.join(base, "videos"), os.path.join(base, "imgs")
    for part in ("part00", "part01"):
        stem = "epoch0-DEMO-step1-" + part
        assert os.path.exists(os.path.join(imgs, stem + ".jpg"))
        if not os.path.exists(os.path.join(vids, stem + ".mp4")):  # no ffmpeg: the JPEG frames and the audio slice stay
            assert sorted(os.listdir(os.path.join(vids, stem))) == ["%06d.jpg" % i for i in range(75)]
            from scipy.io import wavfile
            sr, a = wavfile.read(os.path.join(vids, stem + ".wav"))
            assert sr == 16000 and a.shape[0] == 80000
    assert not glob.glob(os.path.join(vids, "epoch0-DEMO-step1-part02*")) and not glob.glob(os.path.join(vids, "epoch0-DEMO-step1.*"))
    assert os.path.exists(os.path.join(imgs, "epoch0-DEMO-step2.jpg"))  # the short input keeps the usual names
