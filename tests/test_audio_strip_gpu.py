"""The audio strip on the GPU (csrc/audio_strip.hip through speechdrivestemplates_amd/audio_strip.py): every byte of the
three launches against the numpy contract models, the two public functions against the composition of the models, and the wiring into the
pipeline's videos and long images.  Every comparison prints how many bytes it compared."""
import glob
import io
import os
import sys

import numpy as np
import pytest
import torch

from speechdrivestemplates_amd import audio_strip as st
from test_jpeg_host import parse_avi
from test_sync_metrics_host import click_train, stepped

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bytes(name, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    a, b = got.view(np.uint8).ravel(), want.view(np.uint8).ravel()
    bad = np.flatnonzero(a != b)
    print("%s: %d bytes compared, %d differ" % (name, a.size, bad.size))
    assert bad.size == 0, "%s: first difference at byte %d: %d vs %d" % (name, bad[0], a[bad[0]], b[bad[0]])


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- envelope ------------------------------------------------------------------------------------------------------------------------------------
def envelope_tables(L):
    """column tables over L samples: a mixed one (columns wholly before 0, empty columns, pieces of uneven length, columns wholly past L), one
    column that spans the clip, one sample per column"""
    cuts = sorted({0, L // 3, L // 2, L - 1, L} | {min(L, v) for v in (1, 5, 64, 65, 130)})
    mixed = [-10, -4, 0, 0] + cuts[1:] + [L, L + 3, L + 9]
    return {"mixed": np.array(mixed), "whole": np.array([-5, L + 5]), "single": np.arange(L + 1)}


def envelope_audio(L, bounds):
    """-> {name: (L,) float32}: noise; noise with +inf, -inf and NaN at the first, a middle and the last sample of a column; zeros; a
    negative peak"""
    rng = np.random.Generator(np.random.PCG64(100 + L))
    noise = (rng.standard_normal(L) * 0.3).astype(np.float32)
    noise[rng.integers(0, L, max(1, L // 7))] = 0.0
    noise[rng.integers(0, L, max(1, L // 9))] = -0.0
    bad = noise.copy()
    inside = [(max(a, 0), min(b, L)) for a, b in zip(bounds[:-1], bounds[1:]) if max(a, 0) < min(b, L)]
    a, b = max(inside, key=lambda ab: ab[1] - ab[0])  # the longest column
    bad[a], bad[(a + b) // 2], bad[b - 1] = np.inf, -np.inf, np.nan
    if len(inside) > 1:  # and a column whose only sample is not finite, where there is a second column
        a2, _ = min((ab for ab in inside if ab != (a, b)), key=lambda ab: ab[1] - ab[0])
        bad[a2] = np.nan
    neg = np.abs(noise) * np.float32(0.5)
    neg[L // 2] = -0.875
    return {"noise": noise, "nonfinite": bad, "zeros": np.zeros(L, dtype=np.float32), "negative_peak": neg}


@pytest.mark.parametrize("L", [1, 53, 160, 4001])
def test_envelope_equals_the_model_bit_for_bit(L):
    mel = torch.ones(1, 1, device=DEV)
    for tname, bounds in envelope_tables(L).items():
        for aname, x in envelope_audio(L, bounds).items():
            want = st.envelope_model(x, bounds)
            d = st.device_band(gpu(x), mel, bounds, 64)
            name = "envelope L=%d %s %s" % (L, tname, aname)
            same_bytes(name + ": min/max", d["env"].cpu().numpy(), want["env"])
            same_bytes(name + ": flags", d["flags"].cpu().numpy(), want["flags"])
            stats = d["stats"].cpu().numpy()
            same_bytes(name + ": peak", np.array([stats[0]], dtype=np.int64).astype(np.uint32).view(np.float32), np.array([want["peak"]]))
            assert stats[1] == want["nonfinite"] and stats[0] >> 32 == 0
            if aname == "negative_peak":
                assert want["peak"] == np.float32(0.875)
            if aname == "nonfinite":
                assert want["nonfinite"] >= 1 and (want["flags"] == st.NONFINITE).any()


# ---- raster --------------------------------------------------------------------------------------------------------------------------------------
def raster_mels(n_mels, F):
    rng = np.random.Generator(np.random.PCG64(7 * n_mels + F))
    plain = (rng.standard_normal((n_mels, F)) ** 2 * 10.0 ** rng.uniform(-9, 1, (n_mels, F))).astype(np.float32)
    odd = plain.copy()
    odd.flat[0], odd.flat[odd.size // 2], odd.flat[-1] = np.nan, np.inf, 0.0
    return {"plain": plain, "nan_inf": odd, "zero": np.zeros((n_mels, F), dtype=np.float32)}


TICKS = [([], [5, 5, 17], None),  # an empty list, duplicates, an absent list
         ([-7, 0, 3, 74, 75, 76, 10 ** 6], [74], [0, 1, 2, 3, 4])]  # before 0, around the end of 4001 samples (tick 75 is sample 4000), far past it


@pytest.mark.parametrize("S", [64, 80, 160])
@pytest.mark.parametrize("n_mels", [1, 7, 80])
def test_raster_equals_the_model_byte_for_byte(S, n_mels):
    L = 4001
    x = envelope_audio(L, np.array([0, L]))["nonfinite"]
    tables = {"uniform": st.uniform_bounds(L, 97, 10 ** 6)[0], "mixed": envelope_tables(L)["mixed"]}
    assert 26 % 7 and 16 % 7 and 76 % 7  # 7 bins divide no lane height
    for F in (1, 1 + L // 160):  # F = 1: every column clamps to the one frame
        for mname, mel in raster_mels(n_mels, F).items():
            for tname, bounds in tables.items():
                for marks in TICKS:
                    env = st.envelope_model(x, bounds)
                    want = st.raster_model(env, bounds, mel, S, marks)
                    got = st.device_band(gpu(x), gpu(mel), bounds, S, marks)["band"].cpu().numpy()
                    same_bytes("raster S=%d n_mels=%d F=%d %s %s" % (S, n_mels, F, mname, tname), got, want)
                    if mname == "zero":  # ref = 0: every threshold is fl32(0 * k) = 0 and every finite power is >= 0: all 255 count
                        lane = want[st.lanes(S)[2]:, env["flags"] != st.EMPTY]
                        assert lane.size and (lane == st.colormap()[255]).all()


# ---- compose -------------------------------------------------------------------------------------------------------------------------------------
def compose_cases(W):
    """(Nc, c0, ph): a standing band narrower than the picture (it leaves the band on the right), windows that leave it on the left, on the
    right and on both sides, the playhead at column 0, at W - 1, half outside on the left, absent"""
    return [(W - 7, 0, 0), (W - 7, -3, W - 1 - 3), (3 * W, -5, -1), (3 * W, 3 * W - W // 2, 3 * W - W // 2), (3 * W, W, W + W - 1),
            (3 * W, W + 1, W), (W, 0, -1), (5, -(W // 2), 2)]


@pytest.mark.parametrize("shape", [(1, 16, 40), (3, 16, 41), (2, 33, 64)])
@pytest.mark.parametrize("offset", [0, 1])
def test_compose_equals_the_model_byte_for_byte(shape, offset):
    from speechdrivestemplates_amd import _lib
    n, H, W = shape
    rng = np.random.Generator(np.random.PCG64(n * 100 + W))
    flat = rng.integers(0, 256, n * H * W * 3 + offset, dtype=np.uint8)
    frames_dev = gpu(flat)[offset:].view(n, H, W, 3)  # offset 1: a view whose base is not 16-byte aligned
    frames = flat[offset:].reshape(n, H, W, 3)
    for S in (64, 80):
        for Nc, c0, ph in compose_cases(W):
            band = rng.integers(0, 256, (S, Nc, 3), dtype=np.uint8)
            c0s, phs = [c0 + 2 * i for i in range(n)], [ph if ph < 0 else ph + i for i in range(n)]
            got_dev = st.device_compose(frames_dev, gpu(band), c0s, phs)
            vec = _lib.load().sdt_strip_compose_vectorised(frames_dev.data_ptr(), W, got_dev.data_ptr())
            assert vec == int(W * 3 % 16 == 0 and offset == 0)  # (2, 33, 64) unshifted takes the 16-byte path, every other case the byte path
            got = got_dev.cpu().numpy()
            same_bytes("compose %s offset %d S=%d Nc=%d c0=%d ph=%d %s" % (shape, offset, S, Nc, c0, ph, "vector" if vec else "scalar"), got,
                       st.compose_model(frames, band, c0s, phs))
            assert np.array_equal(got[:, :H], frames)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip():
    T, L = 9, 9601
    rng = np.random.Generator(np.random.PCG64(9))
    x, _ = click_train(L, (2000, 6000))
    pred, gt = stepped([1, 1, 4, 1, 1, 5, 1, 1]), stepped([1, 3, 1, 1, 1, 1, 6, 1])
    mel = (rng.standard_normal((7, 1 + L // 160)) ** 2).astype(np.float32)
    frames = rng.integers(0, 256, (T, 48, 64, 3), dtype=np.uint8)
    marks = st.clip_marks(gpu(x), gpu(pred), gpu(gt), parts=[0])
    assert len(marks[0]) == 2 and len(marks[1]) >= 1 and len(marks[2]) >= 1  # two clicks; the speed peaks
    return {"T": T, "L": L, "x": x, "mel": mel, "frames": frames, "marks": marks}


@pytest.mark.parametrize("span_s", [4.3, 0.25])  # 9601 samples: a standing band; a scrolling one (4000 samples in view)
def test_strip_for_clip_equals_the_composed_models(clip, span_s):
    x, mel, frames, marks = clip["x"], clip["mel"], clip["frames"], clip["marks"]
    bounds, c0, ph = st.clip_layout(clip["T"], 64, clip["L"], span_s)
    assert (c0 != 0).any() == (span_s < 0.6)
    want = st.compose_model(frames, st.raster_model(st.envelope_model(x, bounds), bounds, mel, 64, marks), c0, ph)
    got = [st.strip_for_clip(gpu(frames), gpu(x), gpu(mel), marks, height=64, span_s=span_s).cpu().numpy() for _ in range(2)]
    same_bytes("strip_for_clip span %.2f" % span_s, got[0], want)
    same_bytes("strip_for_clip span %.2f, second call" % span_s, got[1], got[0])
    assert (want[:, 48:] == st.PLAYHEAD).all(axis=3).any() and (want[:, 48:] == st.MARKS[0]).all(axis=3).any()


def test_strip_for_long_image_equals_the_composed_models(clip):
    from speechdrivestemplates_amd.render import long_image_layout
    x, mel, marks, T = clip["x"], clip["mel"], clip["marks"], clip["T"]
    width = long_image_layout(T)[0]
    image = np.random.Generator(np.random.PCG64(4)).integers(0, 256, (720, width, 3), dtype=np.uint8)
    bounds = st.long_image_bounds(T, clip["L"])
    want = st.compose_model(image[None], st.raster_model(st.envelope_model(x, bounds), bounds, mel, 80, marks), [0], [-1])[0]
    got = [st.strip_for_long_image(gpu(image), gpu(x), gpu(mel), T, marks, height=80).cpu().numpy() for _ in range(2)]
    same_bytes("strip_for_long_image", got[0], want)
    same_bytes("strip_for_long_image, second call", got[1], got[0])
    assert got[0].shape == (800, width, 3)  # (no playhead: the model composed it with ph = -1)
    with pytest.raises(ValueError, match="columns wide"):
        st.strip_for_long_image(gpu(image[:, :-1]), gpu(x), gpu(mel), T)


def test_a_call_under_capture_raises_before_any_launch(clip):
    frames, x, mel = gpu(clip["frames"]), gpu(clip["x"]), gpu(clip["mel"])
    real = torch.cuda.is_current_stream_capturing
    torch.cuda.is_current_stream_capturing = lambda: True  # (no real capture is opened for a call that must refuse before any launch)
    try:
        for call in (lambda: st.strip_for_clip(frames, x, mel), lambda: st.strip_for_long_image(frames[0], x, mel, 9),
                     lambda: st.device_compose(frames, frames[0], [0] * 9, [0] * 9)):
            with pytest.raises(RuntimeError, match="capture"):
                call()
    finally:
        torch.cuda.is_current_stream_capturing = real


# ---- wiring --------------------------------------------------------------------------------------------------------------------------------------
CANVAS, HEIGHT, FRAMES = (144, 256), 64, 40


def _pipeline(base_path, *opts):
    """the synthetic voice2pose_sdt_bp set-up of __graft_entry__.make_pipeline with videos as AVI and long images, in eval mode"""
    from speechdrivestemplates_amd.config import get_cfg_defaults
    from speechdrivestemplates_amd.core.datasets import gesture_dataset as gd
    from speechdrivestemplates_amd.core.pipelines import get_pipeline
    n_clips = 8
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(REPO, "configs", "voice2pose_sdt_bp.yaml"))
    cfg.merge_from_list(["DATASET.NAME", "SyntheticGestureDataset", "DATASET.SYNTHETIC_CLIPS", n_clips, "SYS.LOG_INTERVAL", 10 ** 9,
                         "DEMO.CODE_INDEX", 3, "TEST.SAVE_NPZ", False, "TEST.SAVE_VIDEO", True, "SYS.VIDEO_FORMAT", ["avi", "img"],
                         "SYS.RENDER_VIDEO", True, "SYS.CANVAS_SIZE", CANVAS] + list(opts))
    cfg.freeze()
    pipe = get_pipeline(cfg.PIPELINE_TYPE)(cfg)
    pipe.num_train_samples = n_clips
    pipe.test_dataset = gd.SyntheticGestureDataset(cfg=cfg, num_clips=n_clips, split="val")
    torch.manual_seed(5)
    pipe.setup_model(cfg, state_dict=None)
    with torch.no_grad():
        pipe.model.clips_code.normal_(0.0, 0.5)
    pipe.base_path = str(base_path)
    return pipe


def _inputs():
    rng = np.random.Generator(np.random.PCG64(77))
    L = FRAMES * 16000 // 15
    audio = torch.from_numpy((rng.standard_normal((1, L)) * 0.1).astype(np.float32))
    stat = {"scale_factor": torch.tensor([1.1]), "mean": torch.from_numpy(rng.standard_normal((1, 242)) * 20.0 + 300.0),
            "std": torch.from_numpy(rng.uniform(2.0, 30.0, (1, 242)))}
    batch = {"audio": audio, "speaker": ["synthetic"], "clip_index": torch.tensor([0]), "num_frames": torch.tensor([FRAMES]), "speaker_stat": stat}
    pose = lambda seed: torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal((FRAMES, 2, 121)).cumsum(0) * 4.0).to(DEV)  # noqa: E731
    return batch, pose(1), pose(2)


def _run(pipe):
    batch, pred, gt = _inputs()
    pipe.write_pair_video("TEST", pred, gt, 1, 0, audio=batch["audio"])
    res = pipe.demo_step(batch, 2)
    pipe.close()
    return batch, pred, gt, res["poses_pred_batch"][0]


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_pipeline_with_the_key_writes_taller_videos_and_a_taller_long_image(tmp_path):
    from PIL import Image
    pipe = _pipeline(tmp_path, "SYS.AUDIO_STRIP.ENABLE", True, "SYS.AUDIO_STRIP.HEIGHT", HEIGHT)
    _run(pipe)
    for stem in ("epoch0-TEST-step1", "epoch0-DEMO-step2"):
        info = parse_avi(_read(os.path.join(str(tmp_path), "videos", stem + ".avi")))
        assert len(info["frames"]) == FRAMES and info["avih"][8:10] == (CANVAS[1], CANVAS[0] + HEIGHT)
        for jpg in (info["frames"][0], info["frames"][-1]):
            assert Image.open(io.BytesIO(jpg)).size == (CANVAS[1], CANVAS[0] + HEIGHT)
    first = np.asarray(Image.open(io.BytesIO(info["frames"][0])))[CANVAS[0]:]
    assert first[:, :2].mean() > 150  # frame 0 of a standing band: the playhead, white, at the left edge
    img = Image.open(os.path.join(str(tmp_path), "imgs", "epoch0-DEMO-step2.jpg"))
    assert img.size[1] == 720 + HEIGHT
    assert len(glob.glob(os.path.join(str(tmp_path), "videos", "*.avi"))) == 2


def test_pipeline_without_the_key_writes_the_parents_bytes_and_imports_nothing(tmp_path):
    import speechdrivestemplates_amd as pkg
    from speechdrivestemplates_amd import render
    from speechdrivestemplates_amd.video import VideoWriter
    name = "speechdrivestemplates_amd.audio_strip"
    module = sys.modules.pop(name)
    delattr(pkg, "audio_strip")
    try:
        pipe = _pipeline(tmp_path / "off")
        assert pipe.strip_opts is None
        batch, pred, gt, demo_pred = _run(pipe)
        assert name not in sys.modules and not hasattr(pkg, "audio_strip")
    finally:
        sys.modules[name] = module
        pkg.audio_strip = module
    # the parent's write_pair_video / write_demo_video, by hand: the renderer's pictures straight into the writer
    cfg, base = pipe.cfg, str(tmp_path / "plain")
    writer = VideoWriter(cfg)
    writer.save_video(cfg, "TEST", render.render_pose_pair_clip(pred, gt, CANVAS, cfg.SYS.VISUALIZATION_SCALING), 1, 0, None,
                      audio=batch["audio"][0], writer=None, base_path=base)
    writer.save_video(cfg, "DEMO", render.render_pose_clip(demo_pred, CANVAS, cfg.SYS.VISUALIZATION_SCALING), 2, 0,
                      long_img=render.render_long_image(demo_pred), audio=batch["audio"][0], base_path=base)
    writer.close()
    files = ["videos/epoch0-TEST-step1.avi", "videos/epoch0-DEMO-step2.avi", "imgs/epoch0-DEMO-step2.jpg"]
    for f in files:
        a, b = _read(os.path.join(str(tmp_path / "off"), f)), _read(os.path.join(base, f))
        print("%s: %d bytes compared" % (f, len(a)))
        assert a == b
    info = parse_avi(_read(os.path.join(base, files[0])))
    assert info["avih"][8:10] == (CANVAS[1], CANVAS[0])
