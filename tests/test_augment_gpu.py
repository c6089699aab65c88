"""The audio augmentation on the GPU (csrc/augment.hip, speechdrivestemplates_amd/augment.py, TRAIN.AUGMENT) against the
numpy contract models.

Bars.  The records' integers are equal; ``ss`` runs the model's additions in the model's order and has no square root: bit-identical.  The
audio is bit-identical to ``audio_model`` where this device's float64 square root is correctly rounded on the test's own arguments ss / L (the
``sqrt_is_exact`` pattern of tests/test_clip_metrics_gpu.py); otherwise sigma may differ in its last bit and every sample is held to one
float32 ulp.  The mel masks write zeros and touch nothing else: bit-identical.  Every comparison prints how many values were bit-identical
before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

from speechdrivestemplates_amd import augment as A
from speechdrivestemplates_amd import clip_metrics as cm
from test_augment_host import ALL_ON, L_CLIP, bits32

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1), (1, 2), (1, 3), (3, 255), (3, 257), (2, 4099), (1, L_CLIP)]
CLIPS = [0, 1 << 31, (1 << 32) + 5]  # (the low 32 bits count)
STEPS = [0, 1, (1 << 32) - 1]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def dev(x):
    return torch.from_numpy(np.array(x, copy=True)).to(DEV)  # (a copy: the shared inputs are read-only arrays)


def i64(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64, device=DEV)


def case_of(shape):
    """-> (clip indices, step) of a shape: the three indices and the three steps take turns"""
    k = SHAPES.index(shape) if shape in SHAPES else 0
    B = shape[0]
    return [CLIPS[(k + b) % 3] for b in range(B)], STEPS[k % 3]


@functools.lru_cache(maxsize=None)
def audio_of(shape):
    x = (0.1 * np.random.Generator(np.random.PCG64([41, shape[0], shape[1]])).standard_normal(shape)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def model_of(shape):
    """audio_model with every augmentation on, computed once per shape"""
    clips, step = case_of(shape)
    y, rec = A.audio_model(audio_of(shape), clips, step, ALL_ON)
    y.setflags(write=False)
    rec.setflags(write=False)
    return y, rec


@functools.lru_cache(maxsize=None)
def sqrt_is_exact():
    rng = np.random.Generator(np.random.PCG64(11))
    x = np.concatenate([rng.uniform(0, 4, 100000), np.exp(rng.uniform(-30, 30, 100000)), [0.0, 1.0, 2.0, 4.0, 2.0 ** -1040]])
    same = np.array_equal(cm.device_sqrt(dev(x)).cpu().numpy(), np.sqrt(x))
    print("  device sqrt(float64) equals numpy's on %d values: %s" % (x.size, same))
    return same


def exact_on(rec, L):
    """is the device's square root correctly rounded on ss / L of these records (the argument of every root the kernels take)"""
    ss = np.ascontiguousarray(rec[:, A.SS]).view(np.float64)
    x = ss[np.isfinite(ss)] / np.float64(L)
    return sqrt_is_exact() and (x.size == 0 or np.array_equal(cm.device_sqrt(dev(x)).cpu().numpy(), np.sqrt(x)))


def same_records(name, got, want, exact):
    ints = [c for c in range(A.REC_COLS) if c not in (A.SIGMA, A.SS)]
    assert np.array_equal(got[:, ints], want[:, ints]), "%s: integer words differ\n%s\n%s" % (name, got[:, :8], want[:, :8])
    same = int((got[:, A.SS] == want[:, A.SS]).sum())
    print("  %-44s %d of %d ss bit-identical" % (name, same, got.shape[0]))
    assert same == got.shape[0], "%s: ss differs in bits" % name
    gs, ws = (np.ascontiguousarray(r[:, A.SIGMA]).view(np.float64) for r in (got, want))
    same = int((got[:, A.SIGMA] == want[:, A.SIGMA]).sum())
    print("  %-44s %d of %d sigma bit-identical (sqrt exact on these inputs: %s)" % (name, same, got.shape[0], exact))
    if exact:
        assert same == got.shape[0], "%s: sigma differs in bits" % name
    else:
        ok = (np.isnan(gs) & np.isnan(ws)) | (np.abs(gs - ws) <= 2.0 ** -51 * np.abs(ws))
        assert ok.all(), "%s: sigma off by more than two ulp" % name


def same_audio(name, got, want, exact):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (name, got.shape, want.shape, got.dtype)
    same = int((bits32(got) == bits32(want)).sum())
    print("  %-44s %d of %d samples bit-identical (sqrt exact on these inputs: %s)" % (name, same, got.size, exact))
    if exact:
        assert same == got.size, "%s: %d of %d samples differ in bits" % (name, got.size - same, got.size)
        return
    with np.errstate(all="ignore"):
        ok = (bits32(got) == bits32(want)) | (np.isnan(got) & np.isnan(want)) | (np.abs(got - want) <= np.spacing(np.abs(want)))
    assert ok.all(), "%s: %d samples off by more than one float32 ulp" % (name, int((~ok).sum()))


def run(x, clips, step, opts, **kw):
    y, rec = A.augment_audio(dev(x), i64(clips), i64([step]), opts, **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy(), rec.cpu().numpy()


# -- records and audio ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_records_and_audio_equal_the_model(shape):
    clips, step = case_of(shape)
    x = audio_of(shape)
    want, want_rec = model_of(shape)
    ss = A.sumsq(dev(x)).cpu().numpy()
    same = int((ss.view(np.int64) == A.sumsq_model(x).view(np.int64)).sum())
    print("  %-44s %d of %d sums of squares bit-identical" % ("sumsq %dx%d" % shape, same, ss.size))
    assert same == ss.size
    got, rec = run(x, clips, step, ALL_ON)
    exact = exact_on(want_rec, shape[1])
    same_records("records %dx%d clips %s step %d" % (shape + (clips, step)), rec, want_rec, exact)
    same_audio("audio %dx%d" % shape, got, want, exact)
    assert np.all(rec[:, A.NONFINITE] == 0) and np.isfinite(got).all()


def test_the_parameters_vary_and_every_branch_is_taken():
    """over a few steps of the (3, 257) case: both signs of the shift, both polarities, noise on and off -- and still the model's bits"""
    x = audio_of((3, 257))
    seen = {"sign": set(), "pol": set(), "noise": set()}
    for step in (2, 3, 4, 5):
        want, want_rec = A.audio_model(x, CLIPS, step, ALL_ON)
        got, rec = run(x, CLIPS, step, ALL_ON)
        exact = exact_on(want_rec, 257)
        same_records("records step %d" % step, rec, want_rec, exact)
        same_audio("audio step %d" % step, got, want, exact)
        seen["sign"].update(int(v) for v in np.sign(rec[:, A.SHIFT]))
        seen["pol"].update(int(v) for v in rec[:, A.POLARITY])
        seen["noise"].update(int(v) for v in rec[:, A.NOISE_ON])
    assert {-1, 1} <= seen["sign"] and seen["pol"] == {0, 1} and seen["noise"] == {0, 1}, seen


@pytest.mark.parametrize("shape", [(3, 3), (3, 257)], ids=["3x3", "3x257"])
def test_a_shift_past_the_clip_leaves_noise_on_zeros(shape):
    opts = A.options(**dict(ALL_ON, shift=1000, noise_prob=1.0))
    x = audio_of(shape)
    whole = 0
    for step in (0, 1, 2):
        want, want_rec = A.audio_model(x, CLIPS, step, opts)
        got, rec = run(x, CLIPS, step, opts)
        exact = exact_on(want_rec, shape[1])
        same_records("records S >= L step %d" % step, rec, want_rec, exact)
        same_audio("audio S >= L step %d" % step, got, want, exact)
        whole += int((np.abs(rec[:, A.SHIFT]) >= shape[1]).sum())
    assert whole >= 1  # some row lost every sample of its own
    quiet = A.options(shift=1000, seed=9)  # no noise: such a row is zeros
    got, rec = run(x, CLIPS, 0, quiet)
    want, want_rec = A.audio_model(x, CLIPS, 0, quiet)
    same_audio("audio S >= L, no noise", got, want, True)
    assert np.array_equal(rec, want_rec)


def test_a_silent_clip_stays_silent():
    x = audio_of((3, 257)).copy()
    x[1] = 0.0
    opts = A.options(**dict(ALL_ON, noise_prob=1.0))
    got, rec = run(x, CLIPS, 1, opts)
    want, want_rec = A.audio_model(x, CLIPS, 1, opts)
    exact = exact_on(want_rec, 257)
    same_records("records with a silent clip", rec, want_rec, exact)
    same_audio("audio with a silent clip", got, want, exact)
    f = np.ascontiguousarray(rec[1]).view(np.float64)
    assert rec[1, A.NOISE_ON] == 1 and f[A.SS] == 0.0 and f[A.SIGMA] == 0.0 and not np.isnan(got).any() and np.all(got[1] == 0.0)


def test_a_nan_stays_in_its_clip_and_sets_its_flag():
    x = audio_of((3, 257)).copy()
    opts = A.options(**dict(ALL_ON, noise_prob=1.0))
    clean, clean_rec = run(x, CLIPS, 1, opts)
    x[1, 200] = np.nan
    got, rec = run(x, CLIPS, 1, opts)
    assert list(rec[:, A.NONFINITE]) == [0, 1, 0] and list(clean_rec[:, A.NONFINITE]) == [0, 0, 0]
    others = [0, 2]
    same = int((bits32(got[others]) == bits32(clean[others])).sum())
    print("  %-44s %d of %d samples of the other rows bit-identical" % ("a NaN in row 1", same, 2 * 257))
    assert same == 2 * 257 and np.array_equal(rec[others], clean_rec[others])
    assert np.isnan(got[1]).all()  # the noise is on: sigma is NaN
    want, want_rec = A.audio_model(x, CLIPS, 1, opts)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(rec[:, :5], want_rec[:, :5])
    x[1, 200] = np.inf
    got, rec = run(x, CLIPS, 1, opts)
    assert list(rec[:, A.NONFINITE]) == [0, 1, 0] and np.array_equal(bits32(got[others]), bits32(clean[others]))


@pytest.mark.parametrize("offset", [0, 1, 2, 3], ids=lambda o: "offset%d" % o)
def test_guard_bands_around_the_output_stay_untouched(offset):
    """the output buffer starts ``offset`` floats past a 16-byte boundary: heads of 0 to 3 elements, rows of every alignment"""
    shape = (3, 257)
    clips, step = case_of(shape)
    want, want_rec = model_of(shape)
    guard, n = 64, 3 * 257
    sentinel = np.float32(-7.5e33)
    buf = torch.full((guard + offset + n + guard,), float(sentinel), dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[guard + offset:guard + offset + n].view(3, 257)
    y, rec = A.augment_audio(dev(audio_of(shape)), i64(clips), i64([step]), ALL_ON, out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert np.all(bits32(host[:guard + offset]) == bits32(sentinel)) and np.all(bits32(host[guard + offset + n:]) == bits32(sentinel))
    same_audio("audio into a view at offset %d" % offset, host[guard + offset:guard + offset + n].reshape(3, 257), want,
               exact_on(want_rec, 257))
    with pytest.raises(RuntimeError, match="never runs in place"):
        xin = dev(audio_of(shape))
        A.augment_audio(xin, i64(clips), i64([step]), ALL_ON, out=xin)


def test_neutral_options_return_the_input_bits():
    x = audio_of((2, 4099)).copy()
    x[0, :4] = [0.0, -0.0, np.float32(1e-40), -np.float32(3e38)]
    got, rec = run(x, [3, 4], 5, A.options())
    same = int((bits32(got) == bits32(x)).sum())
    print("  %-44s %d of %d samples bit-identical" % ("neutral options", same, x.size))
    assert same == x.size
    assert np.array_equal(rec, A.audio_model(x, [3, 4], 5, A.options())[1])


# -- mel masks -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 7, 427], ids=lambda f: "F%d" % f)
@pytest.mark.parametrize("n", [0, 4], ids=lambda n: "n%d" % n)
def test_mel_masks_equal_the_model(F, n):
    rng = np.random.Generator(np.random.PCG64([F, n]))
    mel = rng.uniform(0.5, 2.0, (3, 80, F)).astype(np.float32)
    mel[rng.uniform(size=mel.shape) < 0.05] = np.nan  # outside the rectangles a NaN keeps its bits
    mel[0, 0, 0] = -0.0
    opts = A.options(seed=ALL_ON['seed'], freq_masks=(n, 40), time_masks=(n, 100))
    want, want_rec = A.mel_mask_model(mel, CLIPS, STEPS[2], opts)
    t = dev(mel)
    rec = A.mel_mask(t, i64(CLIPS), i64([STEPS[2]]), opts).cpu().numpy()
    got = t.cpu().numpy()
    same = int((bits32(got) == bits32(want)).sum())
    print("  %-44s %d of %d elements bit-identical, %d zeroed" % ("mel mask F=%d n=%d" % (F, n), same, got.size, int((bits32(got) != bits32(mel)).sum())))
    assert same == got.size and np.array_equal(rec, want_rec)
    if n == 0:
        assert np.array_equal(bits32(got), bits32(mel))
    else:
        assert (bits32(got) != bits32(mel)).any()


# -- graph ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_call_follows_the_step_tensor():
    shape = (3, 4099)
    x, clips = dev(audio_of(shape)), i64(CLIPS)
    mel_src = dev(np.random.Generator(np.random.PCG64(8)).uniform(0.5, 2.0, (3, 80, 26)).astype(np.float32))
    aug = A.Augmenter(ALL_ON, DEV)
    steps = [3, (1 << 32) - 1, 77]
    eager = []
    for s in steps:  # (these eager calls also allocate the augmenter's buffers: the capture and the replays allocate none of them)
        y = aug.audio(x, clips, i64([s]))
        m = aug.mel_masks(mel_src.clone(), clips, i64([s]))
        eager.append((y.cpu().numpy(), m.cpu().numpy(), aug.record.cpu().numpy()))
    assert not np.array_equal(eager[0][0], eager[1][0]) and not np.array_equal(eager[0][2], eager[2][2])
    bufs = {k: [t.data_ptr() for t in v] for k, v in aug._bufs.items()}
    step_t = i64([0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y_static = aug.audio(x, clips, step_t)
        m_static = aug.mel_masks(mel_src.clone(), clips, step_t)
    assert {k: [t.data_ptr() for t in v] for k, v in aug._bufs.items()} == bufs
    for s, (y, m, rec) in zip(steps, eager):
        step_t.copy_(i64([s]))
        g.replay()
        torch.cuda.synchronize()
        got_y, got_m, got_rec = y_static.cpu().numpy(), m_static.cpu().numpy(), aug.record.cpu().numpy()
        same = int((bits32(got_y) == bits32(y)).sum()) + int((bits32(got_m) == bits32(m)).sum())
        print("  %-44s %d of %d values bit-identical" % ("replay at step %d" % s, same, y.size + m.size))
        assert same == y.size + m.size and np.array_equal(got_rec, rec)


# -- pipeline ------------------------------------------------------------------------------------------------------------------------------------
KEYS = ["TRAIN.AUGMENT.SEED", 1234, "TRAIN.AUGMENT.GAIN_DB", 6.0, "TRAIN.AUGMENT.NOISE_SNR_DB", [5.0, 30.0], "TRAIN.AUGMENT.SHIFT_MS", 50.0,
        "TRAIN.AUGMENT.POLARITY", True, "TRAIN.AUGMENT.MEL_FREQ_MASKS", [2, 15], "TRAIN.AUGMENT.MEL_TIME_MASKS", [2, 40]]
ON, OFF = ["TRAIN.AUGMENT.ENABLE", True] + KEYS, ["TRAIN.AUGMENT.ENABLE", False] + KEYS
GLOBAL_STEPS = (1, 2)


def _bits(t):
    return t.detach().float().cpu().numpy().view(np.int32)


def _eval_prediction(pipe, batch):
    code = torch.zeros(2, pipe.cfg.VOICE2POSE.GENERATOR.CLIP_CODE.DIMENSION, device=DEV)
    pipe.model.eval()
    with torch.no_grad():
        out = pipe.model(batch, pipe.train_dataset, return_loss=False, condition_code=code)['poses_pred_batch']
    pipe.model.train()
    torch.cuda.synchronize()
    return _bits(out)


def _manual_steps(pipe, with_step):
    from test_optim_guard_gpu import _batch
    out = []
    for gs in GLOBAL_STEPS:
        batch = _batch(gs, b=2)
        if with_step:
            batch['aug_step'] = torch.tensor([gs], dtype=torch.int64)
        losses, _ = pipe.forward_backward(batch)
        pipe.optimizer_updates(losses)
        torch.cuda.synchronize()
        out.append(_bits(losses['G_loss']))
    return out


def test_pipeline_with_the_key_on_and_off():
    from test_optim_guard_gpu import _batch, _pipe
    on, off, plain = _pipe(ON), _pipe(OFF), _pipe()
    assert on.model.aug_opts is not None and on.model.aug_opts['shift'] == 800 and off.model.aug_opts is None and plain.model.aug_opts is None
    # evaluation hears clean audio: the same bits with the key on and off, and no Augmenter is built for it
    probe = _batch(0, b=2)
    assert np.array_equal(_eval_prediction(on, probe), _eval_prediction(off, probe)) and on.model._augmenters == {}
    with pytest.raises(KeyError, match="aug_step"):
        on.model(_batch(0, b=2), on.train_dataset)
    l_on, l_off, l_plain = _manual_steps(on, True), _manual_steps(off, False), _manual_steps(plain, False)
    print("  G_loss on %s off %s" % ([x.view(np.float32) for x in l_on], [x.view(np.float32) for x in l_off]))
    assert all(np.array_equal(a, b) for a, b in zip(l_off, l_plain)), "the key off is not the step as it was"
    assert all(not np.array_equal(a, b) for a, b in zip(l_on, l_off)), "the augmentation did not reach the loss"
    assert off.model._augmenters == {} and plain.model._augmenters == {} and len(on.model._augmenters) == 1
    rec = next(iter(on.model._augmenters.values())).record.cpu().numpy()
    assert rec.shape == (2, A.REC_COLS) and np.all(rec[:, A.NF] == 2) and np.all(rec[:, A.NT] == 2) and np.all(np.abs(rec[:, A.SHIFT]) <= 800)
    for p in (off, plain):
        p.close()
    # the same seed again, this time through train_step, which puts the step into the batch: the same G_loss bits
    twin = _pipe(ON)
    l_twin = []
    for gs in GLOBAL_STEPS:
        batch = _batch(gs, b=2)
        twin.train_step(batch, 1, gs, 1)
        torch.cuda.synchronize()
        assert 'aug_step' not in batch
        l_twin.append(_bits(twin.last_losses['G_loss']))
    same = sum(int(np.array_equal(a, b)) for a, b in zip(l_on, l_twin))
    print("  %-44s %d of %d G_loss values bit-identical" % ("two runs from the same seed", same, len(l_on)))
    assert same == len(l_on)
    on.close()
    twin.close()
