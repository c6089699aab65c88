"""Per-tensor histograms on the GPU (csrc/tensor_hist.hip, tensor_hist.py) against the numpy contract model
``tensor_hist.model_histograms``: counts and tallies equal, sum and sum of squares bit-identical, min and max equal by value -- on edge-sized
segments with poisoned padding, under bucket contention, with a scale, on a real FlatAdam, and through the Trainer into the event file
(eager and with the step replayed from a hipGraph)."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401
from test_tensor_hist_host import hist_values

from speechdrivestemplates_amd import tb_events
from speechdrivestemplates_amd import tensor_hist as th

pytestmark = pytest.mark.gpu

DEV = "cuda"
C = th.HIST_CHUNK
SEGMENT_SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 257, C - 1, C, C + 1, 2 * C + 17]


def f64_bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_matches_model(got, ref, what=""):
    """got: device (counts, tallies, stats); ref: the model's"""
    counts, tallies, stats = (t.cpu().numpy() for t in got)
    rc, rt, rs = ref
    assert counts.dtype == np.int64 and tallies.dtype == np.int64 and stats.dtype == np.float64
    assert np.array_equal(counts, rc), "%s: counts differ in %d bins" % (what, int((counts != rc).sum()))
    assert np.array_equal(tallies, rt), "%s: tallies %s vs %s" % (what, tallies.tolist(), rt.tolist())
    assert np.array_equal(counts.sum(1), tallies[:, 0]), what
    assert np.array_equal(f64_bits(stats[:, 2:]), f64_bits(rs[:, 2:])), "%s: sums differ: %s vs %s" % (what, stats[:, 2:], rs[:, 2:])
    assert np.array_equal(stats[:, :2], rs[:, :2]), "%s: min / max %s vs %s" % (what, stats[:, :2], rs[:, :2])


def layout(sizes):
    offsets, total = [], 0
    for n in sizes:
        offsets.append(total)
        total += (n + 3) // 4 * 4  # FlatAdam's alignment
    return offsets, total


@pytest.fixture(scope="module")
def segments():
    """(values per segment, offsets, total): shared by the tests, never changed"""
    values = np.random.Generator(np.random.PCG64(11)).permutation(hist_values(100000, 5))
    assert values.size >= sum(SEGMENT_SIZES)
    offsets, total = layout(SEGMENT_SIZES)
    parts, pos = [], 0
    for n in SEGMENT_SIZES:
        parts.append(values[pos:pos + n])
        pos += n
    return parts, offsets, total


def flat_of(segments, pad):
    parts, offsets, total = segments
    flat = np.full(total + 8, pad, dtype=np.float32)  # (padding after the last segment too)
    for p, off in zip(parts, offsets):
        flat[off:off + p.size] = p
    return flat


@pytest.mark.parametrize("pad", [7.0, float("nan")], ids=["pad7", "padnan"])
def test_segments_match_the_model_and_padding_never_shows(segments, pad):
    flat = flat_of(segments, pad)
    offsets = segments[1]
    ref = th.model_histograms(flat, offsets, SEGMENT_SIZES)
    got = th.flat_histograms(torch.from_numpy(flat).to(DEV), offsets, SEGMENT_SIZES)
    assert_matches_model(got, ref, "pad %r" % pad)
    tallies = got[1].cpu().numpy()
    assert tallies[:, 0].tolist() == SEGMENT_SIZES and not tallies[:, 1:].any()  # no 7.0 and no NaN of the padding was counted
    # the same segments packed without padding values in between give the same rows
    alone = th.model_histograms(np.concatenate(segments[0]), np.cumsum([0] + SEGMENT_SIZES[:-1]).tolist(), SEGMENT_SIZES)
    assert np.array_equal(alone[0], ref[0]) and np.array_equal(f64_bits(alone[2]), f64_bits(ref[2]))


def test_contention_and_nonfinite_segments():
    n = 100000
    equal = np.full(n, 0.0123, np.float32)
    e = th.BUCKET_EDGES[900]
    two = np.where(np.arange(n) % 2 == 0, np.float32(e * 0.99), np.float32(e * 1.01)).astype(np.float32)
    nans = np.full(1000, np.nan, np.float32)
    infs = np.where(np.arange(1000) % 3 == 0, -np.inf, np.inf).astype(np.float32)
    mixed = np.concatenate([equal[:5000], nans[:777], infs[:333], two[:5001]])
    mixed = np.random.Generator(np.random.PCG64(2)).permutation(mixed)
    parts = [equal, two, nans, infs, mixed]
    sizes = [p.size for p in parts]
    offsets, total = layout(sizes)
    flat = np.zeros(total, np.float32)
    for p, off in zip(parts, offsets):
        flat[off:off + p.size] = p
    ref = th.model_histograms(flat, offsets, sizes)
    got = th.flat_histograms(torch.from_numpy(flat).to(DEV), offsets, sizes)
    assert_matches_model(got, ref, "contention")
    counts, tallies, stats = (t.cpu().numpy() for t in got)
    assert counts[0].max() == n and (counts[0] > 0).sum() == 1
    assert sorted(counts[1][counts[1] > 0].tolist()) == [n // 2, n // 2] and counts[1, 899] == counts[1, 900] == n // 2
    assert tallies.tolist() == [[n, 0, 0], [n, 0, 0], [0, 1000, 0], [0, 0, 1000], [10001, 777, 333]]
    for s in (2, 3):  # no finite element: empty moments, no count
        assert not counts[s].any()
        assert stats[s, 0] == np.inf and stats[s, 1] == -np.inf
        assert f64_bits(stats[s, 2:]).tolist() == [0, 0]  # +0.0


@pytest.mark.parametrize("scale", [0.125, 1 / 3], ids=["eighth", "third"])
def test_scale_is_one_fp32_multiply(segments, scale):
    flat = flat_of(segments, 7.0)
    offsets = segments[1]
    ref = th.model_histograms(flat, offsets, SEGMENT_SIZES, scale=scale)
    plain = th.model_histograms(flat, offsets, SEGMENT_SIZES)
    assert not np.array_equal(ref[0], plain[0])  # (the scale moves values across buckets: the comparison can tell)
    got = th.flat_histograms(torch.from_numpy(flat).to(DEV), offsets, SEGMENT_SIZES, scale=scale)
    assert_matches_model(got, ref, "scale %r" % scale)


def test_repeatable_and_stream_independent(segments):
    flat = torch.from_numpy(flat_of(segments, 7.0)).to(DEV)
    offsets = segments[1]
    a = th.flat_histograms(flat, offsets, SEGMENT_SIZES)
    b = th.flat_histograms(flat, offsets, SEGMENT_SIZES)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = th.flat_histograms(flat, offsets, SEGMENT_SIZES)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for other in (b, c):
        for x, y in zip(a, other):
            assert torch.equal(x.view(torch.int64), y.view(torch.int64))


def test_wrapper_refuses_what_the_kernel_does_not_take():
    flat = torch.zeros(64, device=DEV)
    with pytest.raises(ValueError, match="2\\^32"):
        th.flat_histograms(flat, [0], [1 << 32])
    with pytest.raises(ValueError, match="segments"):
        th.flat_histograms(flat, [], [])
    with pytest.raises(RuntimeError, match="past the end"):
        th.flat_histograms(flat, [60], [5])
    with pytest.raises(RuntimeError, match="GPU only"):
        th.flat_histograms(torch.zeros(8), [0], [8])
    with pytest.raises(ValueError, match="fp32"):
        th.flat_histograms(flat.double(), [0], [8])


# -- a real optimiser ---------------------------------------------------------------------------------------------------------------
class _Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.c1 = torch.nn.Conv1d(5, 7, 3)
        self.c2 = torch.nn.Conv2d(3, 6, (3, 5))
        # a weight whose logical order is a permutation of its dense memory order, as the engine's channels-last conv weights
        self.perm = torch.nn.Parameter(torch.randn(6, 5, 3, 4).permute(0, 3, 1, 2))
        self.odd = torch.nn.Parameter(torch.randn(C + 3))

    def forward(self, x1, x2):
        return self.c1(x1).square().sum() + self.c2(x2).square().sum() + (self.perm ** 3).sum() + (self.odd * 1e-3).sin().sum()


def _physical(opt, t, i):
    """tensor ``t`` (parameter i's logical shape) in the order it has in the flat buffers"""
    perm = opt._perms[i][0]
    return t.detach().permute(perm).contiguous().reshape(-1).cpu().numpy()


def _check_optimizer(opt, which, tensors, scale):
    """counts, tallies, min and max against the model on the logical tensor; the ordered sums bit for bit against the model on the same
    values in buffer order (a sum's bits depend on its order; for a weight stored as it is indexed the two are the same array)"""
    got = [t.cpu().numpy() for t in th.optimizer_histograms(opt, which)]
    for i, t in enumerate(tensors):
        n = t.numel()
        logical = th.model_histograms(t.detach().cpu().contiguous().numpy().reshape(-1), [0], [n], scale=scale)
        buffer_order = th.model_histograms(_physical(opt, t, i), [0], [n], scale=scale)
        assert np.array_equal(got[0][i], logical[0][0]) and np.array_equal(got[1][i], logical[1][0]), (which, i)
        assert np.array_equal(got[2][i, :2], logical[2][0, :2]), (which, i)
        assert np.array_equal(f64_bits(got[2][i, 2:]), f64_bits(buffer_order[2][0, 2:])), (which, i)
        u = th.model_depth(n) * 2.0 ** -53
        assert abs(got[2][i, 3] - logical[2][0, 3]) <= 2 * u * logical[2][0, 3], (which, i)


def test_real_optimizer_weights_and_gradients():
    from speechdrivestemplates_amd.optim import FlatAdam
    torch.manual_seed(5)
    m = _Small().to(DEV)
    assert not m.perm.is_contiguous()
    opt = FlatAdam(m.parameters(), lr=1e-3)
    assert any(list(p[0]) != sorted(p[0]) for p in opt._perms)  # at least one tensor is stored in another order than it is indexed
    _check_optimizer(opt, "param", opt.params, 1.0)
    opt.zero_grad()
    m(torch.randn(2, 5, 9, device=DEV), torch.randn(2, 3, 8, 9, device=DEV)).backward()
    torch.cuda.synchronize()
    opt.grad_scale = 0.5
    _check_optimizer(opt, "grad", [p.grad for p in opt.params], 0.5)
    assert th.optimizer_histograms(opt, "grad")[1][:, 0].cpu().tolist() == [p.numel() for p in opt.params]
    with pytest.raises(RuntimeError, match="EMA"):
        th.optimizer_histograms(opt, "ema")
    with pytest.raises(ValueError, match="which"):
        th.optimizer_histograms(opt, "weights")
    opt.enable_ema(0.9)
    _check_optimizer(opt, "ema", opt.params, 1.0)
    _check_optimizer(opt, "exp_avg_sq", [torch.zeros_like(p) for p in opt.params], 1.0)


# -- the Trainer ----------------------------------------------------------------------------------------------------------------------
def _pipeline(cfg_name, tmp_path, **sys_opts):
    from __graft_entry__ import make_pipeline
    pipe, cfg = make_pipeline(cfg_name, 4, batch_global=4, sys_opts=dict(OUTPUT_DIR=str(tmp_path), **sys_opts))
    pipe.base_path = str(tmp_path)
    pipe.setup_tb_writer()
    return pipe


def _batch(step):
    from oracle import sdt_oracle as O
    return O.make_batch(4, 4, step=step, seed=1)


def _event_items(tmp_path):
    path, = glob.glob(os.path.join(str(tmp_path), "events.out.tfevents.*"))
    return [(ev["step"], item) for ev in tb_events.read_events(path) for item in ev["values"]]


def _same_histogram(h, fields):
    mn, mx, num, s, sq, limit, bucket = fields
    return (h["min"] == mn and h["max"] == mx and h["num"] == num and h["bucket_limit"] == limit and h["bucket"] == bucket
            and f64_bits([h["sum"], h["sum_squares"]]).tolist() == f64_bits([s, sq]).tolist())


def test_trainer_writes_weights_and_gradients_of_every_owned_parameter(tmp_path):
    pipe = _pipeline("voice2pose_sdt_bp", tmp_path, TENSORBOARD=True, HISTOGRAM_INTERVAL=1, HIP_GRAPH=False)
    assert len(pipe.optimizers) >= 2  # (generator and clip-code table: names come from more than one optimiser)
    for step in (1, 2):
        pipe.train_step(_batch(step - 1), step, step, 1)
    torch.cuda.synchronize()
    owned = {id(p) for opt in pipe.optimizers.values() for p in opt.params}
    names = {n: p for n, p in pipe.model.named_parameters() if id(p) in owned}
    assert len(names) == len(owned)
    items = _event_items(tmp_path)
    for prefix in ("weights/", "grads/"):
        for step in (1, 2):
            tags = [it["tag"] for s, it in items if s == step and it["tag"].startswith(prefix) and "histo" in it]
            assert sorted(tags) == sorted(prefix + n for n in names), (prefix, step)
    assert not any(it["tag"].startswith(("ema/", "nonfinite/")) for _, it in items)
    model = {}
    for opt in pipe.optimizers.values():
        sizes = [p.numel() for p in opt.params]
        counts, tallies, stats = th.model_histograms(opt.flat_param.detach().cpu().numpy(), opt.offsets, sizes)
        for i, p in enumerate(opt.params):
            model[id(p)] = (counts[i], tallies[i], stats[i])
    scalars = {(s, it["tag"]): it["simple_value"] for s, it in items if "simple_value" in it}
    for name, p in names.items():
        for step in (1, 2):
            for prefix in ("weights/", "grads/"):
                h, = [it["histo"] for s, it in items if s == step and it["tag"] == prefix + name]
                assert h["num"] == p.numel() and sum(h["bucket"]) == p.numel(), (name, step)
        h, = [it["histo"] for s, it in items if s == 2 and it["tag"] == "weights/" + name]
        assert _same_histogram(h, th.to_proto_fields(*model[id(p)])), name
        assert h["min"] == float(p.detach().min()) and h["max"] == float(p.detach().max()), name  # the tag names THIS tensor
        # weight_norm: sqrt of the ordered sum of squares (model_depth additions deep), stored as an fp32 simple_value (half an ulp, 2^-24);
        # the reference norm is numpy's pairwise float64 sum (at most 64 further roundings for any size here)
        x = p.detach().double().cpu().numpy().reshape(-1)
        ref = float(np.sqrt(np.sum(x * x)))
        tol = (th.model_depth(p.numel()) + 64) * 2.0 ** -53 + 2.0 ** -24
        assert abs(scalars[(2, "weight_norm/" + name)] - ref) <= tol * ref, name
        assert (2, "grad_norm/" + name) in scalars and (1, "weight_norm/" + name) in scalars
    pipe.close()


def test_default_interval_writes_no_histogram(tmp_path):
    pipe = _pipeline("pose2pose", tmp_path, TENSORBOARD=True, LOG_INTERVAL=1)
    assert pipe.cfg.SYS.HISTOGRAM_INTERVAL is None
    for step in (1, 2):
        pipe.train_step(_batch(step - 1), step, step, 1)
    torch.cuda.synchronize()
    items = _event_items(tmp_path)
    assert items and not any("histo" in it for _, it in items)
    assert all(it["tag"].startswith("train/") for _, it in items), sorted({it["tag"] for _, it in items})
    pipe.close()
    from speechdrivestemplates_amd.core.pipelines import get_pipeline
    from speechdrivestemplates_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_list(["SYS.HISTOGRAM_INTERVAL", 3])
    with pytest.raises(ValueError, match="TENSORBOARD"):
        get_pipeline("Pose2Pose")(cfg)


def test_hipgraph_run_writes_the_gradient_of_the_replayed_step(tmp_path):
    pipe = _pipeline("pose2pose", tmp_path, TENSORBOARD=True, HISTOGRAM_INTERVAL=1, HIP_GRAPH=True)
    snaps, write = {}, pipe.write_histograms

    def spying(global_step):
        snaps[global_step] = {k: (o.flat_grad.detach().clone(), float(o.grad_scale)) for k, o in pipe.optimizers.items()}
        write(global_step)

    pipe.write_histograms = spying
    for step in (1, 2, 3, 4):  # two eager warm-ups, the capture, one replay
        pipe.train_step(_batch(step - 1), step, step, 1)
    torch.cuda.synchronize()
    assert pipe._graphed.segments is not None and pipe._graphed.calls == 4
    items = _event_items(tmp_path)
    checked = 0
    for key, opt in pipe.optimizers.items():
        grad, scale = snaps[4][key]
        sizes = [p.numel() for p in opt.params]
        counts, tallies, stats = th.model_histograms(grad.cpu().numpy(), opt.offsets, sizes, scale=scale)
        by_id = {id(p): i for i, p in enumerate(opt.params)}
        for name, p in pipe.model.named_parameters():
            if id(p) in by_id:
                i = by_id[id(p)]
                h, = [it["histo"] for s, it in items if s == 4 and it["tag"] == "grads/" + name]
                assert _same_histogram(h, th.to_proto_fields(counts[i], tallies[i], stats[i])), name
                assert h["num"] == p.numel()
                checked += 1
    assert checked >= 4 and any(float(g.abs().max()) > 0 for g, _ in snaps[4].values())
    assert sorted({s for s, it in items if "histo" in it}) == [1, 2, 3, 4]
    pipe.close()
