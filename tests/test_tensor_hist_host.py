"""Per-tensor histograms, the parts that need no GPU: the bucket rule and the ordered sums of the numpy contract
model, the TensorBoard trimming rule, the HistogramProto records of tb_events, the configuration key and the library's constants."""
import math
import os
import struct
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from speechdrivestemplates_amd import tb_events as tb  # noqa: E402
from speechdrivestemplates_amd import tensor_hist as th  # noqa: E402
from speechdrivestemplates_amd.config import check_histograms, get_cfg_defaults  # noqa: E402

E = th.BUCKET_EDGES


def hist_values(n, seed):
    """normal * exp(U(-30, 30)), then the nearest fp32 of every edge with both fp32 neighbours, +-0, +-1e-13, +-1e-45 and +-3e38"""
    rng = np.random.Generator(np.random.PCG64(seed))
    v = (rng.standard_normal(n) * np.exp(rng.uniform(-30, 30, n))).astype(np.float32)
    with np.errstate(over='ignore'):
        e32 = E.astype(np.float32)
    e32 = e32[np.isfinite(e32)]
    near = np.concatenate([e32, np.nextafter(e32, np.float32(np.inf)), np.nextafter(e32, np.float32(-np.inf))])
    near = near[np.isfinite(near)]
    special = np.array([0.0, -0.0, 1e-13, -1e-13, 1e-45, -1e-45, 3e38, -3e38], dtype=np.float32)
    return np.concatenate([v, near, special]).astype(np.float32)


def test_bucket_edges_are_tensorboards_default():
    assert E.dtype == np.float64 and E.shape == (1549,) and th.NUM_BUCKETS == 1548
    assert E[774] == 0.0 and E[775] == 1e-12 and E[776] == 1e-12 * 1.1 and np.array_equal(E[:774], -E[:774:-1])
    assert np.all(np.diff(E) > 0) and E[-1] < 1e20 <= E[-1] * 1.1


def test_bucket_rule_matches_numpy_histogram():
    v = hist_values(200000, 1)
    counts, tallies, stats = th.model_histograms(v, [0], [v.size])
    v64 = v.astype(np.float64)
    ref, _ = np.histogram(np.clip(v64, E[0], E[-1]), bins=E)
    assert np.array_equal(counts[0], ref)
    assert counts[0].sum() == v.size == tallies[0, 0] and tallies[0, 1] == 0 and tallies[0, 2] == 0
    assert stats[0, 0] == v64.min() and stats[0, 1] == v64.max()
    # both zeros in [0, 1e-12); the values beyond the table in the outermost bucket of their sign
    z = th.model_histograms(np.array([0.0, -0.0, 3e38, -3e38], np.float32), [0], [4])[0][0]
    assert z[774] == 2 and z[1547] == 1 and z[0] == 1 and z.sum() == 4


def test_model_counts_nonfinite_apart_and_ignores_padding():
    flat = np.array([1.0, np.nan, np.inf, -np.inf, 7.0, 7.0, 7.0, 7.0, 2.0, 7.0, 7.0, 7.0], np.float32)
    counts, tallies, stats = th.model_histograms(flat, [0, 8], [4, 1])
    assert tallies.tolist() == [[1, 1, 2], [1, 0, 0]] and counts.sum(1).tolist() == [1, 1]
    assert stats.tolist() == [[1.0, 1.0, 1.0, 1.0], [2.0, 2.0, 2.0, 4.0]]
    empty = th.model_histograms(np.array([np.nan, np.inf], np.float32), [0], [2])[2][0]
    assert empty[0] == np.inf and empty[1] == -np.inf and empty[2] == 0 and empty[3] == 0 and not np.signbit(empty[2:]).any()
    # scale: one fp32 multiply before the widening
    s = th.model_histograms(np.array([3.0], np.float32), [0], [1], scale=1 / 3)[2][0]
    assert s[2] == float(np.float32(3.0) * np.float32(1 / 3))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, th.HIST_CHUNK - 1, th.HIST_CHUNK + 1, 2 * th.HIST_CHUNK + 17])
def test_model_sums_within_depth_bound_of_fsum(n):
    v = np.random.Generator(np.random.PCG64(n)).permutation(hist_values(40000, 2))[:n]
    _, _, stats = th.model_histograms(v, [0], [n])
    v64 = [float(x) for x in v]
    u = th.model_depth(n) * 2.0 ** -53
    sq = math.fsum(x * x for x in v64)
    assert abs(stats[0, 3] - sq) <= u * sq
    assert abs(stats[0, 2] - math.fsum(v64)) <= u * math.fsum(abs(x) for x in v64)


def test_model_depth():
    c = th.HIST_CHUNK
    assert th.model_depth(1) == th.model_depth(c) == c // 256 + 8 + 1 + 8
    assert th.model_depth(256 * c + 1) == c // 256 + 8 + 2 + 8


def _torch_trim(counts, limits):
    """torch.utils.tensorboard.summary.make_histogram, the lines that trim, restated"""
    cum_counts = np.cumsum(np.greater(counts, 0))
    start, end = np.searchsorted(cum_counts, [0, cum_counts[-1] - 1], side="right")
    start = int(start)
    end = int(end) + 1
    counts = counts[start - 1:end] if start > 0 else np.concatenate([[0], counts[:end]])
    limits = limits[start:end + 1]
    return limits.tolist(), counts.tolist()


@pytest.mark.parametrize("bins", [{0: 3}, {1547: 2}, {800: 5}, {0: 1, 5: 2, 9: 4}, {700: 1, 701: 7, 900: 2, 1547: 1}],
                         ids=["bin0", "last", "single", "gaps_from_0", "gaps"])
def test_trimming_is_make_histograms(bins):
    counts = np.zeros(1548, np.int64)
    for b, c in bins.items():
        counts[b] = c
    n = int(counts.sum())
    mn, mx, num, s, sq, limit, bucket = th.to_proto_fields(counts, [n, 0, 0], [1.0, 2.0, 3.0, 4.0])
    ref_limit, ref_bucket = _torch_trim(counts, E)
    assert limit == ref_limit and bucket == [float(x) for x in ref_bucket] and len(limit) == len(bucket)
    assert (mn, mx, num, s, sq) == (1.0, 2.0, float(n), 3.0, 4.0)
    assert sum(bucket) == n and bucket[0] == 0


def test_no_finite_element_no_histogram():
    assert th.to_proto_fields(np.zeros(1548, np.int64), [0, 4, 1], [np.inf, -np.inf, 0.0, 0.0]) is None


# -- event file -----------------------------------------------------------------------------------------------------------------------
def test_histogram_summary_bytes_by_hand():
    got = tb.histogram_summary("w", -1.0, 2.0, 3.0, 1.5, 5.25, [0.0, 2.5], [1.0, 2.0])
    d = lambda x: struct.pack("<d", x)  # noqa: E731
    histo = (b"\x09" + d(-1.0) + b"\x11" + d(2.0) + b"\x19" + d(3.0) + b"\x21" + d(1.5) + b"\x29" + d(5.25)
             + b"\x32\x10" + d(0.0) + d(2.5) + b"\x3a\x10" + d(1.0) + d(2.0))
    assert len(histo) == 81
    value = b"\x0a\x01w" + b"\x2a\x51" + histo  # tag (field 1), histo (field 5, wire type 2, 81 bytes)
    assert got == b"\x0a\x56" + value and len(value) == 0x56


def test_add_histogram_raw_round_trip_is_bit_exact(tmp_path):
    v = hist_values(5000, 3)
    counts, tallies, stats = th.model_histograms(v, [0], [v.size])
    fields = th.to_proto_fields(counts[0], tallies[0], stats[0])
    odd = (-0.0, 5e-324, 1.7976931348623157e308, -1e-300, 0.1, [-0.0, 1e-12, 1.1e-12], [0.0, 3.0, 2.0 ** 53])
    w = tb.EventWriter(str(tmp_path))
    w.add_histogram_raw("weights/a.weight", *fields, step=7)
    w.add_histogram_raw("odd", *odd, step=-2)
    w.close()
    events = tb.read_events(w.path)
    bits = lambda xs: [struct.pack("<d", x) for x in xs]  # noqa: E731
    for ev, tag, step, f in ((events[1], "weights/a.weight", 7, fields), (events[2], "odd", -2, odd)):
        item = ev["values"][0]
        h = item["histo"]
        assert ev["step"] == step and item["tag"] == tag and set(item) == {"tag", "histo"}
        assert bits([h["min"], h["max"], h["num"], h["sum"], h["sum_squares"]]) == bits(f[:5])
        assert bits(h["bucket_limit"]) == bits(f[5]) and bits(h["bucket"]) == bits(f[6])
    with pytest.raises(ValueError):
        tb.histogram_summary("x", 0, 0, 0, 0, 0, [1.0], [1.0, 2.0])


def test_scalar_and_image_records_keep_their_bytes():
    assert tb.scalar_summary("a", 1.5) == b"\x0a\x08\x0a\x01a\x15\x00\x00\xc0\x3f"
    assert tb.image_summary("i", b"xy", 2, 3) == b"\x0a\x0f\x0a\x01i\x22\x0a\x08\x02\x10\x03\x18\x03\x22\x02xy"


def test_describe_lists_scalar_image_and_histogram(tmp_path, capsys):
    w = tb.EventWriter(str(tmp_path))
    w.add_scalar("train/loss", 0.25, 1)
    w.add_image_bytes("train/fig", b"\x89PNG\r\n\x1a\n....", 4, 6, 2)
    w.add_histogram_raw("weights/w", -1.0, 3.0, 4.0, 4.0, 12.0, [0.0, 1.0, 4.0], [0.0, 1.0, 3.0], 3)
    w.close()
    lines = tb.describe(tb.read_events(w.path))
    assert lines == ["- file_version brain.Event:2", "1 train/loss 0.25", "2 train/fig image 4x6 12 bytes",
                     "3 weights/w histogram num=4 min=-1 max=3 mean=1 std=1.41421356 buckets=3"]
    out = tmp_path / "x"
    tb.main([w.path, "--extract", str(out)])
    assert "extracted 2 files" in capsys.readouterr().out
    z = np.load(str(out / "0001_step3_weights_w.npz"))
    assert z["bucket"].tolist() == [0.0, 1.0, 3.0] and z["bucket_limit"].tolist() == [0.0, 1.0, 4.0] and float(z["sum_squares"]) == 12.0


# -- configuration and constants --------------------------------------------------------------------------------------------------------
def _cfg(**sys_opts):
    cfg = get_cfg_defaults()
    opts = []
    for k, v in sys_opts.items():
        opts += ["SYS." + k, v]
    cfg.merge_from_list(opts)
    return cfg


def test_config_default_and_validation():
    cfg = get_cfg_defaults()
    assert cfg.SYS.HISTOGRAM_INTERVAL is None and cfg.SYS.TENSORBOARD is False
    check_histograms(cfg)
    check_histograms(_cfg(TENSORBOARD=True, HISTOGRAM_INTERVAL=5))
    for bad in (0, -1, 2.5, True, "often"):
        with pytest.raises(ValueError, match="positive integer"):
            check_histograms(_cfg(TENSORBOARD=True, HISTOGRAM_INTERVAL=bad))
    with pytest.raises(ValueError, match="TENSORBOARD"):
        check_histograms(_cfg(HISTOGRAM_INTERVAL=5))


def test_model_constants_are_the_librarys():
    from speechdrivestemplates_amd import ops
    c = ops.tensor_hist_constants()
    assert (c["threads"], c["chunk"], c["buckets"]) == (th.HIST_THREADS, th.HIST_CHUNK, th.NUM_BUCKETS)
    assert c["chunk"] % (4 * c["threads"]) == 0 and c["buckets"] == E.size - 1 and c["max_segments"] == 65536


def test_plan_and_unsupported_sizes():
    from speechdrivestemplates_amd import ops
    c = th.HIST_CHUNK
    seg, chunks = ops.tensor_hist_plan([0, 4, 4 + 2 * c + 20], [3, 2 * c + 17, 5], 4 + 2 * c + 20 + 8)
    assert seg.tolist() == [[0, 3, 0], [4, 2 * c + 17, 1], [4 + 2 * c + 20, 5, 4]]
    assert chunks.tolist() == [[0, 0], [1, 0], [1, 1], [1, 2], [2, 0]]
    with pytest.raises(ValueError, match="2\\^32"):
        ops.tensor_hist_plan([0], [1 << 32], 1 << 33)
    with pytest.raises(ValueError, match="segments"):
        ops.tensor_hist_plan([], [], 16)
    with pytest.raises(ValueError, match="segments"):
        ops.tensor_hist_plan([0] * 65537, [1] * 65537, 16)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.tensor_hist_plan([2], [1], 16)
    with pytest.raises(RuntimeError, match="past the end"):
        ops.tensor_hist_plan([8], [9], 16)
