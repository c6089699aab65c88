"""The numpy contract of the bootstrap over clip records (speechdrivestemplates_amd/bootstrap.py) and TEST.BOOTSTRAP's
checks.  No GPU: tests/test_bootstrap_gpu.py holds csrc/bootstrap.hip to these models bit for bit."""
import numpy as np
import pytest

from speechdrivestemplates_amd import bootstrap as bs
from speechdrivestemplates_amd import clip_metrics as cm
from speechdrivestemplates_amd.augment import philox4x32
from speechdrivestemplates_amd.config import check_bootstrap, get_cfg_defaults
from test_clip_metrics_host import alphas_for, part_table, poses

BIG_SEED = (1 << 63) + 5
# the statistical check (n = 512, R = 2000): the largest |half-width / (1.96 s / sqrt(n)) - 1| of the model over the seeds 1 .. 20 is
# 0.0338 (seed 1); doubled.  DESIGN.md section 34 records it.
WIDTH_MARGIN = 2 * 0.0338


def records(n, T=3, K=7, m=1, n_alphas=2, seed=0):
    pred, gt = poses(m * n, T, K, seed=seed)
    return cm.clip_metrics_model(pred, gt, part_table(K), alphas_for(n_alphas), m)


def holed_table(n, N, seed=0, **kw):
    """n live records inside a table of N rows; the other rows are unseen or nonfinite, the first and the last row among them"""
    assert N >= n + 2
    rng = np.random.Generator(np.random.PCG64(seed + 31 * n))
    live = 1 + np.sort(rng.permutation(N - 2)[:n])
    table = np.zeros((N, cm.COLS), dtype=np.int64)
    table[live] = records(n, seed=seed, **kw)
    dead = np.setdiff1d(np.arange(N), live)
    bad = dead[::2]  # seen, but left out: a record with its nonfinite word set
    table[bad] = records(len(bad), seed=seed + 1, **kw)
    table[bad, cm.NONFINITE] = 1
    return table, live


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


@pytest.mark.parametrize("seed", [0, 1, BIG_SEED, 0x0123456789abcdef])
def test_draws_are_the_philox_words(seed):
    key = (seed & 0xffffffff, seed >> 32)
    for n in (1, 2, 7, 63, 1000):
        R = 3
        rows = bs.draws_model(n, R, seed)
        assert rows.shape == (R, n) and rows.dtype == np.int64 and (rows >= 0).all() and (rows < n).all()
        for r in range(R):
            for i in sorted({0, 1, 2, 3, 4, 5, n // 2, n - 1}):
                if i < n:
                    word = int(philox4x32([i >> 2, 3, r, 0], key)[i & 3])
                    assert rows[r, i] == (word * n) >> 32, (n, r, i)
    if seed >> 32:  # the high word of the seed is the second key word
        assert not np.array_equal(bs.draws_model(1000, 2, seed), bs.draws_model(1000, 2, seed & 0xffffffff))
    assert not np.array_equal(bs.draws_model(1000, 2, seed)[0], bs.draws_model(1000, 2, seed)[1])


def test_rank_of_is_exact_on_the_decimal_level():
    assert bs.rank_of(1000, 0.95) == 25 and bs.rank_of(1000, 0.9) == 50 and bs.rank_of(100, 0.99) == 0 and bs.rank_of(100, 0.02) == 49
    assert bs.rank_of(257, 0.01) == 127 and bs.rank_of(1000, 0.002) == 499
    for bad in (0, 1, 1.5, -0.1, True, "0.9"):
        with pytest.raises(ValueError):
            bs.rank_of(1000, bad)


def test_point_row_is_the_epoch_vector_and_the_stages_fit_together():
    table, live = holed_table(130, 200, m=3, n_alphas=3)
    sizes, alphas = cm.part_sizes(part_table(7)), alphas_for(3)
    R, a = 100, 2
    st = bs.stages_model([table], None, sizes, 3, R, a, 7)
    assert st['n'] == 130 and st['dense_a'].shape == (130, bs.W) and st['sums_a'].shape == (R + 1, bs.W)
    assert np.array_equal(st['dense_a'][:, :36], table[live, :36])
    epoch = cm.epoch_model([table], sizes, 3)
    assert np.array_equal(bits(st['values_a'][R]), epoch[:36]) and st['pair_frames_a'][R] == epoch[cm.OUT_PAIR_FRAMES] > 0
    # every interval end is one of the replicate values, and the ranks are those of a plain sort
    for c in range(bs.VALUES):
        col = np.sort(st['values_a'][:R, c])
        assert st['lohi_a'][c, 0] == col[a] and st['lohi_a'][c, 1] == col[R - 1 - a]
    # integer words of a replicate: n draws of whole records
    assert (st['sums_a'][:R, bs.POS] == 130 * 3 * 3).all() and (st['sums_a'][:R, bs.PAIR] == 130 * 3 * 3).all()
    named = bs.intervals_model(table, sizes, alphas, R, 0.95, 7)
    want = cm.epoch_values(epoch, alphas)
    assert list(named) == ['L2'] + [k for k in want if k not in ('clips_nonfinite', 'clips_seen', 'index_errors')]
    for k, (point, lo, hi) in named.items():
        assert lo <= point <= hi and lo < hi, k
        assert k == 'L2' or point == want[k]
    # two ranks: the higher rank's record of a clip the lower rank has seen is not read
    other = table.copy()
    other[live[::2], :20] = bits(np.full(20, 1e9))
    assert bs.intervals_model([table, other], sizes, alphas, R, 0.95, 7) == named
    assert bs.intervals_model([other, table], sizes, alphas, R, 0.95, 7) != named
    assert bs.intervals_model(table, sizes, alphas, R, 0.95, 8) != named  # another seed, other draws


def test_one_copy_has_no_diversity_keys():
    table, _ = holed_table(5, 9)
    named = bs.intervals_model(table, cm.part_sizes(part_table(7)), alphas_for(2), 100, 0.9, 0)
    assert 'L2_hands' in named and 'diversity' not in named and 'diversity_hands' not in named


@pytest.mark.parametrize("n", [1, 64, 130])
def test_identical_records_give_a_degenerate_interval(n):
    """no clip left out, every record the same: a replicate adds the same numbers in the same chunks as the epoch sum"""
    table = np.repeat(records(1, m=2, seed=n), n, axis=0)
    sizes = cm.part_sizes(part_table(7))
    st = bs.stages_model([table], None, sizes, 2, 100, 2, BIG_SEED)
    assert (st['sums_a'][:100] == st['sums_a'][100]).all()
    named = bs.named_intervals(st, alphas_for(2), 100)
    assert 'diversity' in named
    for k, (point, lo, hi) in named.items():
        assert bits(lo) == bits(point) == bits(hi), k


def test_one_live_clip_and_none():
    table, live = holed_table(1, 5)
    sizes = cm.part_sizes(part_table(7))
    st = bs.stages_model([table], None, sizes, 2, 100, 0, 3)
    assert st['n'] == 1 and (st['sums_a'][:100] == st['sums_a'][100]).all() and (st['values_a'][:100] == st['values_a'][100]).all()
    table[live, cm.NONFINITE] = 1
    st = bs.stages_model([table], None, sizes, 2, 100, 0, 3)
    assert st['n'] == 0 and set(st) == {'n', 'dense_a'} and st['dense_a'].shape == (0, bs.W)
    assert bs.intervals_model(table, sizes, alphas_for(2), 100, 0.9, 3) == {} and bs.paired_model(table, table, sizes, alphas_for(2), 100) == {}


def test_paired_with_itself_and_with_halved_errors():
    table, live = holed_table(65, 80, m=2)
    sizes, alphas = cm.part_sizes(part_table(7)), alphas_for(2)
    same = bs.paired_model(table, table, sizes, alphas, 257, 0.9, BIG_SEED)
    assert 'diversity' in same
    for k, v in same.items():
        assert v['a'] == v['b'] and bits(v['diff']) == 0 and bits(v['diff_lo']) == 0 and bits(v['diff_hi']) == 0, k
        assert v['share_a_less'] == 0 and v['share_a_greater'] == 0, k
    half = table.copy()
    half[:, 0:4] = bits(table[:, 0:4].copy().view(np.float64) * 0.5)  # every l2_sum halved: exact
    res = bs.paired_model(table, half, sizes, alphas, 257, 0.9, BIG_SEED)
    for k in ('L2', 'L2_body', 'L2_face', 'L2_hands'):
        assert res[k]['share_a_greater'] == 1 and res[k]['share_a_less'] == 0 and res[k]['diff_lo'] > 0, k
        assert res[k]['b'] == res[k]['a'] / 2 and res[k]['diff_lo'] <= res[k]['diff'] <= res[k]['diff_hi']
    for k in ('PCK', 'vel_L2', 'speed_ratio'):
        assert res[k]['diff'] == 0 and res[k]['share_a_greater'] == 0 and res[k]['share_a_less'] == 0, k
    # live on different clips: only those live in both count
    other = half.copy()
    other[live[:5], cm.SEEN] = 0
    other[live[5:9], cm.NONFINITE] = 1
    st = bs.stages_model([table], [other], sizes, 2, 100, 2, 1)
    assert st['n'] == 56 and np.array_equal(st['dense_a'][:, :36], table[live[9:], :36]) and np.array_equal(st['dense_b'][:, :36], other[live[9:], :36])
    assert (st['signs'].sum(axis=1) == 100).all()


def l2_table(n, seed):
    """n records of one copy and 3 frames whose l2_sum_all comes from a fixed RNG (the other float words stay 0)"""
    rng = np.random.Generator(np.random.PCG64(1234 + seed))
    table = np.zeros((n, cm.COLS), dtype=np.int64)
    table[:, 0] = bits(rng.gamma(4.0, 50.0, n))
    table[:, cm.SEEN], table[:, cm.COPIES], table[:, cm.FRAMES] = 1, 1, 3
    return table


def width_deviation(seed, n=512, R=2000):
    """|half-width of the 95 % interval of L2 / the normal-theory half-width 1.96 s / sqrt(n) - 1|, s the sample standard deviation of the
    per-clip values"""
    sizes = (4, 2, 1, 1)
    table = l2_table(n, seed)
    point, lo, hi = bs.intervals_model(table, sizes, [0.1], R, 0.95, seed)['L2']
    per_clip = table[:, 0].copy().view(np.float64) / (3 * sizes[0])
    assert abs(point - per_clip.mean()) <= 1e-12 * point and lo < point < hi
    return abs((hi - lo) / 2 / (1.96 * per_clip.std(ddof=1) / np.sqrt(n)) - 1)


def test_interval_width_agrees_with_normal_theory():
    dev = width_deviation(0)
    print("  half-width against 1.96 s / sqrt(n): deviation %.4f, margin %.4f" % (dev, WIDTH_MARGIN))
    assert dev <= WIDTH_MARGIN


def _cfg(**keys):
    cfg = get_cfg_defaults()
    cfg.PIPELINE_TYPE = "Voice2Pose"
    cfg.TEST.CLIP_METRICS = keys.pop("CLIP_METRICS", True)
    for k, v in keys.items():
        cfg.TEST.BOOTSTRAP[k] = v
    return cfg


def test_check_bootstrap():
    cfg = get_cfg_defaults()
    assert dict(cfg.TEST.BOOTSTRAP) == {"ENABLE": False, "REPLICATES": 1000, "LEVEL": 0.95, "SEED": 0}
    assert check_bootstrap(cfg) is None and check_bootstrap(_cfg()) is None
    assert check_bootstrap(_cfg(ENABLE=True)) == {'replicates': 1000, 'level': 0.95, 'seed': 0, 'rank': 25}
    assert check_bootstrap(_cfg(ENABLE=True, REPLICATES=100, LEVEL=0.02, SEED=BIG_SEED)) == {
        'replicates': 100, 'level': 0.02, 'seed': BIG_SEED, 'rank': 49}
    for on in (False, True):  # the ranges are checked whether or not the key is on
        for key, bad in (("REPLICATES", 99), ("REPLICATES", 20001), ("REPLICATES", 1000.0), ("REPLICATES", True), ("LEVEL", 0), ("LEVEL", 1),
                         ("LEVEL", 1.2), ("LEVEL", float("nan")), ("LEVEL", "0.9"), ("SEED", -1), ("SEED", 1 << 64), ("SEED", 0.5)):
            with pytest.raises(ValueError, match=r"TEST\.BOOTSTRAP\.%s" % key):
                check_bootstrap(_cfg(ENABLE=on, **{key: bad}))
    with pytest.raises(ValueError, match=r"TEST\.BOOTSTRAP\.ENABLE"):
        check_bootstrap(_cfg(ENABLE=1))
    with pytest.raises(ValueError, match=r"TEST\.BOOTSTRAP\.ENABLE needs TEST\.CLIP_METRICS"):
        check_bootstrap(_cfg(ENABLE=True, CLIP_METRICS=False))


def test_command_line_arguments(tmp_path):
    a = bs.parse_args(["t.npz"])
    assert (a.compare, a.files, a.replicates, a.level, a.seed, a.rank, a.out) == (False, ["t.npz"], 1000, 0.95, 0, 25, None)
    assert a.part_sizes == list(cm.part_sizes(part_table(121)))
    a = bs.parse_args(["compare", "a.npz", "b.npz", "--replicates", "200", "--level", "0.9", "--seed", str(BIG_SEED), "--part-sizes", "7", "3", "2",
                       "2", "--out", "ci.npz"])
    assert (a.compare, a.files, a.replicates, a.rank, a.seed, a.part_sizes, a.out) == (True, ["a.npz", "b.npz"], 200, 10, BIG_SEED, [7, 3, 2, 2],
                                                                                      "ci.npz")
    for bad in (["t.npz", "--replicates", "50"], ["t.npz", "--level", "1"], ["compare", "a.npz"], ["a.npz", "b.npz"]):
        with pytest.raises(SystemExit):
            bs.parse_args(bad)
    table, _ = holed_table(5, 9)
    cm.save_table(str(tmp_path / "t.npz"), table, [0.1, 0.2])
    got, alphas = bs.load_table(str(tmp_path / "t.npz"))
    assert np.array_equal(got, table) and alphas == [0.1, 0.2]
    np.savez(str(tmp_path / "bad.npz"), table=table)
    with pytest.raises(KeyError):
        bs.load_table(str(tmp_path / "bad.npz"))


def test_device_route_has_no_cpu_fallback():
    table, _ = holed_table(5, 9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bs.clip_metric_intervals([table], cm.part_sizes(part_table(7)), [0.1], 100, 0.9, 0)
