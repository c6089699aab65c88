"""The numpy contract model of the feature-set metrics (prdc.py), no GPU: against an independent brute force on
lattice-valued inputs, on analytic cases, through the rank-table merge, the configuration check and the command line."""
import logging

import numpy as np
import pytest

from speechdrivestemplates_amd import prdc

RNG = np.random.Generator(np.random.PCG64(33))


def lattice(n, D, rng=RNG, span=128):
    """integers in [-span, span] divided by 8: every difference, square and partial sum of a d2 is exact in float64 whatever the formula"""
    return rng.integers(-span, span + 1, size=(n, D)).astype(np.float64) / 8.0


def brute_force(real, gen, k):
    """independent of prdc_model: the distance matrices by broadcasting over all columns at once, np.partition, boolean matrices"""
    real, gen = np.asarray(real, dtype=np.float64), np.asarray(gen, dtype=np.float64)

    def dist(x, y):
        return ((x[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)

    def radii(x):
        d = dist(x, x)
        out = np.empty(len(x))
        for i in range(len(x)):
            others = np.delete(d[i], i)  # self leaves by position
            out[i] = np.partition(others, k - 1)[k - 1] if len(others) >= k else np.inf
        return out

    ra, rb, d = radii(real), radii(gen), dist(gen, real)
    inside = d <= ra[None, :]
    nearest = np.array([min(np.flatnonzero(row == row.min())) for row in d], dtype=np.int64)
    return dict(real_radius=ra, gen_radius=rb, gen_ball_count=inside.sum(axis=1), gen_nearest=nearest, gen_nearest_d2=d.min(axis=1),
                real_covered=(d.min(axis=0) <= ra).astype(np.int64), real_recalled=(d <= rb[:, None]).any(axis=0).astype(np.int64),
                num_precision=int(inside.any(axis=1).sum()), num_recall=int((d <= rb[:, None]).any(axis=0).sum()),
                num_density=int(inside.sum()), num_coverage=int((d.min(axis=0) <= ra).sum()))


@pytest.mark.parametrize("nr,ng,D,k", [(17, 23, 1, 1), (40, 33, 3, 3), (65, 64, 32, 5), (50, 70, 64, 16), (6, 9, 2, 5)])
def test_model_equals_an_independent_brute_force_on_lattice_inputs(nr, ng, D, k):
    """a coarse lattice in few columns gives many exact ties (duplicated rows, equal radii, equal nearest distances): everything must be EQUAL"""
    span = 2 if D <= 3 else 128
    real, gen = lattice(nr, D, span=span), lattice(ng, D, span=span)
    got, ref = prdc.prdc_model(real, gen, k), brute_force(real, gen, k)
    for key, want in ref.items():
        assert np.array_equal(np.asarray(got[key]), np.asarray(want)), key
    assert got['precision'] == ref['num_precision'] / ng and got['recall'] == ref['num_recall'] / nr
    assert got['density'] == ref['num_density'] / (k * ng) and got['coverage'] == ref['num_coverage'] / nr
    assert got['err'] == 0 and (got['rows_real'], got['rows_gen'], got['k']) == (nr, ng, k)


def test_d2_is_the_ordered_sum_of_separately_rounded_terms_and_symmetric():
    x, y = RNG.standard_normal((9, 7)).astype(np.float32).astype(np.float64), RNG.standard_normal((5, 7)).astype(np.float32).astype(np.float64)
    d = prdc.d2_matrix(x, y)
    for i in range(9):
        for j in range(5):
            s = np.float64(0.0)
            for c in range(7):
                t = x[i, c] - y[j, c]
                s = s + t * t
            assert d[i, j] == s
    assert np.array_equal(d, prdc.d2_matrix(y, x).T)


def test_identical_sets_score_one():
    x = RNG.standard_normal((30, 8)).astype(np.float32)
    res = prdc.prdc_model(x, x.copy(), 3)
    assert res['precision'] == res['recall'] == res['coverage'] == 1.0
    assert np.array_equal(res['gen_nearest'], np.arange(30)) and not res['gen_nearest_d2'].any()


def test_two_distant_clusters_score_zero():
    real = RNG.standard_normal((20, 4)).astype(np.float32)
    gen = (RNG.standard_normal((25, 4)) + 1000.0).astype(np.float32)
    res = prdc.prdc_model(real, gen, 5)
    assert res['precision'] == res['recall'] == res['density'] == res['coverage'] == 0.0
    assert res['num_density'] == 0 and not res['real_covered'].any() and not res['real_recalled'].any()


def test_one_real_row_repeated_is_precise_and_recalls_one_row():
    real = RNG.standard_normal((16, 4)).astype(np.float32)
    gen = np.repeat(real[7:8], 12, axis=0)
    res = prdc.prdc_model(real, gen, 3)
    assert res['precision'] == 1.0  # every copy sits at distance 0 from real row 7, inside its ball
    assert res['num_recall'] == 1 and res['recall'] == 1.0 / 16  # the generated radii are 0: only the row itself is within them
    assert np.array_equal(res['real_recalled'], np.arange(16) == 7) and not res['gen_radius'].any()
    assert np.array_equal(res['gen_nearest'], np.full(12, 7))


def test_duplicated_real_rows_have_radius_zero_and_still_hold_a_point():
    real = np.concatenate([np.zeros((4, 2)), lattice(6, 2) + 50.0]).astype(np.float32)  # four rows at the origin: their 3rd neighbour is at d2 0
    gen = np.zeros((5, 2), dtype=np.float32)
    res = prdc.prdc_model(real, gen, 3)
    assert not res['real_radius'][:4].any()
    assert np.array_equal(res['gen_ball_count'], [4] * 5)  # 0 <= 0
    assert res['precision'] == 1.0 and res['real_covered'][:4].all()


def test_nearest_row_ties_resolve_to_the_lowest_position():
    real = np.array([[3.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]], dtype=np.float32)
    res = prdc.prdc_model(real, np.zeros((1, 2), dtype=np.float32), 2)
    assert res['gen_nearest'][0] == 1 and res['gen_nearest_d2'][0] == 1.0


@pytest.mark.parametrize("nr,ng,err", [(5, 20, prdc.ERR_REAL_ROWS), (20, 3, prdc.ERR_GEN_ROWS), (5, 5, prdc.ERR_REAL_ROWS | prdc.ERR_GEN_ROWS),
                                       (0, 9, prdc.ERR_REAL_ROWS)])
def test_too_few_rows_give_nan_and_an_error_word_not_an_exception(nr, ng, err):
    res = prdc.prdc_model(lattice(nr, 3), lattice(ng, 3), 5)
    assert res['err'] == err and all(np.isnan(res[v]) for v in prdc.VALUES)
    assert prdc.describe_error(res)
    words = prdc.model_words(res)
    assert all(int(w) == 0x7ff8000000000000 for w in words[:4]) and words[prdc.OUT_ERR] == err
    if nr <= 5:
        assert np.isinf(res['real_radius']).all()


def _step(rng, B, Dh, m):
    return [rng.standard_normal((m * B, Dh)).astype(np.float32) for _ in range(4)]


def test_merge_of_rank_tables_lowest_rank_wins_and_a_nonfinite_clip_leaves_both_sets():
    rng = np.random.Generator(np.random.PCG64(7))
    N, Dh, m, k = 12, 3, 2, 2
    t0, t1 = prdc.new_table(N, 2 * Dh, m), prdc.new_table(N, 2 * Dh, m)
    a, b = _step(rng, 5, Dh, m), _step(rng, 6, Dh, m)
    b[0][6 + 2, 1] = np.nan  # copy 1 of the clip at position 2 of rank 1's step
    idx0, idx1 = np.array([0, 2, 4, 6, 99]), np.array([2, 3, 5, 6, 7, -1])  # clips 2 and 6 on both ranks; one index outside each table
    prdc.commit_model(t0, *a, idx0, m)
    prdc.commit_model(t1, *b, idx1, m)
    g = prdc.gather_model([t0, t1], 2 * Dh, m)
    assert (g['clips_seen'], g['clips_nonfinite'], g['index_errors']) == (7, 1, 2)  # clips 0 2 3 4 5 6 7; rank 1's clip 5 is the bad one
    live = [0, 2, 3, 4, 6, 7]
    assert list(g['real_clip']) == live and list(g['gen_clip']) == [c for c in live for _ in range(m)]
    assert list(g['gen_copy']) == [0, 1] * len(live)

    def rows_of(step, pos, B):
        mu_p, lv_p, mu_g, lv_g = step
        return np.concatenate([mu_g[pos], lv_g[pos]]), [np.concatenate([mu_p[j * B + pos], lv_p[j * B + pos]]) for j in range(m)]
    gt2, pred2 = rows_of(a, 1, 5)  # clip 2: rank 0 has it
    assert np.array_equal(g['real'][1], gt2.astype(np.float64)) and np.array_equal(g['gen'][2:4], np.array(pred2, dtype=np.float64))
    gt3, pred3 = rows_of(b, 1, 6)  # clip 3: rank 1 alone
    assert np.array_equal(g['real'][2], gt3.astype(np.float64)) and np.array_equal(g['gen'][4:6], np.array(pred3, dtype=np.float64))
    # the other order of the ranks gives clip 2 and clip 6 from the other table
    g10 = prdc.gather_model([t1, t0], 2 * Dh, m)
    assert np.array_equal(g10['real'][1], rows_of(b, 0, 6)[0].astype(np.float64))
    # mu alone; the floor pass splits the live list by position
    gm = prdc.gather_model([t0, t1], 2 * Dh, m, dim_used=Dh)
    assert np.array_equal(gm['real'], g['real'][:, :Dh]) and np.array_equal(gm['gen'], g['gen'][:, :Dh])
    gf = prdc.gather_model([t0, t1], 2 * Dh, m, floor=True)
    assert list(gf['real_clip']) == live[0::2] and list(gf['gen_clip']) == live[1::2]
    assert np.array_equal(gf['real'], g['real'][0::2]) and np.array_equal(gf['gen'], g['real'][1::2])
    words, rows = prdc.result_model([t0, t1], 2 * Dh, m, k)
    res = prdc.result_values(words)
    assert (res['rows_real'], res['rows_gen'], res['rows_real_floor'], res['rows_gen_floor']) == (6, 12, 3, 3)
    assert res['err'] == 0 and res['err_floor'] == 0 and res['clips_nonfinite'] == 1 and res['index_errors'] == 2
    assert res['precision'] == prdc.prdc_model(g['real'], g['gen'], k)['precision'] and len(rows['gen_radius']) == 12


def _cfg(**prdc_keys):
    from speechdrivestemplates_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.PIPELINE_TYPE = "Voice2Pose"
    cfg.VOICE2POSE.POSE_ENCODER.NAME = "PoseSeqEncoder"
    for key, v in prdc_keys.items():
        cfg.TEST.PRDC[key] = v
    return cfg


def test_check_prdc_messages_name_their_key():
    from speechdrivestemplates_amd.config import check_prdc
    assert check_prdc(_cfg()) is None  # off by default
    assert check_prdc(_cfg(ENABLE=True)) == {'k': 5} and check_prdc(_cfg(ENABLE=True, K=16)) == {'k': 16}
    for bad in (0, 17, 2.0, True, None):  # the range is checked whether or not the key is on
        for on in (False, True):
            with pytest.raises(ValueError, match=r"TEST\.PRDC\.K"):
                check_prdc(_cfg(ENABLE=on, K=bad))
    with pytest.raises(ValueError, match=r"TEST\.PRDC\.ENABLE"):
        check_prdc(_cfg(ENABLE=1))
    cfg = _cfg(ENABLE=True)
    cfg.VOICE2POSE.POSE_ENCODER.NAME = None
    with pytest.raises(ValueError, match=r"TEST\.PRDC\.ENABLE needs VOICE2POSE\.POSE_ENCODER\.NAME"):
        check_prdc(cfg)
    cfg = _cfg(ENABLE=True)
    cfg.PIPELINE_TYPE = "Pose2Pose"
    with pytest.raises(ValueError, match=r"TEST\.PRDC\.ENABLE is a Voice2Pose key"):
        check_prdc(cfg)
    cfg = _cfg(ENABLE=True)
    cfg.TEST.MULTIPLE = 17
    with pytest.raises(ValueError, match=r"TEST\.PRDC\.ENABLE takes TEST\.MULTIPLE from 1 to 16"):
        check_prdc(cfg)


def test_command_line_round_trip_on_npy_files_through_the_model_route(tmp_path, capsys):
    real, gen = lattice(40, 6).astype(np.float32), lattice(30, 6).astype(np.float32)
    gen[:3] += 500.0  # three rows far outside
    np.save(tmp_path / "a.npy", real)
    np.save(tmp_path / "b.npy", gen)
    out = str(tmp_path / "rows.npz")
    assert prdc.main([str(tmp_path / "a.npy"), str(tmp_path / "b.npy"), "--k", "3", "--worst", "2", "--out", out, "--host"]) == 0
    lines = capsys.readouterr().out.splitlines()
    ref = prdc.prdc_model(real, gen, 3)
    printed = dict(line.split(": ", 1) for line in lines if not line.startswith(("outside", "uncovered")))
    for v in prdc.VALUES:
        assert float(printed[v]) == ref[v] and int(printed['num_' + v]) == ref['num_' + v]
    assert sum(line.startswith("outside: generated row") for line in lines) == 2
    with np.load(out) as z:
        assert int(z['k']) == 3 and np.array_equal(z['gen_ball_count'], ref['gen_ball_count']) and np.array_equal(z['real_radius'], ref['real_radius'])
        assert float(z['precision']) == ref['precision']
    # the leading half of the columns, and too few rows: exit status 1, a line that says why, no exception
    assert prdc.main([str(tmp_path / "a.npy"), str(tmp_path / "b.npy"), "--mu-only", "--host", "--worst", "0"]) == 0
    assert float(dict(x.split(": ", 1) for x in capsys.readouterr().out.splitlines())['coverage']) == prdc.prdc_model(real[:, :3], gen[:, :3], 5)['coverage']
    np.save(tmp_path / "c.npy", gen[:4])
    assert prdc.main([str(tmp_path / "a.npy"), str(tmp_path / "c.npy"), "--host"]) == 1
    assert "error: the generated set has 4 row(s)" in capsys.readouterr().out


def test_device_route_refuses_the_cpu_and_bad_sizes_before_any_launch():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prdc.prdc_device(lattice(8, 2), lattice(8, 2), 3, device='cpu')
    with pytest.raises(ValueError, match="k must be an integer from 1 to 16"):
        prdc.prdc_model(lattice(8, 2), lattice(8, 2), 17)
    with pytest.raises(ValueError, match=r"one D in \[1, 64\]"):
        prdc.prdc_model(lattice(8, 65), lattice(8, 65), 3)
    with pytest.raises(ValueError, match="must be finite"):
        prdc.prdc_model(np.array([[np.inf, 0.0]] * 4), lattice(8, 2), 3)
    logging.getLogger().info("prdc host checks done")
