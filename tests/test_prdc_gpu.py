"""The feature-set metrics on the device (csrc/prdc.hip) against the numpy contract model (prdc.prdc_model / result_model; DESIGN.md section
33): every integer equal, every float64 word bit-identical.  Nothing has a tolerance: there is no square root, no atomic on a float and every
order is fixed.  Shapes are the smallest at which the kernels can go wrong: k + 1 rows, one row either side of a wave and of a workgroup of 256
queries, widths either side of the padded register widths 8 / 16 / 32 / 64, and one case that spans several LDS tiles and several slices."""
import numpy as np
import pytest
import torch

from speechdrivestemplates_amd import prdc

pytestmark = pytest.mark.gpu


def lattice(rng, n, D, span):
    return (rng.integers(-span, span + 1, size=(n, D)).astype(np.float64) / 8.0).astype(np.float32)


def make_sets(seed, nr, ng, D, kind):
    """'lattice': integers / 8 on a coarse grid (massive exact ties, duplicated rows); 'random': float32 normal features, the generated set shifted"""
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == 'lattice':
        span = 2 if D <= 3 else 8
        return lattice(rng, nr, D, span), lattice(rng, ng, D, span)
    return rng.standard_normal((nr, D)).astype(np.float32), (0.8 * rng.standard_normal((ng, D)) + 0.3).astype(np.float32)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x.astype(np.int64)


def assert_same(label, got, ref, keys):
    """prints how many words agree, then asserts that all do"""
    same = total = 0
    bad = []
    for key in keys:
        g, r = bits(np.atleast_1d(got[key])), bits(np.atleast_1d(ref[key]))
        assert g.shape == r.shape, (label, key, g.shape, r.shape)
        same, total = same + int((g == r).sum()), total + g.size
        if not np.array_equal(g, r):
            bad.append(key)
    print("  %-44s %d of %d words identical" % (label, same, total))
    assert not bad, (label, bad)


ROW_KEYS = prdc.GEN_ROWS + prdc.REAL_ROWS
VALUE_KEYS = prdc.VALUES + tuple('num_' + v for v in prdc.VALUES) + ('rows_real', 'rows_gen', 'k', 'err')

CASES = [  # (Nr, Ng, D, k, kind): set sizes from {k + 1, 63, 64, 65, 130, 257}, mixed
    (2, 257, 1, 1, 'lattice'), (63, 65, 3, 3, 'lattice'), (64, 64, 32, 5, 'random'), (65, 63, 64, 16, 'random'), (130, 17, 3, 16, 'lattice'),
    (257, 130, 64, 5, 'lattice'), (257, 257, 32, 1, 'random'), (4, 64, 1, 3, 'lattice'), (130, 257, 64, 3, 'random'), (6, 6, 3, 5, 'lattice'),
    (64, 130, 1, 5, 'random'), (63, 64, 32, 16, 'lattice')]


@pytest.mark.parametrize("nr,ng,D,k,kind", CASES)
def test_plain_arrays_match_the_model_bit_for_bit(nr, ng, D, k, kind):
    real, gen = make_sets(nr * 1000 + ng + D + k, nr, ng, D, kind)
    ref, dev = prdc.prdc_model(real, gen, k), prdc.prdc_device(real, gen, k)
    assert_same("%dx%d D=%d k=%d %s" % (nr, ng, D, k, kind), dev, ref, VALUE_KEYS + ROW_KEYS)
    assert ref['err'] == 0 and np.array_equal(dev['words'], prdc.model_words(ref))


def test_1500_rows_span_several_tiles_and_slices_and_match_in_one_piece():
    from speechdrivestemplates_amd import _lib
    slices = int(_lib.load().sdt_prdc_slices(1500, 1500))
    assert slices >= 4 and -(-1500 // slices) > 2 * 32  # several slices, each of several 32-row tiles
    real, gen = make_sets(1500, 1500, 1500, 64, 'random')
    ref, dev = prdc.prdc_model(real, gen, 5), prdc.prdc_device(real, gen, 5)
    assert_same("1500x1500 D=64 k=5 (%d slices)" % slices, dev, ref, VALUE_KEYS + ROW_KEYS)
    assert 0 < ref['num_precision'] < 1500 and 0 < ref['num_coverage'] < 1500  # (the case exercises both outcomes of every comparison)


@pytest.mark.parametrize("kind", ['lattice', 'random'])
def test_no_word_depends_on_the_number_of_slices(monkeypatch, kind):
    real, gen = make_sets(77, 257, 130, 64, kind)
    ref = prdc.prdc_model(real, gen, 5)
    runs = {}
    for slices in (None, 1, 2, 300):  # the library's choice, one slice, two, more slices than rows (most of them empty)
        monkeypatch.setattr(prdc, "_SLICES", slices)
        runs[slices] = prdc.prdc_device(real, gen, 5)
        assert_same("%s, slices %s" % (kind, slices), runs[slices], ref, VALUE_KEYS + ROW_KEYS)


def test_too_few_rows_give_nan_and_an_error_word_on_the_device():
    real, gen = make_sets(5, 5, 40, 3, 'lattice')
    ref, dev = prdc.prdc_model(real, gen, 5), prdc.prdc_device(real, gen, 5)
    assert_same("5x40 k=5", dev, ref, VALUE_KEYS + ROW_KEYS)
    assert dev['err'] == prdc.ERR_REAL_ROWS and all(np.isnan(dev[v]) for v in prdc.VALUES) and np.isinf(dev['real_radius']).all()


# ---- the accumulator ---------------------------------------------------------------------------------------------------------------------------
def feed(accs, tables, rng, N, Dh, m, batch, poison=None, indices=None):
    """commits the clips ``indices`` (default: all N, in a shuffled order, in steps of ``batch``) to every accumulator of ``accs`` and, through the
    model, to every numpy table of ``tables``; ``poison``: {clip: value} puts a non-finite value into one feature of that clip"""
    order = rng.permutation(N) if indices is None else np.asarray(indices)
    for lo in range(0, len(order), batch):
        idx = order[lo:lo + batch]
        B = len(idx)
        step = [(0.7 * rng.standard_normal((m * B, Dh)) + s).astype(np.float32) for s in (0.2, 0.0, 0.0, 0.0)]
        for clip, value in (poison or {}).items():
            where = np.flatnonzero(idx == clip)
            if len(where):
                t = clip % 4  # one of the four tensors: the last copy of a prediction, copy 0 of a ground truth (the one that is kept)
                step[t][((m - 1) * B if t < 2 else 0) + where[0], Dh - 1] = value
        for acc in accs:
            acc.add(*[torch.from_numpy(x).cuda() for x in step], torch.from_numpy(idx.astype(np.int64)))
        for t in tables:
            prdc.commit_model(t, *step, idx, m)


def check_accumulator(label, acc, tables, dim_used=None, gathered=None):
    words = acc.result_words(gathered, dim_used)
    ref_words, ref_rows = prdc.result_model(tables, acc.dim, acc.copies, acc.k, dim_used)
    assert_same(label + " epoch words", {'w': words}, {'w': ref_words}, ['w'])
    assert_same(label + " rows", acc.rows(), ref_rows, ROW_KEYS + ('real_clip', 'gen_clip', 'gen_copy'))
    return prdc.result_values(words)


@pytest.mark.parametrize("N,Dh,m,k,batch", [(63, 1, 1, 1, 8), (65, 16, 3, 5, 7), (130, 32, 1, 16, 32), (64, 32, 3, 3, 5), (40, 4, 16, 5, 4)])
def test_accumulator_matches_the_model(N, Dh, m, k, batch):
    rng = np.random.Generator(np.random.PCG64(N + Dh + m))
    acc, table = prdc.FeatureSetAccumulator(N, 2 * Dh, m, k), prdc.new_table(N, 2 * Dh, m)
    feed([acc], [table], rng, N, Dh, m, batch)
    assert np.array_equal(acc.state().cpu().numpy(), table)
    res = check_accumulator("N=%d D=%d m=%d k=%d" % (N, 2 * Dh, m, k), acc, [table])
    assert res['rows_real'] == N and res['rows_gen'] == N * m and res['rows_real_floor'] == (N + 1) // 2 and res['rows_gen_floor'] == N // 2
    first = acc.result_words()
    check_accumulator("mu alone", acc, [table], dim_used=Dh)
    assert np.array_equal(acc.result_words(), first)  # two calls, the same bits (and no trace of the mu-only call between them)
    acc.reset()
    assert not acc.state().any() and acc.result()['clips_seen'] == 0


def test_nonfinite_clips_an_index_outside_the_table_and_unseen_clips():
    rng = np.random.Generator(np.random.PCG64(4))
    N, Dh, m = 70, 8, 3
    acc, table = prdc.FeatureSetAccumulator(N, 2 * Dh, m, 3), prdc.new_table(N, 2 * Dh, m)
    indices = [i for i in range(N) if i % 9 != 4] + [N, -1, N + 5]  # some clips never arrive; three indices outside the table
    feed([acc], [table], rng, N, Dh, m, 8, poison={3: np.nan, 12: np.inf, 33: -np.inf, 62: np.nan}, indices=indices)
    assert np.array_equal(acc.state().cpu().numpy(), table)
    res = check_accumulator("NaN / inf / outside", acc, [table])
    seen = sum(i % 9 != 4 for i in range(N))
    assert (res['clips_seen'], res['clips_nonfinite'], res['index_errors'], res['rows_real']) == (seen, 4, 3, seen - 4)
    rows = acc.rows()
    assert not set(rows['real_clip']) & {3, 12, 33, 62} and not set(rows['gen_clip']) & {3, 12, 33, 62}


@pytest.mark.parametrize("ranks", [2, 3])
def test_rank_tables_on_one_device(ranks):
    rng = np.random.Generator(np.random.PCG64(ranks))
    N, Dh, m, k = 66, 16, 2, 5
    accs = [prdc.FeatureSetAccumulator(N, 2 * Dh, m, k) for _ in range(ranks)]
    tables = [prdc.new_table(N, 2 * Dh, m) for _ in range(ranks)]
    for r in range(ranks):  # rank r has the clips n with n % ranks == r, and every rank the clips 10 .. 19 (with its own features)
        own = [n for n in range(N) if n % ranks == r or 10 <= n < 20]
        feed([accs[r]], [tables[r]], rng, N, Dh, m, 8, poison={11: np.nan} if r == 0 else None, indices=own)
    for label, gathered in (("list of accumulators", accs), ("stacked tensor", torch.stack([a.state() for a in accs]))):
        res = check_accumulator("%d ranks, %s" % (ranks, label), accs[0], tables, gathered=gathered)
        assert res['clips_seen'] == N and res['clips_nonfinite'] == 1  # (clip 11: rank 0's record wins, and it is the poisoned one)
    check_accumulator("%d ranks, reversed" % ranks, accs[-1], tables[::-1], gathered=accs[::-1])


def test_too_few_live_clips_warn_and_do_not_raise(caplog):
    acc, table = prdc.FeatureSetAccumulator(9, 4, 1, 5), prdc.new_table(9, 4, 1)
    feed([acc], [table], np.random.Generator(np.random.PCG64(1)), 9, 2, 1, 4, indices=[0, 2, 4, 6, 8])
    check_accumulator("5 clips, k = 5", acc, [table])
    with caplog.at_level("WARNING"):
        res = acc.result()
    assert res['err'] == prdc.ERR_REAL_ROWS | prdc.ERR_GEN_ROWS and res['err_floor'] and all(np.isnan(res[v]) for v in prdc.VALUES)
    assert any("needs more than k = 5" in r.getMessage() for r in caplog.records)


def test_unsupported_sizes_raise_before_any_launch():
    for args in ((8, 66, 1, 5), (8, 7, 1, 5), (8, 8, 17, 5), (8, 8, 1, 17), (8, 8, 1, 0), (0, 8, 1, 5), ((1 << 20) // 2 + 1, 8, 2, 5)):
        with pytest.raises(ValueError):
            prdc.FeatureSetAccumulator(*args)
    acc = prdc.FeatureSetAccumulator(8, 8, 2, 3)
    for dim_used in (0, 9):
        with pytest.raises(ValueError, match="dim_used"):
            acc.result(dim_used=dim_used)
    x = torch.zeros((4, 4), dtype=torch.float32, device='cuda')
    with pytest.raises(ValueError, match="copies of one batch"):
        acc.add(x[:3], x[:3], x[:3], x[:3], torch.zeros(3, dtype=torch.int64))
    with pytest.raises(TypeError):
        acc.add(x, x, x, x.double(), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="tables"):
        acc.result(gathered=[acc] * 65)
    with pytest.raises(ValueError):
        prdc.prdc_device(np.zeros((8, 65), dtype=np.float32), np.zeros((8, 65), dtype=np.float32), 3)
    with pytest.raises(ValueError, match="must be finite"):
        prdc.prdc_device(np.full((8, 2), np.nan, dtype=np.float32), np.zeros((8, 2), dtype=np.float32), 3)
    assert not acc.state().any()  # nothing was committed
    # the C entry points themselves refuse (status "unsupported size"), whatever the binding lets through
    from speechdrivestemplates_amd import _lib
    lib, p = _lib.load(), lambda t: t.data_ptr()
    buf = torch.zeros(64, dtype=torch.int64, device='cuda')
    UNSUPPORTED = -3
    assert lib.sdt_prdc_knn(p(buf), p(buf), 1, 65, 5, 1, p(buf), 64, p(buf), None) == UNSUPPORTED
    assert lib.sdt_prdc_knn(p(buf), p(buf), 1, 8, 17, 1, p(buf), 64, p(buf), None) == UNSUPPORTED
    assert lib.sdt_prdc_knn(p(buf), p(buf), (1 << 20) + 1, 8, 5, 1, p(buf), 1 << 40, p(buf), None) == UNSUPPORTED
    assert lib.sdt_prdc_cross(p(buf), p(buf), 1, p(buf), p(buf), 1, p(buf), 0, 1, p(buf), 64, p(buf), p(buf), p(buf), None) == UNSUPPORTED
    assert lib.sdt_prdc_commit(p(buf), p(buf), p(buf), p(buf), p(buf), 1, 17, 4, p(buf), 4, None) == UNSUPPORTED
    assert lib.sdt_prdc_cols(65, 1) == 0 and lib.sdt_prdc_cols(64, 16) == 2 + 64 * 17


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------------------
SIXTEEN = [v + sfx + floor for sfx in ('_mu', '_mu_logvar') for floor in ('', '_floor') for v in prdc.VALUES]


def _set_keys(cfg, on, multiple=1):
    cfg.defrost()
    cfg.TEST.PRDC.ENABLE, cfg.TEST.MULTIPLE = on, multiple
    cfg.freeze()


def test_validate_returns_the_sixteen_values_of_the_model_and_leaves_every_other_key_alone(monkeypatch):
    from oracle import sdt_oracle as O
    from speechdrivestemplates_amd import ops
    from test_fgd_gpu import _validation_pipeline
    n_val = 24
    pipe, cfg = _validation_pipeline(n_val=n_val, batch=8)
    losses, _ = pipe.forward_backward(O.make_batch(4, 16, step=0, seed=1))
    pipe.optimizer_updates(losses)
    steps = []
    orig = pipe.prdc_observer.step

    def recording_step(ctx):  # the features the same test_step hands the observer
        r = ctx.results
        ops.join_side_stream()
        steps.append([r[key].detach().cpu().numpy().copy() for key in ('mu_pred', 'logvar_pred', 'mu_gt', 'logvar_gt')] +
                     [ctx.batch['clip_index'].cpu().numpy().copy()])
        return orig(ctx)
    monkeypatch.setattr(pipe.prdc_observer, "step", recording_step)

    def run(on, multiple=1):
        _set_keys(cfg, on, multiple)
        del steps[:]
        torch.manual_seed(5)
        return pipe.validate(pipe.test_dataloader, 1)

    try:
        off = run(False)
        assert pipe.feature_sets() is None and not steps and not set(off) & set(SIXTEEN)  # nothing constructed, nothing launched
        for multiple in (1, 2):
            on = run(True, multiple)
            assert list(on) == list(off) + SIXTEEN + ['prdc_clips_nonfinite'] if multiple == 1 else set(SIXTEEN) <= set(on)
            acc = pipe.feature_sets()
            Dh = steps[0][0].shape[1]
            table = prdc.new_table(n_val, 2 * Dh, multiple)
            for step in steps:
                prdc.commit_model(table, *step[:4], step[4], multiple)
            assert acc.copies == multiple and np.array_equal(acc.state().cpu().numpy(), table)
            same = 0
            for sfx, dim_used in (('_mu', Dh), ('_mu_logvar', 2 * Dh)):
                ref = prdc.result_values(prdc.result_model([table], 2 * Dh, multiple, cfg.TEST.PRDC.K, dim_used)[0])
                assert ref['rows_real'] == n_val and ref['rows_gen'] == n_val * multiple and ref['err'] == 0 and ref['err_floor'] == 0
                for floor in ('', '_floor'):
                    for v in prdc.VALUES:
                        got, want = np.float64(on[v + sfx + floor]), np.float64(ref[v + floor])
                        print("  m=%d %-28s validate %.17g model %.17g" % (multiple, v + sfx + floor, got, want))
                        same += int(got.view(np.int64) == want.view(np.int64))
            print("  m=%d: %d of 16 values identical" % (multiple, same))
            assert same == 16 and on['prdc_clips_nonfinite'] == 0
            if multiple == 1:  # every key validate() returned before keeps its bits
                for key in off:
                    assert torch.equal(torch.as_tensor(on[key]), torch.as_tensor(off[key])), key
        again = run(False)
        for key in off:
            assert torch.equal(torch.as_tensor(again[key]), torch.as_tensor(off[key])), key
        assert list(again) == list(off)
    finally:
        _set_keys(cfg, False)
