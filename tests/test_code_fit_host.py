"""Fitting template codes to clips (TEST.FIT_CODE, code_fit.py): the numpy contract models of the four kernels against
brute-force float64 / math.fsum / exact-rational restatements, the configuration check, the candidate rows, the command line's arguments,
DEMO.CODE_PATH's errors and the float64 loop model on a toy chain.  No GPU."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from speechdrivestemplates_amd import code_fit as cf
from speechdrivestemplates_amd.config import check_fit_code, get_cfg_defaults

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(*opts, name="voice2pose_sdt_bp"):
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(REPO, "configs", name + ".yaml"))
    cfg.merge_from_list(list(opts))
    return cfg


# ---- contract models ---------------------------------------------------------------------------------------------------------------------------
def _round_f32(x):
    """the float32 nearest to the rational x, ties to even"""
    f = np.float32(float(x))
    cands = sorted({np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))}, key=float)
    dist = [abs(Fraction(float(c)) - x) for c in cands]
    best = min(dist)
    tied = [c for c, d in zip(cands, dist) if d == best]
    if len(tied) == 1:
        return tied[0]
    return next(c for c in tied if (c.view(np.uint32) & 1) == 0)


def test_fma32_is_the_exactly_rounded_fused_operation():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(400).astype(np.float32)
    b = rng.standard_normal(400).astype(np.float32)
    c = (-(a.astype(np.float64) * b)).astype(np.float32) + (rng.standard_normal(400) * 1e-7).astype(np.float32)  # cancellation: ties and
    c[200:] = rng.standard_normal(200).astype(np.float32) * np.float32(1e4)                                      # long carries
    got = cf.fma32(a, b, c)
    for i in range(400):
        want = _round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i].view(np.uint32) == want.view(np.uint32), (i, a[i], b[i], c[i])
    separate = (a * b + c).astype(np.float32)
    assert (separate.view(np.uint32) != got.view(np.uint32)).any()  # (the fused result is not the twice-rounded one)
    assert np.isnan(cf.fma32(np.float32(np.inf), np.float32(0), np.float32(1)))


@pytest.mark.parametrize("B,n", [(1, 2), (3, 484), (2, 15488), (33, 70)])
def test_loss_model_against_fsum(B, n):
    rng = np.random.default_rng(B * 1000 + n)
    pred = rng.standard_normal((B, n)).astype(np.float32)
    gt = rng.standard_normal((B, n)).astype(np.float32)
    pred[0, 0] = gt[0, 0]  # an exact zero difference
    loss, dpred = cf.loss_model(pred, gt)
    for b in range(B):
        want = math.fsum(abs(float(p) - float(g)) for p, g in zip(pred[b], gt[b])) / n
        assert abs(loss[b] - want) <= 4 * n * 2.0 ** -53 * want  # (a float64 sum of n positive terms in any order)
    e = pred.astype(np.float64) - gt
    assert dpred.dtype == np.float32 and dpred[0, 0] == 0 and not np.signbit(dpred[0, 0])
    assert np.array_equal(dpred, (np.sign(e) * np.float32(1.0 / n)).astype(np.float32))


def test_loss_model_nonfinite_stays_in_its_clip():
    rng = np.random.default_rng(1)
    pred = rng.standard_normal((4, 300)).astype(np.float32)
    gt = rng.standard_normal((4, 300)).astype(np.float32)
    clean = cf.loss_model(pred, gt)[0]
    pred[1, 7] = np.nan
    pred[2, 9], gt[3, 11] = np.inf, -np.inf
    pred[3, 12], gt[3, 12] = np.inf, np.inf  # inf - inf: a NaN difference
    loss, dpred = cf.loss_model(pred, gt)
    assert loss[0] == clean[0] and np.isnan(loss[1:]).all()
    assert np.isnan(dpred[1, 7]) and dpred[2, 9] == np.float32(1 / 300) and dpred[3, 11] == np.float32(1 / 300) and np.isnan(dpred[3, 12])
    assert np.isfinite(np.delete(dpred[1], 7)).all()


def test_adam_model_against_float64_adam():
    rng = np.random.default_rng(2)
    p = rng.standard_normal(64).astype(np.float32)
    g = (rng.standard_normal(64) * 1e-2).astype(np.float32)
    m, v = np.zeros(64, np.float32), np.zeros(64, np.float32)
    p64, m64, v64 = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    for step in (1, 2, 3):
        p, m, v = cf.adam_model(p, g, m, v, 0.05, step)
        m64 = 0.9 * m64 + 0.1 * g
        v64 = 0.999 * v64 + 0.001 * g.astype(np.float64) ** 2
        p64 = p64 - 0.05 / (1 - 0.9 ** step) * (m64 / (np.sqrt(v64) / math.sqrt(1 - 0.999 ** step) + 1e-8))
        assert np.abs(p - p64).max() < 1e-5 * step  # (fp32 rounding of a step of size lr: a few 1e-8 relative per operation on O(1) values)
    assert p.dtype == m.dtype == v.dtype == np.float32


def test_step_model_bookkeeping_prior_and_nonfinite():
    rng = np.random.default_rng(3)
    B, T, C, D = 4, 5, 8, 3
    code0 = rng.standard_normal((B, D)).astype(np.float32)
    st = cf.new_state(code0, 4)
    h = rng.standard_normal((B, T, C + D)).astype(np.float32)
    h0 = h.copy()
    dh = rng.standard_normal((B, T, C + D)).astype(np.float32)
    mu, ivar = rng.standard_normal(D), np.array([2.0, 0.0, 0.5])
    cf.step_model(st, dh, np.array([1.0, 2.0, np.nan, 3.0]), h, C, 0.05, 0.3, mu, ivar)
    assert np.array_equal(st['best_loss'], [1.0, 2.0, np.inf, 3.0])
    assert np.array_equal(st['best_code'][[0, 1, 3]], code0[[0, 1, 3]]) and (st['best_code'][2] == 0).all()
    assert np.array_equal(st['nonfinite'], [0, 0, 1, 0]) and np.array_equal(st['code'][2], code0[2]) and (st['m'][2] == 0).all()
    assert np.array_equal(h[..., :C], h0[..., :C]) and np.array_equal(h[..., C:], np.repeat(st['code'][:, None], T, axis=1))
    # the gradient: brute-force float64 column sums plus the prior, dimension 1 with a zero ivar gets no prior term
    g = np.array([[math.fsum(float(x) for x in dh[b, :, C + d]) for d in range(D)] for b in range(B)]).astype(np.float32)
    g = (g.astype(np.float64) + 0.3 * (code0.astype(np.float64) - mu) * ivar / D).astype(np.float32)
    want = cf.adam_model(code0, g, np.zeros_like(code0), np.zeros_like(code0), 0.05, 1)[0]
    for b in (0, 1, 3):
        assert np.abs(st['code'][b] - want[b]).max() <= 2e-7  # (same operations up to the association of the prior's products)
    after1 = st['code'].copy()
    dh[1, 2, C] = np.inf  # a non-finite gradient: clip 1 keeps its state, a strictly better loss still counts
    cf.step_model(st, dh, np.array([1.0, 1.5, 0.5, 4.0]), h, C, 0.05)  # equal, better, better (after a NaN), worse
    assert np.array_equal(st['best_loss'], [1.0, 1.5, 0.5, 3.0])
    assert np.array_equal(st['best_code'][0], code0[0]) and np.array_equal(st['best_code'][1], after1[1])
    assert np.array_equal(st['best_code'][2], code0[2]) and np.array_equal(st['best_code'][3], code0[3])
    assert np.array_equal(st['nonfinite'], [0, 1, 1, 0]) and np.array_equal(st['code'][1], after1[1])
    assert st['counter'] == 2 and np.array_equal(st['history'][1], [1.0, 1.5, 0.5, 4.0]) and np.isnan(st['history'][2]).all()
    cf.step_model(st, None, np.array([0.1, 9.0, 9.0, 9.0]), h, C, 0.05, mode=1)  # bookkeeping only: no step, the counter stays
    assert st['counter'] == 2 and st['best_loss'][0] == 0.1 and np.array_equal(st['history'][2], [0.1, 9.0, 9.0, 9.0])


def test_set_and_pick_models():
    h = np.zeros((2, 3, 5), np.float32)
    cf.set_model(np.array([[1, 2], [3, 4]], np.float32), h, 3)
    assert (h[..., :3] == 0).all() and np.array_equal(h[0, 1, 3:], [1, 2]) and np.array_equal(h[1, 2, 3:], [3, 4])
    losses = np.array([[2.0, np.nan, np.nan, 1.0], [1.0, np.nan, np.inf, 1.0], [1.0, np.nan, 5.0, 0.5]])
    cands = np.arange(6, dtype=np.float32).reshape(3, 2)
    idx, best, codes = cf.pick_model(losses, cands)
    assert np.array_equal(idx, [1, -1, 2, 2])  # a tie goes to the lowest index, a clip without a finite loss has none
    assert np.array_equal(best[[0, 2, 3]], [1.0, 5.0, 0.5]) and np.isnan(best[1])
    assert np.array_equal(codes, cands[[1, 0, 2, 2]])


def test_candidate_rows_and_table_stats():
    assert cf.candidate_rows(10, 4) == [0, 2, 5, 7] and cf.candidate_rows(3, 5) == [0, 0, 1, 1, 2] and cf.candidate_rows(7, 1) == [0]
    with pytest.raises(ValueError):
        cf.candidate_rows(0, 4)
    t = np.array([[1.0, 5.0], [3.0, 5.0], [8.0, 5.0]], np.float32)
    mean, mu, ivar = cf.table_stats_model(t)
    assert mean.dtype == np.float32 and np.array_equal(mu, [4.0, 5.0]) and ivar[0] == 1.0 / 13.0 and ivar[1] == 0.0
    assert np.array_equal(cf.table_stats_model(t[:1])[2], [0.0, 0.0])


# ---- configuration -----------------------------------------------------------------------------------------------------------------------------
def test_check_fit_code_accepts():
    assert check_fit_code(_cfg()) is None  # off by default
    on = check_fit_code(_cfg("TEST.FIT_CODE.ENABLE", True))
    assert on == {'steps': 100, 'lr': 0.05, 'init': 'mean', 'candidates': 0, 'prior': 0.0}
    t = check_fit_code(_cfg("TEST.FIT_CODE.ENABLE", True, "TEST.FIT_CODE.INIT", "table", "TEST.FIT_CODE.CANDIDATES", 4, "TEST.FIT_CODE.STEPS", 1000,
                            "TEST.FIT_CODE.PRIOR", 0.5, "TEST.FIT_CODE.LR", 1))
    assert t == {'steps': 1000, 'lr': 1.0, 'init': 'table', 'candidates': 4, 'prior': 0.5}


@pytest.mark.parametrize("opts,name,match", [
    (("TEST.FIT_CODE.ENABLE", 1), None, "TEST.FIT_CODE.ENABLE must be True or False"),
    (("TEST.FIT_CODE.STEPS", 0), None, "TEST.FIT_CODE.STEPS"),
    (("TEST.FIT_CODE.STEPS", 1001), None, "TEST.FIT_CODE.STEPS"),
    (("TEST.FIT_CODE.LR", 0.0), None, "TEST.FIT_CODE.LR"),
    (("TEST.FIT_CODE.INIT", "best"), None, "TEST.FIT_CODE.INIT"),
    (("TEST.FIT_CODE.CANDIDATES", 65), None, "TEST.FIT_CODE.CANDIDATES"),
    (("TEST.FIT_CODE.INIT", "table"), None, "TEST.FIT_CODE.CANDIDATES must be at least 1"),
    (("TEST.FIT_CODE.PRIOR", -0.1), None, "TEST.FIT_CODE.PRIOR"),
    (("TEST.FIT_CODE.ENABLE", True), "pose2pose", "TEST.FIT_CODE.ENABLE is a Voice2Pose key"),
    (("TEST.FIT_CODE.ENABLE", True), "voice2pose_s2g", "CLIP_CODE.DIMENSION"),
    (("TEST.FIT_CODE.ENABLE", True, "TEST.MULTIPLE", 2), None, "TEST.MULTIPLE"),
    (("TEST.FIT_CODE.ENABLE", True, "VOICE2POSE.GENERATOR.CLIP_CODE.SAMPLE_FROM_NORMAL", True), None, "SAMPLE_FROM_NORMAL"),
    (("TEST.FIT_CODE.ENABLE", True, "VOICE2POSE.GENERATOR.CLIP_CODE.TEST_WITH_GT_CODE", True), None, "TEST_WITH_GT_CODE"),
])
def test_check_fit_code_rejects(opts, name, match):
    with pytest.raises(ValueError, match=match):
        check_fit_code(_cfg(*opts, name=name or "voice2pose_sdt_bp"))


# ---- command line and DEMO.CODE_PATH -----------------------------------------------------------------------------------------------------------
def test_cli_arguments():
    a = cf.parse_args(["--config", "c.yaml", "--checkpoint", "x.pth", "--clip", "clip.npz", "--out", "o.npz"])
    assert (a.steps, a.lr, a.init, a.candidates, a.prior, a.opts) == (None, None, None, None, None, [])
    a = cf.parse_args(["--config", os.path.join(REPO, "configs", "voice2pose_sdt_bp.yaml"), "--checkpoint", "x.pth", "--clip", "clip.npz", "--out",
                       "o.npz", "--steps", "7", "--lr", "0.1", "--init", "table", "--candidates", "3", "--prior", "0.25", "DATASET.NUM_FRAMES", "32"])
    cfg, opts = cf.cfg_from_args(a)
    assert opts == {'steps': 7, 'lr': 0.1, 'init': 'table', 'candidates': 3, 'prior': 0.25}
    assert cfg.TEST.FIT_CODE.ENABLE is True and cfg.DATASET.NUM_FRAMES == 32
    for bad in (["--init", "random"], ["--steps", "many"], ["DATASET.NUM_FRAMES"]):
        with pytest.raises(SystemExit):
            cf.parse_args(["--config", "c", "--checkpoint", "x", "--clip", "k", "--out", "o"] + bad)
    with pytest.raises(SystemExit):
        cf.parse_args(["--config", "c.yaml"])


def test_demo_code_path_errors(tmp_path):
    good, flat, wide, rows, named, nan = (str(tmp_path / n) for n in ("g.npz", "f.npz", "w.npz", "r.npz", "n.npz", "nan.npz"))
    v = np.arange(32, dtype=np.float64)[None]
    np.savez(good, v=v)
    np.savez(flat, v=v[0])
    np.savez(wide, v=np.zeros((1, 16)))
    np.savez(rows, v=np.zeros((2, 32)))
    np.savez(named, code=v)
    np.savez(nan, v=np.full((1, 32), np.nan))
    assert cf.demo_code(_cfg()) is None
    for path in (good, flat):
        got = cf.demo_code(_cfg("DEMO.CODE_PATH", path))
        assert got.shape == (1, 32) and got.dtype == np.float32 and np.array_equal(got, v)  # as it is: no x10 (that is Pose2Pose's)
    assert cf.demo_code(_cfg("DEMO.CODE_PATH", good, name="pose2pose")) is None  # Pose2Pose reads the key itself
    assert cf.demo_code(_cfg("DEMO.CODE_PATH", good, name="voice2pose_s2g")) is None  # no code: the key stays ignored
    with pytest.raises(ValueError, match="DEMO.CODE_PATH and DEMO.CODE_INDEX"):
        cf.demo_code(_cfg("DEMO.CODE_PATH", good, "DEMO.CODE_INDEX", 3))
    with pytest.raises(ValueError, match="16 dimensions"):
        cf.demo_code(_cfg("DEMO.CODE_PATH", wide))
    with pytest.raises(ValueError, match=r"\(1, D\) or \(D,\)"):
        cf.demo_code(_cfg("DEMO.CODE_PATH", rows))
    with pytest.raises(ValueError, match="no array 'v'"):
        cf.demo_code(_cfg("DEMO.CODE_PATH", named))
    with pytest.raises(ValueError, match="non-finite"):
        cf.demo_code(_cfg("DEMO.CODE_PATH", nan))


# ---- the float64 loop model on a toy chain -----------------------------------------------------------------------------------------------------
def _toy(seed, B=2, T=6, C=3, D=4, n_out=5):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(B, C, T, generator=g, dtype=torch.float64)
    w1 = torch.randn(8, C + D, 3, generator=g, dtype=torch.float64) * 0.4
    w2 = torch.randn(n_out, 8, 3, generator=g, dtype=torch.float64) * 0.4
    gt = torch.randn(B, n_out * T, generator=g, dtype=torch.float64)

    def tail(code, feat=feat):  # two conv blocks with an instance norm over the channels between them, per clip
        x = torch.cat([feat, code.unsqueeze(2).repeat(1, 1, T)], 1)
        y = torch.nn.functional.conv1d(x, w1, padding=1)
        y = torch.nn.functional.leaky_relu((y - y.mean(1, keepdim=True)) / torch.sqrt(y.var(1, unbiased=False, keepdim=True) + 1e-5), 0.2)
        return torch.nn.functional.conv1d(y, w2, padding=1).permute(0, 2, 1).reshape(code.shape[0], -1)

    return tail, feat, gt


def test_loop_model_gradient_matches_finite_differences():
    tail, _, gt = _toy(0)
    code0 = torch.zeros(2, 4, dtype=torch.float64)
    mu, ivar = torch.full((4,), 0.1, dtype=torch.float64), torch.tensor([1.0, 2.0, 0.0, 0.5], dtype=torch.float64)
    res = cf.loop_model(tail, gt, code0, 3, 0.05, 0.2, mu, ivar)
    assert res['history'].shape == (4, 2) and len(res['grads']) == 3 and len(res['codes']) == 4
    assert res['min_abs_diff'] > 1e-5  # no |pred - gt| near the kink of the L1 loss: the finite differences are meaningful
    for it in range(3):
        c = res['codes'][it]

        def clip_loss(cc, b):
            return float(((tail(cc) - gt).abs().mean(dim=1) + 0.2 * 0.5 / 4 * (((cc - mu) ** 2) * ivar).sum(dim=1))[b])

        for b in range(2):
            for d in range(4):
                e = torch.zeros_like(c)
                e[b, d] = 1e-6
                fd = (clip_loss(c + e, b) - clip_loss(c - e, b)) / 2e-6
                assert abs(fd - float(res['grads'][it][b, d])) < 1e-7, (it, b, d)
    assert torch.equal(res['loss_first'], res['history'][0]) and torch.equal(res['loss_best'], res['history'].min(dim=0).values)
    best_it = res['history'].argmin(dim=0)
    for b in range(2):
        assert torch.equal(res['code'][b], res['codes'][int(best_it[b])][b])


def test_loop_model_clips_are_independent():
    tail, feat, gt = _toy(1)
    code0 = torch.zeros(2, 4, dtype=torch.float64)
    a = cf.loop_model(tail, gt, code0, 3, 0.05)
    feat2, gt2 = feat.clone(), gt.clone()
    feat2[1] += 1.0
    gt2[1] -= 0.5
    b = cf.loop_model(lambda c: tail(c, feat2), gt2, code0, 3, 0.05)
    assert torch.equal(a['history'][:, 0], b['history'][:, 0]) and torch.equal(a['code'][0], b['code'][0])
    assert not torch.equal(a['history'][:, 1], b['history'][:, 1])
