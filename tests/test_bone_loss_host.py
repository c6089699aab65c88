"""Host side of the limb-length / limb-direction loss (VOICE2POSE.GENERATOR.LAMBDA_BONE, LAMBDA_BONE_DIR, BONE_MIN_LENGTH; DESIGN.md
section 29): the config keys and their validation, the edge table of the 121-keypoint skeleton, the tables ops.BoneTable builds, and
``bone_loss_f64`` / ``bone_grad_f64`` -- the float64 torch model of the contract that tests/test_bone_loss_gpu.py compares the kernels
with.  No GPU."""
import os

import pytest
import torch

from speechdrivestemplates_amd.config import check_bone_loss, get_cfg_defaults
from speechdrivestemplates_amd.core.datasets import gesture_dataset as gd


def _geometry(pred, gt, mean, std, edges, root, score, min_conf):
    """X, Y (B, T, 2, K) float64, the edges' live mask m (B, T, E) and their vectors vp, vg (B, T, 2, E); dead edges carry zero vectors
    (selected with torch.where BEFORE any arithmetic that could spread a NaN from under the mask)"""
    B, T, _, K = pred.shape
    st, mu = std.double().reshape(B, 1, 2, K), mean.double().reshape(B, 1, 2, K)
    root = torch.as_tensor(root, dtype=torch.int64)
    has, ridx = root >= 0, root.clamp(min=0)
    zero = torch.zeros((), dtype=torch.float64)

    def glob(v):
        P = v.double() * st + mu  # the same expression for pred and gt
        return P + torch.where(has, P[..., ridx], zero)

    X, Y = glob(pred), glob(gt)
    if score is not None and min_conf is not None:
        s = score.reshape(B, T, 2, K) > min_conf  # in the score's own precision, strict
        own = s[:, :, 0] & s[:, :, 1]
        live = own & (~has | own[..., ridx])
    else:
        live = torch.ones(B, T, K, dtype=torch.bool)
    edges = torch.as_tensor(edges, dtype=torch.int64).reshape(-1, 2)
    a, b = edges[:, 0], edges[:, 1]
    m = live[..., a] & live[..., b]
    vp = torch.where(m[:, :, None], X[..., b] - X[..., a], zero)
    vg = torch.where(m[:, :, None], Y[..., b] - Y[..., a], zero)
    return m, vp, vg, a, b, st, has, ridx


def _length(v):
    """|v| over dim 2 with sqrt only ever seeing a positive operand: 0 with a zero gradient where v = 0"""
    sq = v[:, :, 0] * v[:, :, 0] + v[:, :, 1] * v[:, :, 1]
    pos = sq > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))


def bone_loss_f64(pred, gt, mean, std, edges, root, score=None, min_conf=None, edge_w=None, lam_bone=1.0, lam_dir=1.0, min_len=1.0):
    """(G_bone_loss, G_bone_dir_loss) of DESIGN.md section 29 in float64, differentiable in ``pred``.  pred, gt, score: (B, T, 2, K); mean,
    std: (B, 2 K); edges: (E, 2) keypoint pairs; root: K part roots (-1: none); edge_w: E weights (None: 1)."""
    m, vp, vg, _, _, _, _, _ = _geometry(pred, gt, mean, std, edges, root, score, min_conf)
    w = torch.ones(m.shape[2], dtype=torch.float64) if edge_w is None else torch.as_tensor(edge_w, dtype=torch.float64)
    zero = torch.zeros((), dtype=torch.float64)
    lp, lg = _length(vp), _length(vg)
    ln = (lp - lg).abs() / lg.clamp(min=min_len)
    bone = lam_bone * torch.where(m, w * ln, zero).sum() / max(int(m.sum()), 1)
    md = m & (lp > 0) & (lg > 0)
    dot = vp[:, :, 0] * vg[:, :, 0] + vp[:, :, 1] * vg[:, :, 1]
    cos = dot / torch.where(md, lp * lg, torch.ones_like(lp))
    bone_dir = lam_dir * torch.where(md, w * (1.0 - cos), zero).sum() / max(int(md.sum()), 1)
    return bone, bone_dir


def bone_grad_f64(pred, gt, mean, std, edges, root, score=None, min_conf=None, edge_w=None, lam_bone=1.0, lam_dir=1.0, min_len=1.0,
                  g_bone=1.0, g_dir=1.0):
    """The gradient of g_bone * G_bone_loss + g_dir * G_bone_dir_loss in ``pred`` written out analytically, float64 (B, T, 2, K), and
    ``terms``: per element the sum of the ABSOLUTE edge contributions that were added up to it (times |std|) -- the scale of the rounding
    error of that sum, which the tolerance of the GPU test is built on; 0 where nothing was added."""
    m, vp, vg, a, b, st, has, ridx = _geometry(pred, gt, mean, std, edges, root, score, min_conf)
    w = torch.ones(m.shape[2], dtype=torch.float64) if edge_w is None else torch.as_tensor(edge_w, dtype=torch.float64)
    zero, one = torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64)
    lp, lg = _length(vp), _length(vg)
    md = m & (lp > 0) & (lg > 0)
    cl = g_bone / max(int(m.sum()), 1) * lam_bone
    cd = g_dir / max(int(md.sum()), 1) * lam_dir
    lp_safe = torch.where(lp > 0, lp, one)
    t = torch.where(m & (lp > 0), (cl * w) * torch.sign(lp - lg) / lg.clamp(min=min_len), zero)
    ex, ey = t * (vp[:, :, 0] / lp_safe), t * (vp[:, :, 1] / lp_safe)
    # -(vg / (lp lg) - (vp.vg) vp / (lp^3 lg)) = -(c / (lp^3 lg)) (-vp_y, vp_x), c = vp_x vg_y - vp_y vg_x (2-D): exactly 0 where vp == vg
    c = vp[:, :, 0] * vg[:, :, 1] - vp[:, :, 1] * vg[:, :, 0]
    q = torch.where(md, (cd * w) * c / torch.where(md, lp * lp * lp * lg, one), zero)
    e = torch.stack([ex + q * vp[:, :, 1], ey - q * vp[:, :, 0]], dim=2)  # (B, T, 2, E): + at the edge's b end, - at its a end
    dX, absX = torch.zeros_like(pred, dtype=torch.float64), torch.zeros_like(pred, dtype=torch.float64)
    dX.index_add_(3, b, e)
    dX.index_add_(3, a, -e)
    absX.index_add_(3, b, e.abs())
    absX.index_add_(3, a, e.abs())
    kids = torch.nonzero(has).reshape(-1)  # ascending: the children are added into their roots
    tot, tot_abs = dX.clone(), absX.clone()
    tot.index_add_(3, ridx[kids], dX[..., kids])
    tot_abs.index_add_(3, ridx[kids], absX[..., kids])
    return st * tot, st.abs() * tot_abs


def _cfg(**gen):
    cfg = get_cfg_defaults()
    opts = []
    for k, v in gen.items():
        opts += ["VOICE2POSE.GENERATOR." + k, v]
    cfg.merge_from_list(opts)
    cfg.freeze()
    return cfg


def test_defaults_are_off():
    g = get_cfg_defaults().VOICE2POSE.GENERATOR
    assert g.LAMBDA_BONE == 0.0 and g.LAMBDA_BONE_DIR == 0.0 and g.BONE_MIN_LENGTH == 1.0
    assert check_bone_loss(get_cfg_defaults()) is None
    assert check_bone_loss(_cfg(BONE_MIN_LENGTH=3.0, REG_MIN_CONFIDENCE=0.3)) is None  # both lambdas 0: still nothing to run
    assert check_bone_loss(_cfg(LAMBDA_BONE=0.5)) == (0.5, 0.0, 1.0, None, None)
    assert check_bone_loss(_cfg(LAMBDA_BONE_DIR=2, BONE_MIN_LENGTH=4)) == (0.0, 2.0, 4.0, None, None)
    assert check_bone_loss(_cfg(LAMBDA_BONE=1, REG_MIN_CONFIDENCE=0.3, REG_PART_WEIGHTS=[1, 0.5, 2])) == (1.0, 0.0, 1.0, 0.3, (1.0, 0.5, 2.0))


@pytest.mark.parametrize("key,value", [
    ("LAMBDA_BONE", -0.1), ("LAMBDA_BONE", "long"), ("LAMBDA_BONE", None), ("LAMBDA_BONE", True), ("LAMBDA_BONE", float("nan")),
    ("LAMBDA_BONE_DIR", -1), ("LAMBDA_BONE_DIR", [1.0]), ("LAMBDA_BONE_DIR", float("inf")),
    ("BONE_MIN_LENGTH", 0), ("BONE_MIN_LENGTH", -1.0), ("BONE_MIN_LENGTH", None), ("BONE_MIN_LENGTH", "short"),
    ("BONE_MIN_LENGTH", float("nan")),
])
def test_bad_values_raise_and_name_the_key(key, value):
    with pytest.raises(ValueError, match="VOICE2POSE.GENERATOR." + key + " "):
        check_bone_loss(_cfg(**{key: value}))


def test_model_construction_rejects_bad_values():
    from speechdrivestemplates_amd.core.pipelines.voice2pose import Voice2PoseModel
    with pytest.raises(ValueError, match="VOICE2POSE.GENERATOR.LAMBDA_BONE "):
        Voice2PoseModel(_cfg(LAMBDA_BONE=-1.0), num_train_samples=4)
    with pytest.raises(ValueError, match="VOICE2POSE.GENERATOR.BONE_MIN_LENGTH"):
        Voice2PoseModel(_cfg(LAMBDA_BONE_DIR=1.0, BONE_MIN_LENGTH=0.0), num_train_samples=4)
    with pytest.raises(ValueError, match="VOICE2POSE.GENERATOR.REG_PART_WEIGHTS"):  # a reused key, checked with the limb loss on
        Voice2PoseModel(_cfg(LAMBDA_BONE=1.0, REG_PART_WEIGHTS=[1.0, 2.0]), num_train_samples=4)

    def real(*opts):
        cfg = get_cfg_defaults()
        cfg.merge_from_file(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "voice2pose_sdt_bp.yaml"))
        cfg.merge_from_list(list(opts))
        cfg.freeze()
        return cfg

    off = Voice2PoseModel(real(), num_train_samples=4)
    assert off.bone_opts is None and off.bone_table is None
    on = Voice2PoseModel(real("VOICE2POSE.GENERATOR.LAMBDA_BONE", 1.0, "VOICE2POSE.GENERATOR.REG_PART_WEIGHTS", [1.0, 0.5, 2.0]),
                         num_train_samples=4)
    assert on.bone_table.E == 108 and on.bone_table.edge_w == [1.0] * 5 + [0.5] * 63 + [2.0] * 40
    assert on.bone_table.root == gd.PoseTransforms.part_roots(True)


def test_skeleton_edges():
    T = gd.PoseTransforms
    edges = T.skeleton_edges()
    assert len(edges) == 108 and len(set(edges)) == 108 and len({frozenset(e) for e in edges}) == 108
    assert edges[:5] == [(1, 4), (1, 2), (2, 3), (4, 5), (5, 6)]
    face = edges[5:68]
    assert face[:16] == [(9 + k, 10 + k) for k in range(16)]            # the jaw, open
    assert face[16:20] == [(26 + k, 27 + k) for k in range(4)]          # 17-21 behind the 9 body keypoints
    assert face[31:37] == [(45 + k, 46 + k) for k in range(5)] + [(50, 45)]  # the first closed chain, 36-41
    assert face[-1] == (9 + 67, 9 + 60)
    for base, hand in ((79, edges[68:88]), (100, edges[88:])):
        assert hand[:5] == [(base, base + 1), (base + 1, base + 2), (base + 2, base + 3), (base + 3, base + 4), (base, base + 5)]
        assert [b for _, b in hand] == [base + 1 + i for i in range(20)]  # every joint but the wrist point is the far end of one limb
        assert [a for a, _ in hand[::4]] == [base] * 5
    parts = T.part_table()
    assert all(0 <= a < 121 and 0 <= b < 121 and parts[a] == parts[b] for a, b in edges)  # every limb lies inside one part
    # limbs that touch a part root: the forearms end at the wrists (body limbs: neither end is in a part), and of the limbs with an end IN a
    # part only the one at HEAD_ROOT touches a root -- the hands hang off their own first point, not off the wrist
    roots = {gd.HEAD_ROOT, gd.HAND_ROOT_L, gd.HAND_ROOT_R}
    in_part = T.part_roots(True)
    at_root = [e for e in edges if roots & set(e)]
    assert at_root == [(2, 3), (5, 6), (38, 39)]
    assert [e for e in at_root if in_part[e[0]] >= 0 or in_part[e[1]] >= 0] == [(38, gd.HEAD_ROOT)]
    # the roots as one list agree with _part_index
    sel, root = T._part_index("cpu")
    want = [-1] * 121
    for k, r in zip(sel.tolist(), root.tolist()):
        want[k] = r
    assert T.part_roots(True) == want and T.part_roots(False) == [-1] * 121


def test_bone_table_round_trips_and_validates():
    from speechdrivestemplates_amd.ops import BoneTable, bone_incidence
    edges = gd.PoseTransforms.skeleton_edges()
    ptr, inc = bone_incidence(edges, 121)
    assert len(ptr) == 122 and ptr[0] == 0 and ptr[-1] == len(inc) == 216
    back = {}
    for k in range(121):
        row = inc[ptr[k]:ptr[k + 1]]
        assert row == sorted(row)  # ascending edge index within a keypoint
        for ent in row:
            back.setdefault(ent >> 1, [None, None])[0 if ent & 1 else 1] = k
    assert [tuple(back[e]) for e in range(108)] == edges
    tab = BoneTable(edges, gd.PoseTransforms.part_roots(True))
    assert (tab.inc_ptr, tab.inc_edge) == (ptr, inc)
    kids = {k: tab.child_idx[tab.child_ptr[k]:tab.child_ptr[k + 1]] for k in range(121)}
    assert kids[gd.HAND_ROOT_L] == list(range(79, 100)) and kids[gd.HAND_ROOT_R] == list(range(100, 121))
    assert kids[gd.HEAD_ROOT] == [k for k in range(9, 79) if k != gd.HEAD_ROOT] and sum(len(v) for v in kids.values()) == 111
    empty = BoneTable([], [-1, -1])
    assert empty.E == 0 and empty.inc_ptr == [0, 0, 0] and empty.inc_edge == []
    for bad in (dict(edges=[(0, 3)], root=[-1] * 3), dict(edges=[(1, 1)], root=[-1] * 3), dict(edges=[(-1, 0)], root=[-1] * 3),
                dict(edges=[(0, 1)], root=[-1, 2, 0]),           # root 2 is itself in a part
                dict(edges=[(0, 1)], root=[-1, 1, -1]),          # its own root
                dict(edges=[(0, 1)], root=[-1, 3, -1]), dict(edges=[(0, 1)], root=[-1] * 257), dict(edges=[(0, 1)] * 513, root=[-1] * 3),
                dict(edges=[(0, 1)], root=[-1] * 3, edge_w=[-1.0]), dict(edges=[(0, 1)], root=[-1] * 3, edge_w=[1.0, 1.0]),
                dict(edges=[(0, 1)], root=[-1] * 3, edge_w=[float("nan")])):
        with pytest.raises(ValueError, match="BoneTable"):
            BoneTable(**bad)


# three keypoints in a chain, mean 1 and std 2 (the normalised values below are exact):
#   prediction (0,0) (3,4) (3,10): limbs (3,4) and (0,6), lengths 5 and 6;  truth (0,0) (0,10) (8,10): limbs (0,10) and (8,0), lengths 10 and 8
def _chain():
    P = torch.tensor([[0.0, 3.0, 3.0], [0.0, 4.0, 10.0]])
    Q = torch.tensor([[0.0, 0.0, 8.0], [0.0, 10.0, 10.0]])
    mean, std = torch.full((1, 6), 1.0, dtype=torch.float64), torch.full((1, 6), 2.0, dtype=torch.float64)
    return ((P - 1) / 2).reshape(1, 1, 2, 3), ((Q - 1) / 2).reshape(1, 1, 2, 3), mean, std, [(0, 1), (1, 2)], [-1, -1, -1]


def test_f64_model_on_a_three_keypoint_chain():
    pred, gt, mean, std, edges, root = _chain()
    bone, bdir = bone_loss_f64(pred, gt, mean, std, edges, root)
    assert float(bone) == (5 / 10 + 2 / 8) / 2 and abs(float(bdir) - (0.2 + 1.0) / 2) < 1e-15  # cos 40 / 50 and 0
    bone, bdir = bone_loss_f64(pred, gt, mean, std, edges, root, edge_w=[2.0, 4.0], lam_bone=3.0, lam_dir=0.0, min_len=16.0)
    assert float(bone) == 3.0 * (2 * 5 / 16 + 4 * 2 / 16) / 2 and float(bdir) == 0.0  # both true limbs under the floor
    # length term alone: both limbs too short, so each pulls its far end outwards along itself
    grad, terms = bone_grad_f64(pred, gt, mean, std, edges, root, lam_dir=0.0)
    want = torch.tensor([[0.06, -0.06, 0.0], [0.08, -0.08 + 0.125, -0.125]], dtype=torch.float64).reshape(1, 1, 2, 3)
    assert torch.allclose(grad, want, rtol=0, atol=1e-16)
    assert torch.allclose(terms, torch.tensor([[0.06, 0.06, 0.0], [0.08, 0.205, 0.125]], dtype=torch.float64).reshape(1, 1, 2, 3), rtol=0, atol=1e-16)
    # a score below the threshold at keypoint 2 (x alone) kills the second limb: the first is all that is left
    score = torch.ones(1, 1, 2, 3)
    score[0, 0, 0, 2] = 0.3
    bone, bdir = bone_loss_f64(pred, gt, mean, std, edges, root, score=score, min_conf=0.3)
    assert float(bone) == 0.5 and abs(float(bdir) - 0.2) < 1e-15


def _random(B, T, K, seed):
    gen = torch.Generator().manual_seed(seed)
    pred, gt = torch.randn(B, T, 2, K, generator=gen), torch.randn(B, T, 2, K, generator=gen)
    mean = 20.0 * torch.randn(B, 2 * K, generator=gen, dtype=torch.float64)
    std = 2.0 + 28.0 * torch.rand(B, 2 * K, generator=gen, dtype=torch.float64)
    score = torch.rand(B, T, 1, K, generator=gen).expand(B, T, 2, K).contiguous()
    return pred, gt, mean, std, score


def test_analytic_gradient_is_autograd_of_the_model():
    T = gd.PoseTransforms
    pred, gt, mean, std, score = _random(2, 3, 121, 0)
    edges, root = T.skeleton_edges(), T.part_roots(True)
    w = [(1.0, 0.5, 2.0)[T.part_table()[a]] for a, _ in edges]
    for sc, mc in ((None, None), (score, 0.3)):
        p = pred.double().requires_grad_(True)
        bone, bdir = bone_loss_f64(p, gt, mean, std, edges, root, sc, mc, w, 0.7, 0.3, 1.0)
        (0.75 * bone + 1.5 * bdir).backward()
        grad, terms = bone_grad_f64(pred, gt, mean, std, edges, root, sc, mc, w, 0.7, 0.3, 1.0, 0.75, 1.5)
        assert bool((p.grad != 0).any()) and bool(((grad - p.grad).abs() <= 1e-12 * terms).all())
        assert not grad[terms == 0].any() and not p.grad[terms == 0].any()


def test_hierarchical_against_global_on_an_edge_that_crosses_a_part():
    """(6, 79): the left wrist to the first point of its hand.  With hierarchical poses keypoint 79 is stored relative to 6, so the limb is
    P[79] alone and the wrist gets no gradient; fed the same skeleton in global coordinates the model gives the same losses, the same
    gradient at 79 and its opposite at 6."""
    T = gd.PoseTransforms
    gen = torch.Generator().manual_seed(1)
    pred = torch.round(torch.randn(2, 3, 2, 121, generator=gen) * 64) / 64  # (sums of two of these are exact in fp32)
    gt = torch.round(torch.randn(2, 3, 2, 121, generator=gen) * 64) / 64
    mean, std = torch.zeros(2, 242, dtype=torch.float64), torch.ones(2, 242, dtype=torch.float64)
    pg, gg = pred.clone(), gt.clone()
    pg[..., 79] += pred[..., 6]
    gg[..., 79] += gt[..., 6]
    edges = [(6, 79)]
    h = bone_loss_f64(pred, gt, mean, std, edges, T.part_roots(True))
    n = bone_loss_f64(pg, gg, mean, std, edges, T.part_roots(False))
    assert float(h[0]) == float(n[0]) and float(h[1]) == float(n[1]) and float(h[0]) > 0 and float(h[1]) > 0
    gh, th = bone_grad_f64(pred, gt, mean, std, edges, T.part_roots(True))
    gn, _ = bone_grad_f64(pg, gg, mean, std, edges, T.part_roots(False))
    assert torch.equal(gh[..., 79], gn[..., 79]) and torch.equal(gn[..., 6], -gn[..., 79]) and bool(gn[..., 79].any())
    assert not gh[..., 6].any() and bool((th[..., 6] > 0).all())  # +g - g: an exact 0 that is a sum of two terms


def test_nothing_under_the_mask_leaks_from_the_model():
    T = gd.PoseTransforms
    pred, gt, mean, std, score = _random(2, 3, 121, 2)
    edges, root = T.skeleton_edges(), T.part_roots(True)
    dead = ~(score > 0.3)
    base = bone_loss_f64(pred, gt, mean, std, edges, root, score, 0.3) + bone_grad_f64(pred, gt, mean, std, edges, root, score, 0.3)
    for junk in (1e6, float("nan")):
        p2, g2 = pred.clone(), gt.clone()
        p2[dead], g2[dead] = junk, junk
        p = p2.double().requires_grad_(True)
        bone, bdir = bone_loss_f64(p, g2, mean, std, edges, root, score, 0.3)
        (bone + bdir).backward()
        got = (bone.detach(), bdir.detach()) + bone_grad_f64(p2, g2, mean, std, edges, root, score, 0.3)
        assert all(torch.equal(x, y) for x, y in zip(got, base))
        assert torch.isfinite(p.grad).all() and bool((p.grad - base[2]).abs().max() <= 1e-12 * base[3].max())
    # a masked root takes its whole part with it
    s2 = torch.ones_like(score)
    s2[..., gd.HAND_ROOT_L] = 0.0
    grad, _ = bone_grad_f64(pred, gt, mean, std, edges, root, s2, 0.3)
    assert not grad[..., 79:100].any() and not grad[..., gd.HAND_ROOT_L].any() and bool(grad[..., 100:121].any())
    assert bool(bone_grad_f64(pred, gt, mean, std, edges, T.part_roots(False), s2, 0.3)[0][..., 79:100].any())


def test_degenerate_limbs_give_finite_gradients():
    pred, gt, mean, std, edges, root = _chain()
    mean, std = torch.zeros_like(mean), torch.ones_like(std)

    def both(p, g):
        pl = p.double().requires_grad_(True)
        bone, bdir = bone_loss_f64(pl, g, mean, std, edges, root)
        (bone + bdir).backward()
        grad, terms = bone_grad_f64(p, g, mean, std, edges, root)
        assert torch.isfinite(pl.grad).all() and torch.isfinite(grad).all() and bool((grad - pl.grad).abs().max() <= 1e-15)
        return float(bone.detach()), float(bdir.detach()), grad, terms

    # lp = 0 on the first limb: its length error is |0 - lg| / lg = 1 with a gradient of exactly 0, and it has no direction
    p0 = pred.clone()
    p0[..., 1] = p0[..., 0]
    bone, bdir, grad, terms = both(p0, gt)
    lg = [float(torch.linalg.vector_norm(gt[0, 0, :, k + 1].double() - gt[0, 0, :, k].double())) for k in range(2)]
    lp1 = float(torch.linalg.vector_norm(p0[0, 0, :, 2].double() - p0[0, 0, :, 1].double()))
    assert abs(bone - (1.0 + abs(lp1 - lg[1]) / lg[1]) / 2) < 1e-15 and not grad[..., 0].any() and terms[..., 0].sum() == 0
    assert bool(grad[..., 2].any())
    # lg = 0 on the first limb: the divisor is the floor, the direction term leaves it out (md counts one limb, not two)
    g0 = gt.clone()
    g0[..., 1] = g0[..., 0]
    bone, bdir, grad, _ = both(pred, g0)
    bone1, bdir1 = bone_loss_f64(pred, g0, mean, std, edges[1:], root)
    lp0 = float(torch.linalg.vector_norm(pred[0, 0, :, 1].double() - pred[0, 0, :, 0].double()))
    assert abs(bone - (lp0 / 1.0 + float(bone1)) / 2) < 1e-15 and bdir == float(bdir1) and bool(grad[..., 0].any())
    # pred == gt bitwise: both losses' terms are 0 (the length term exactly) and so is the gradient, exactly
    bone, bdir, grad, terms = both(gt.clone(), gt)
    assert bone == 0.0 and abs(bdir) < 1e-15 and not grad.any() and not terms.any()
    # no edges at all, and everything masked: 0 / max(0, 1)
    assert [float(x) for x in bone_loss_f64(pred, gt, mean, std, [], root)] == [0.0, 0.0]
    assert [float(x) for x in bone_loss_f64(pred, gt, mean, std, edges, root, torch.zeros_like(pred), 0.5)] == [0.0, 0.0]
    assert not bone_grad_f64(pred, gt, mean, std, edges, root, torch.zeros_like(pred), 0.5)[0].any()
