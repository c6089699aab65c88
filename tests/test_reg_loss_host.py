"""Host side of the masked / part-weighted / velocity regression loss (VOICE2POSE.GENERATOR.LAMBDA_VEL, REG_MIN_CONFIDENCE,
REG_PART_WEIGHTS): the config keys and their validation, the keypoint part table, and ``reg_loss_f64`` -- the
float64 torch model of the contract that tests/test_reg_loss_gpu.py compares the kernels with.  No GPU."""
import pytest
import torch
from torch import nn

from speechdrivestemplates_amd.config import check_reg_loss, get_cfg_defaults
from speechdrivestemplates_amd.core.datasets import gesture_dataset as gd


def reg_loss_f64(pred, gt, score=None, min_conf=None, chan_w=None, lam_reg=1.0, lam_vel=0.0):
    """(reg, vel) of DESIGN.md section 21 in float64, differentiable in ``pred`` (torch.sign semantics: sign(0) = 0).
    pred, gt, score: (B, T, ...) of one shape; chan_w: one weight per trailing element of a frame (None: 1); the comparison
    ``score > min_conf`` is made in the score's own precision.  Masked elements are replaced BEFORE the arithmetic (torch.where), so
    a NaN under the mask cannot reach a sum or a gradient."""
    B, T = pred.shape[0], pred.shape[1]
    e = pred.double().reshape(B, T, -1) - gt.double().reshape(B, T, -1)
    if score is not None and min_conf is not None:
        m = (score.reshape(B, T, -1) > min_conf)
    else:
        m = torch.ones_like(e, dtype=torch.bool)
    w = torch.ones(e.shape[2], dtype=torch.float64) if chan_w is None else chan_w.double().reshape(-1)
    w = w.to(e.device)
    zero = torch.zeros((), dtype=torch.float64, device=e.device)
    reg = lam_reg * (torch.where(m, e, zero).abs() * w).sum() / max(int(m.sum()), 1)
    m2 = m[:, 1:] & m[:, :-1]
    e_hi, e_lo = torch.where(m2, e[:, 1:], zero), torch.where(m2, e[:, :-1], zero)
    vel = lam_vel * ((e_hi - e_lo).abs() * w).sum() / max(int(m2.sum()), 1)
    return reg, vel


def _cfg(**gen):
    cfg = get_cfg_defaults()
    opts = []
    for k, v in gen.items():
        opts += ["VOICE2POSE.GENERATOR." + k, v]
    cfg.merge_from_list(opts)
    cfg.freeze()
    return cfg


def test_defaults_are_the_plain_l1_mean():
    g = get_cfg_defaults().VOICE2POSE.GENERATOR
    assert g.LAMBDA_VEL == 0.0 and g.REG_MIN_CONFIDENCE is None and g.REG_PART_WEIGHTS is None
    assert check_reg_loss(get_cfg_defaults()) is None
    assert check_reg_loss(_cfg(LAMBDA_VEL=0.5)) == (0.5, None, None)
    assert check_reg_loss(_cfg(REG_MIN_CONFIDENCE=0)) == (0.0, 0.0, None)
    assert check_reg_loss(_cfg(REG_PART_WEIGHTS=[1, 0.5, 2])) == (0.0, None, (1.0, 0.5, 2.0))
    assert check_reg_loss(_cfg(REG_PART_WEIGHTS="[0, 1, 1]")) == (0.0, None, (0.0, 1.0, 1.0))  # (a command-line override arrives as a string)


@pytest.mark.parametrize("key,value", [
    ("LAMBDA_VEL", -0.1), ("REG_PART_WEIGHTS", [1.0, -1.0, 1.0]),                      # a negative number
    ("REG_PART_WEIGHTS", [1.0, 1.0]), ("REG_PART_WEIGHTS", [1.0, 1.0, 1.0, 1.0]),      # a wrong length
    ("LAMBDA_VEL", "fast"), ("LAMBDA_VEL", None), ("LAMBDA_VEL", True), ("LAMBDA_VEL", float("nan")),  # not a number
    ("REG_MIN_CONFIDENCE", "high"), ("REG_MIN_CONFIDENCE", [0.1]), ("REG_MIN_CONFIDENCE", float("inf")),
    ("REG_PART_WEIGHTS", [1.0, "x", 1.0]), ("REG_PART_WEIGHTS", 2.0), ("REG_PART_WEIGHTS", [1.0, None, 1.0]),
])
def test_bad_values_raise_and_name_the_key(key, value):
    with pytest.raises(ValueError, match="VOICE2POSE.GENERATOR." + key):
        check_reg_loss(_cfg(**{key: value}))


def test_model_construction_rejects_bad_values():
    from speechdrivestemplates_amd.core.pipelines.voice2pose import Voice2PoseModel
    with pytest.raises(ValueError, match="VOICE2POSE.GENERATOR.REG_PART_WEIGHTS"):
        Voice2PoseModel(_cfg(REG_PART_WEIGHTS=[1.0, 2.0]), num_train_samples=4)
    with pytest.raises(ValueError, match="VOICE2POSE.GENERATOR.LAMBDA_VEL"):
        Voice2PoseModel(_cfg(LAMBDA_VEL=-1.0), num_train_samples=4)


def test_part_table():
    T = gd.PoseTransforms
    parts = T.part_table()
    assert len(parts) == 121 and set(parts) == {T.BODY, T.FACE, T.HANDS}  # a list: each keypoint is in exactly one part
    assert [k for k, p in enumerate(parts) if p == T.BODY] == list(range(0, 9))
    assert [k for k, p in enumerate(parts) if p == T.FACE] == list(range(9, 79))
    assert [k for k, p in enumerate(parts) if p == T.HANDS] == list(range(79, 121))
    # _part_index: the keypoints that hang off the head root are face, those off a wrist are hands; the roots: head root is face, wrists are body
    sel, root = T._part_index("cpu")
    for k, r in zip(sel.tolist(), root.tolist()):
        assert parts[k] == (T.FACE if r == gd.HEAD_ROOT else T.HANDS), (k, r)
    assert parts[gd.HEAD_ROOT] == T.FACE and parts[gd.HAND_ROOT_L] == T.BODY and parts[gd.HAND_ROOT_R] == T.BODY
    assert sorted(sel.tolist() + [gd.HEAD_ROOT]) == [k for k, p in enumerate(parts) if p != T.BODY]


def test_f64_model_is_the_reference_mean_without_options():
    gen = torch.Generator().manual_seed(3)
    p, g = torch.randn(3, 5, 2, 7, generator=gen), torch.randn(3, 5, 2, 7, generator=gen)
    lam = 0.75
    reg, vel = reg_loss_f64(p, g, lam_reg=lam)
    ref = (nn.L1Loss(reduction='none')(p.double(), g.double()) * lam).mean()  # voice2pose.py:141-142
    assert abs(float(reg) - float(ref)) <= p.numel() * 2.0 ** -53 * abs(float(ref)) and float(vel) == 0.0  # (two float64 summation orders)
    assert abs(float(reg) - float(nn.L1Loss()(p, g) * lam)) <= 2.0 ** -20 * float(ref)  # (the fp32 mean itself)
    # unit weights and a mask that lets everything through change nothing
    reg2, _ = reg_loss_f64(p, g, score=torch.ones_like(p), min_conf=0.5, chan_w=torch.ones(14), lam_reg=lam)
    assert float(reg2) == float(reg)


def test_f64_model_terms():
    """hand-checked values: B = 1, T = 3, C = 2"""
    p = torch.tensor([[[1.0, 0.0], [3.0, 0.0], [2.0, 5.0]]])
    g = torch.zeros_like(p)
    s = torch.tensor([[[1.0, 1.0], [1.0, 0.5], [1.0, 1.0]]])
    reg, vel = reg_loss_f64(p, g, lam_reg=1.0, lam_vel=2.0)
    assert float(reg) == 11.0 / 6 and float(vel) == 2.0 * (2 + 0 + 1 + 5) / 4
    reg, vel = reg_loss_f64(p, g, score=s, min_conf=0.5, chan_w=torch.tensor([1.0, 10.0]), lam_reg=1.0, lam_vel=1.0)
    assert float(reg) == (1 + 3 + 2 + 10 * 5) / 5 and float(vel) == (2 + 1) / 2  # (1, 1) is masked (0.5 > 0.5 is false): both pairs of channel 1 die
    reg, vel = reg_loss_f64(p, g, score=s, min_conf=1.0, lam_vel=1.0)
    assert float(reg) == 0.0 and float(vel) == 0.0  # everything masked: 0 / max(0, 1)
    pn = p.clone().requires_grad_(True)
    gn = g.clone()
    gn[0, 1, 1] = float("nan")
    reg, vel = reg_loss_f64(pn, gn, score=s, min_conf=0.5, lam_vel=1.0)
    (reg + vel).backward()
    assert torch.isfinite(reg) and torch.isfinite(vel) and torch.isfinite(pn.grad).all() and float(pn.grad[0, 1, 1]) == 0.0
