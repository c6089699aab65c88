"""Optimiser-side safeguards, host side (no GPU): the config keys, the EVAL_WITH_EMA precondition, and the numpy contract model of
the kernel's ordered float64 sum of squares (optim.sumsq_model) against math.fsum."""
import math

import numpy as np
import pytest

from speechdrivestemplates_amd import _lib, optim
from speechdrivestemplates_amd.config import check_optim_guard, get_cfg_defaults


def test_keys_exist_with_their_defaults():
    cfg = get_cfg_defaults()
    assert cfg.TRAIN.GRAD_CLIP_NORM is None
    assert cfg.TRAIN.SKIP_NONFINITE_STEP is False
    assert cfg.TRAIN.EMA_DECAY is None
    assert cfg.SYS.EVAL_WITH_EMA is False
    check_optim_guard(cfg)  # the defaults are a valid configuration
    cfg.merge_from_list(["TRAIN.GRAD_CLIP_NORM", "0.5", "TRAIN.SKIP_NONFINITE_STEP", "True", "TRAIN.EMA_DECAY", "0.999", "SYS.EVAL_WITH_EMA", "True"])
    assert cfg.TRAIN.GRAD_CLIP_NORM == 0.5 and cfg.TRAIN.SKIP_NONFINITE_STEP is True and cfg.TRAIN.EMA_DECAY == 0.999
    check_optim_guard(cfg)


def test_eval_with_ema_without_an_ema_source_raises():
    cfg = get_cfg_defaults()
    cfg.merge_from_list(["SYS.EVAL_WITH_EMA", True])
    with pytest.raises(ValueError, match="EVAL_WITH_EMA.*EMA_DECAY"):
        check_optim_guard(cfg)
    check_optim_guard(cfg, checkpoint_has_ema=True)  # a checkpoint that carries an EMA is a source
    cfg.merge_from_list(["TRAIN.EMA_DECAY", 0.99])
    check_optim_guard(cfg)


@pytest.mark.parametrize("key,bad", [("TRAIN.GRAD_CLIP_NORM", 0.0), ("TRAIN.GRAD_CLIP_NORM", -1.0), ("TRAIN.EMA_DECAY", 1.0),
                                     ("TRAIN.EMA_DECAY", 0.0), ("TRAIN.EMA_DECAY", True)])
def test_out_of_range_values_raise(key, bad):
    cfg = get_cfg_defaults()
    cfg.merge_from_list([key, bad])
    with pytest.raises(ValueError, match=key.split(".")[1]):
        check_optim_guard(cfg)


def test_model_constants_are_the_librarys():
    lib = _lib.load()
    assert lib.sdt_grad_sumsq_partials() == 1 + optim.SUMSQ_MAX_BLOCKS
    assert lib.sdt_optim_guard_pass_elems(0) == optim.SUMSQ_MAX_BLOCKS * optim.SUMSQ_THREADS * 4


# one more than a full block of float4s; one more than a grid pass (second trip of the thread loop); a size with a second trip of the
# FINAL block's loop would need > 256 * 256 * 4 * ... elements per block count: covered by the pass size (2048 blocks = 8 final trips)
PASS = optim.SUMSQ_MAX_BLOCKS * optim.SUMSQ_THREADS * 4


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1025, 300001, PASS + 1])
def test_contract_model_against_fsum(n):
    """All squares are exact in float64 and non-negative, so the model's relative error is bounded by gamma_k = k u / (1 - k u),
    u = 2^-53, k = the most additions any one square passes through: the longest serial run of a thread plus the tree depths
    (optim.sumsq_model_depth states them).  For the sizes here k <= 41: a bound of at most 4.6e-15."""
    rng = np.random.Generator(np.random.PCG64(n))
    g = (rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))).astype(np.float32)
    g[0], g[-1] = np.float32(1e-30), np.float32(1e19)  # squares that underflow / overflow fp32
    exact = math.fsum(float(x) * float(x) for x in g)  # each product is exact in float64
    k = optim.sumsq_model_depth(n)
    assert k <= 41
    u = 2.0 ** -53
    bound = k * u / (1 - k * u)
    got = float(optim.sumsq_model(g))
    print("n=%d depth=%d rel err %.3e bound %.3e" % (n, k, abs(got - exact) / exact, bound))
    assert abs(got - exact) <= bound * exact


def test_contract_model_flags_any_non_finite_element():
    for bad in (np.nan, np.inf, -np.inf):
        for n, pos in ((5, 0), (5, 3), (5, 4), (1029, 1023), (1029, 1028)):
            g = np.ones(n, dtype=np.float32)
            g[pos] = bad
            assert not np.isfinite(optim.sumsq_model(g))
    assert optim.sumsq_model(np.full(7, 3e38, dtype=np.float32)) == 7 * np.float64(np.float32(3e38)) ** 2  # no overflow in float64
