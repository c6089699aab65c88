"""The clip-code figure on the GPU (csrc/code_pca.hip, code_pca.py): fit and projection against scikit-learn's
float64 PCA (tests/golden/code_pca_reference.npz), the raster against the contract recomputed by numpy from the device's own
coordinates (exact), determinism, the loud failures, and the pipeline wiring (SYS.EPOCH_FIGURES on and off, the CLI).

The bar of every compared quantity: 100 x the error the float64 numpy restatement of the same algorithm has against the same fixture
(profiles/r08_code_pca_host_error.txt, recorded by tests/test_code_pca_host.py) -- the kernels differ from the restatement by
summation order only -- with a floor of 1e-12 x the quantity's largest magnitude, so that an exactly-zero host error (the mean) stays
passable.  The measured figures of every case are printed before each assertion (profiles/r08_test_code_pca_gpu.txt).
"""
import glob
import logging
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from test_code_pca_host import (QUANTITIES, axis_limits, contract_counts, contract_image, errors_against_fixture, read_host_errors)

sys.path.insert(0, GOLDEN)
import synth_code_tables as S  # noqa: E402

pytestmark = pytest.mark.gpu

GPU_FACTOR, GPU_FLOOR = 100.0, 1e-12


def CP():
    from speechdrivestemplates_amd import code_pca
    return code_pca


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# -- (a) fit and projection ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(S.CASES))
def test_fit_project_matches_scikit_learn(case):
    table = S.case_table(case)
    fit = CP().fit_project(dev(table))  # the (N, F, D) case goes in as it is
    n = int(np.prod(table.shape[:-1]))
    assert fit["X"].shape == (n, 2) and fit["X"].dtype == torch.float64 and fit["X"].is_cuda
    assert fit["n_rows"] == n and fit["dim"] == table.shape[-1] and 1 <= fit["sweeps"] <= 12
    X = fit["X"].cpu().numpy()
    rec = read_host_errors()
    for q, (err, scale) in errors_against_fixture(case, dict(fit, X=X)).items():
        bar = max(GPU_FACTOR * rec[(case, q)], GPU_FLOOR * scale)
        print("code_pca %s %s: gpu error %.3e, host restatement %.3e, bar %.3e (scale %.4g, %d sweeps, off %.2e)"
              % (case, q, err, rec[(case, q)], bar, scale, fit["sweeps"], fit["offdiag"]))
        assert err <= bar, "%s %s: %.3e > %.3e" % (case, q, err, bar)
    # signs are part of the result: the entry of largest magnitude of each component is positive
    c = fit["components"]
    assert (c[np.arange(2), np.abs(c).argmax(axis=1)] > 0).all()
    # the device's min / max are exact and its axis limits are the contract's arithmetic on them
    assert fit["minmax"] == (X[:, 0].min(), X[:, 0].max(), X[:, 1].min(), X[:, 1].max())
    assert fit["limits"] == axis_limits(*fit["minmax"][:2]) + axis_limits(*fit["minmax"][2:])
    assert np.array_equal(fit["eigenvalues"], np.sort(fit["eigenvalues"])[::-1]) and np.array_equal(fit["explained_variance"], fit["eigenvalues"][:2])
    if case == "constcol":
        assert fit["components"][:, S.CONST_COL].tolist() == [0.0, 0.0] and fit["mean"][S.CONST_COL] == np.float64(np.float32(S.CONST_VALUE))


# -- (b) raster, exact -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,canvas,marker", [("n4096", (480, 640), 2), ("n100000", (480, 640), 2), ("d64", (480, 640), 1),
                                                ("n300", (100, 131), 3), ("frames", (64, 48), 5), ("n100000", (960, 1600), 2),
                                                ("n100000", (64, 80), 4)])
def test_raster_equals_the_contract_on_the_device_coordinates(case, canvas, marker):
    cp = CP()
    fit = cp.fit_project(dev(S.case_table(case)))
    image, counts = cp.render_scatter(fit["X"], fit["limits"], canvas=canvas, marker_px=marker, return_counts=True)
    ph, pw = cp.plot_rectangle(canvas)
    assert image.shape == canvas + (3,) and image.dtype == torch.uint8 and counts.shape == (ph, pw)
    ref = contract_counts(fit["X"].cpu().numpy(), fit["limits"], ph, pw, marker)
    assert ref.sum() > 0.9 * fit["n_rows"] * marker * marker  # (only markers at the rectangle's edge lose pixels)
    assert np.array_equal(counts.cpu().numpy(), ref)
    table = cp.colour_table()
    assert ref.max() >= (len(table) if canvas == (64, 80) else 1)  # 1.6 million increments on 2240 pixels: counts past the table are clamped
    assert np.array_equal(image.cpu().numpy(), contract_image(ref, table, canvas))


def test_raster_skips_points_outside_the_limits_and_takes_other_colours():
    cp = CP()
    X = dev(np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 0.5], [np.nan, 0.5], [0.5, -0.1], [0.25, 0.75]]))
    limits = (0.0, 1.0, 0.0, 1.0)
    image, counts = cp.render_scatter(X, limits, canvas=(40, 50), marker_px=1, alpha=0.5, colour=(200, 10, 0), return_counts=True)
    ref = contract_counts(X.cpu().numpy(), limits, 16, 26, 1)
    assert ref.sum() == 3 and np.array_equal(counts.cpu().numpy(), ref)
    assert np.array_equal(image.cpu().numpy(), contract_image(ref, cp.colour_table(0.5, (200, 10, 0)), (40, 50)))
    with pytest.raises(ValueError):
        cp.render_scatter(X, (0.0, 0.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        cp.render_scatter(X, limits, canvas=(24, 24))
    with pytest.raises(RuntimeError, match="marker_px"):
        cp.render_scatter(X, limits, marker_px=0)


# -- (c) determinism ---------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    cp = CP()
    t = dev(S.case_table("n100000"))
    a, b = cp.fit_project(t), cp.fit_project(t)
    assert torch.equal(a["X"], b["X"]) and a["limits"] == b["limits"]
    for k in ("mean", "components", "eigenvalues"):
        assert np.array_equal(a[k], b[k]), k
    assert torch.equal(cp.clip_code_figure(t), cp.clip_code_figure(t))


# -- (d) loud failures -------------------------------------------------------------------------------------------------------------
def test_loud_failures():
    cp = CP()
    t = S.case_table("n4096")
    for row, col, bad in ((1234, 5, np.nan), (4095, 31, np.inf), (0, 0, -np.inf)):
        u = t.copy()
        u[row, col] = bad
        u[min(row + 7, 4095), 3] = np.nan  # a later bad row does not change the one that is named
        with pytest.raises(ValueError, match=r"non-finite entry in row %d$" % row):
            cp.fit_project(dev(u))
    with pytest.raises(ValueError, match="at least 2 rows"):
        cp.fit_project(dev(t[:1]))
    with pytest.raises(ValueError, match=r"outside \[2, 64\]"):
        cp.fit_project(torch.zeros(100, 65, device="cuda"))
    with pytest.raises(ValueError, match=r"outside \[2, 64\]"):
        cp.fit_project(torch.zeros(100, 1, device="cuda"))
    with pytest.raises(TypeError):
        cp.fit_project(dev(t.astype(np.float64)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cp.fit_project(torch.from_numpy(t))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cp.render_scatter(torch.zeros(4, 2, dtype=torch.float64), (0, 1, 0, 1))
    with pytest.raises(ValueError, match="no variance"):
        cp.fit_project(torch.full((50, 32), 0.5, device="cuda"))
    with pytest.raises(RuntimeError, match="did not converge in 1 sweeps"):  # the error word, never a silently unconverged result
        cp.fit_project(dev(t), max_sweeps=1)
    assert cp.fit_project(dev(t[:2]))["explained_variance_ratio"][0] == pytest.approx(1.0, abs=1e-12)  # two rows: one direction


# -- (e) pipelines -----------------------------------------------------------------------------------------------------------------
def _train_cfg(tmp_path, name, figures):
    from speechdrivestemplates_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(REPO, "configs", name + ".yaml"))
    opts = ["DATASET.NAME", "SyntheticGestureDataset", "DATASET.SYNTHETIC_CLIPS", 8, "TRAIN.BATCH_SIZE", 4, "TEST.BATCH_SIZE", 4,
            "TRAIN.NUM_EPOCHS", 2, "SYS.NUM_WORKERS", 0, "SYS.LOG_INTERVAL", 100, "SYS.OUTPUT_DIR", str(tmp_path),
            "TRAIN.SAVE_VIDEO", False, "TEST.SAVE_VIDEO", False, "TEST.SAVE_NPZ", False, "TRAIN.VALIDATE", False]
    if figures:
        opts += ["SYS.EPOCH_FIGURES", True]
    cfg.merge_from_list(opts)
    cfg.freeze()
    return cfg


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB")), dict(im.text)


@pytest.mark.parametrize("name,key", [("voice2pose_sdt_bp", "clips_code"), ("pose2pose", "clip_code_mu")])
def test_train_writes_the_figure_of_every_epoch(tmp_path, caplog, capsys, name, key):
    from speechdrivestemplates_amd.core.pipelines import get_pipeline
    cp = CP()
    torch.manual_seed(5)
    cfg = _train_cfg(tmp_path, name, True)
    pipe = get_pipeline(cfg.PIPELINE_TYPE)(cfg)
    with caplog.at_level(logging.INFO):
        pipe.train(cfg, "f", None)
    base = glob.glob(str(tmp_path / "*_f"))[0]
    assert sorted(os.listdir(os.path.join(base, "figures"))) == ["epoch1-clip_code.png", "epoch2-clip_code.png"]
    codes = getattr(pipe.model, key).detach()
    assert codes.shape == (8, 32)
    expect, meta = cp.clip_code_figure(codes, return_meta=True)  # nothing has moved the table since the last epoch's figure
    pixels, text = _png(os.path.join(base, "figures", "epoch2-clip_code.png"))
    assert pixels.shape == (480, 640, 3) and np.array_equal(pixels, expect.cpu().numpy())
    assert eval(text["explained_variance_ratio"]) == meta["explained_variance_ratio"] and eval(text["limits"]) == meta["limits"]
    assert not np.array_equal(pixels, _png(os.path.join(base, "figures", "epoch1-clip_code.png"))[0])  # the table moved in between
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("[TRAIN] epoch plotting: Clip Code, evr=(")]
    assert len(lines) == 2 and lines[1].rstrip().endswith(cp.describe(meta)), lines
    # the CLI on the checkpoint of the last epoch draws the same picture (and finds the table by itself)
    ckpt = sorted(glob.glob(os.path.join(base, "checkpoints", "checkpoint_epoch-2_*.pth")))[0]
    out = str(tmp_path / "cli" / "fig.png")
    assert cp.main(["--checkpoint", ckpt, "--out", out]) == 0
    assert np.array_equal(_png(out)[0], pixels) and _png(out)[1]["key"] == repr("module." + key)
    assert cp.describe(meta) in capsys.readouterr().out
    out2 = str(tmp_path / "cli" / "small.png")
    assert cp.main(["--checkpoint", ckpt, "--out", out2, "--key", "module." + key, "--canvas", "120x160", "--marker-px", "3"]) == 0
    assert np.array_equal(_png(out2)[0], cp.clip_code_figure(codes, canvas=(120, 160), marker_px=3).cpu().numpy())
    pipe.close()


def test_train_default_writes_no_figures(tmp_path, caplog):
    from speechdrivestemplates_amd.core.pipelines import get_pipeline
    cfg = _train_cfg(tmp_path, "pose2pose", False)
    pipe = get_pipeline(cfg.PIPELINE_TYPE)(cfg)
    with caplog.at_level(logging.INFO):
        pipe.train(cfg, "f", None)
    pipe.close()
    base = glob.glob(str(tmp_path / "*_f"))[0]
    assert not os.path.exists(os.path.join(base, "figures"))
    assert not any("epoch plotting" in r.getMessage() for r in caplog.records)


def test_external_codes_and_pipelines_without_a_table():
    sys.path.insert(0, REPO)
    from __graft_entry__ import make_pipeline
    from speechdrivestemplates_amd.core.pipelines.trainer import Trainer
    cp = CP()
    pipe, cfg = make_pipeline("voice2pose_sdt_vae", 16)  # external, plain-tensor codes (not a Parameter, not moved by .cuda())
    assert cfg.VOICE2POSE.GENERATOR.CLIP_CODE.EXTERNAL_CODE and not isinstance(pipe.model.clips_code, torch.nn.Parameter)
    codes = pipe.model.clips_code.clone()
    fig = pipe.draw_figure_epoch()
    assert list(fig) == ["clip_code"] and torch.equal(fig["clip_code"], cp.clip_code_figure(codes.cuda()))
    assert pipe.figure_meta["clip_code"]["n_rows"] == 16
    pipe.close()
    pipe, cfg = make_pipeline("voice2pose_s2g", 8)  # no clip codes at all
    assert cfg.VOICE2POSE.GENERATOR.CLIP_CODE.DIMENSION is None and pipe.draw_figure_epoch() == {}
    pipe.close()
    assert Trainer.draw_figure_epoch(pipe) == {}
