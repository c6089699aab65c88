"""The template axes on the GPU (csrc/code_axes.hip, code_axes.py) against the numpy contract models of the same
file: bit for bit.  The device's Jacobi, projection, order statistics and search round every operation on its own in a fixed order, and
the models restate that order, so nothing here is compared by a tolerance except the moments: ``sdt_code_pca_moments`` (not new) sums
in per-workgroup partials, the host in numpy's order, and the bound of that comparison is the worst-case rounding of two N-term
float64 sums, 2 (N + 8) u per unit of the summed magnitudes (u = 2^-53), computed from the table.  The Jacobi model therefore starts
from the DEVICE's covariance.  Then the old two-component path (same bits), the edges, the loud failures, and both demo modes reading
the file the command line writes.
"""
import glob
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from test_code_pca_host import contract_moments

sys.path.insert(0, GOLDEN)
import synth_axes_tables as A  # noqa: E402
import synth_code_tables as S  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
_FITS = {}


def CA():
    from speechdrivestemplates_amd import code_axes
    return code_axes


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the fixture tables are read-only)


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def table_of(case):
    return S.make_table((70001, 4), 39) if case == "n70001_d4" else A.case_table(case)  # more tiles than the projection's grid has workgroups


def device_fit(case):
    if case not in _FITS:
        _FITS[case] = CA().fit_axes(dev(table_of(case)))
    return _FITS[case]


CASES = list(A.CASES) + ["n70001_d4"]


# -- (a) every stage against its model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_fit_axes_equals_the_models(case):
    ca = CA()
    t = table_of(case)
    n, d = t.shape
    fit = device_fit(case)
    assert fit["n_rows"] == n and fit["dim"] == d
    for k, shape in (("mean", (d,)), ("components", (d, d)), ("explained_variance", (d,)), ("explained_variance_ratio", (d,)), ("projections", (n, d))):
        assert fit[k].shape == shape and fit[k].dtype == torch.float64 and fit[k].is_cuda, k
    mean, cov = fit["mean"].cpu().numpy(), fit["covariance"].cpu().numpy()
    # the moments (the existing kernel): two orders of summation of the same terms
    ref_mean, ref_cov = contract_moments(t)
    x = t.astype(np.float64)
    mean_bound = 2 * (n + 8) * U * np.abs(x).sum(axis=0) / n
    sd = np.sqrt(np.diag(ref_cov))
    cov_bound = 2 * (n + 8) * U * np.outer(sd, sd) + 8 * np.outer(mean_bound, mean_bound)
    print("code_axes %s: mean error / bound %.3e, covariance error / bound %.3e" % (
        case, (np.abs(mean - ref_mean) / np.maximum(mean_bound, 1e-300)).max(), (np.abs(cov - ref_cov) / np.maximum(cov_bound, 1e-300)).max()))
    assert (np.abs(mean - ref_mean) <= mean_bound).all() and (np.abs(cov - ref_cov) <= cov_bound).all()
    # the decomposition: the model on the device's covariance, bit for bit
    lam, comps, sweeps, off = ca.model_components(cov)
    assert fit["sweeps"] == sweeps and fit["offdiag"] == off
    assert np.array_equal(bits(fit["explained_variance"]), bits(lam))
    assert np.array_equal(bits(fit["components"]), bits(comps))
    trace = float(np.cumsum(np.diag(cov))[-1])
    assert np.array_equal(bits(fit["explained_variance_ratio"]), bits(lam / trace))
    # the projection: the model on the device's mean and components, bit for bit
    assert np.array_equal(bits(fit["projections"]), bits(ca.model_project(t, mean, comps)))
    if case == "zeros_col":
        assert lam[-1] == 0.0 and (fit["projections"][:, -1] == 0).all()


@pytest.mark.parametrize("case", CASES)
def test_axis_quantiles_equal_the_model(case):
    ca = CA()
    fit = device_fit(case)
    P = fit["projections"].cpu().numpy()
    n = P.shape[0]
    got = ca.axis_quantiles(fit["projections"], A.QUANTILES).cpu().numpy()
    ref = ca.model_quantiles(P, ca.quantile_ranks(A.QUANTILES, n))
    assert got.shape == ref.shape == (P.shape[1], 5) and (got == ref).all()
    assert (got[:, 0] == P.min(axis=0)).all() and (got[:, 4] == P.max(axis=0)).all()  # ranks 0 and N - 1
    for k in (0, P.shape[1] - 1):
        assert got[k, 2] == np.quantile(P[:, k], 0.5, method="lower")


@pytest.mark.parametrize("case", CASES)
def test_nearest_codes_equal_the_model(case):
    ca = CA()
    t = table_of(case)
    q = A.case_queries(case) if case in A.CASES else np.random.Generator(np.random.PCG64(5)).standard_normal((3, t.shape[1]))
    index, dist2 = ca.nearest_codes(dev(t), dev(q))
    ref_index, ref_dist2 = ca.model_nearest(t, q)
    assert index.dtype == torch.int64 and index.shape == dist2.shape == (len(q),)
    assert np.array_equal(index.cpu().numpy(), ref_index) and np.array_equal(bits(dist2), bits(ref_dist2))
    if case == "dups":
        assert index.tolist() == [7]
    elif case in A.CASES:  # a query equal to a table row: that row, or a lower identical one, at distance zero
        assert dist2[9].item() == 0.0 and np.array_equal(t[index[9].item()], t[t.shape[0] // 2])


# -- (b) the old two-component path carries the same bits -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["n4096_d32", "n1000_d64"])
def test_fit_axes_against_fit_project(case):
    from speechdrivestemplates_amd import code_pca
    fit, old = device_fit(case), code_pca.fit_project(dev(A.case_table(case)))
    assert np.array_equal(bits(fit["components"][:2]), bits(old["components"]))
    assert np.array_equal(bits(fit["explained_variance"][:2]), bits(old["explained_variance"]))
    assert np.array_equal(bits(fit["explained_variance"]), bits(old["eigenvalues"]))
    assert np.array_equal(bits(fit["projections"][:, :2]), bits(old["X"]))
    assert np.array_equal(bits(fit["mean"]), bits(old["mean"])) and fit["sweeps"] == old["sweeps"] and fit["offdiag"] == old["offdiag"]
    assert np.array_equal(bits(fit["explained_variance_ratio"][:2]), bits(old["explained_variance_ratio"]))


# -- (c) edges ---------------------------------------------------------------------------------------------------------------------------
def test_order_statistics_keep_zeros_tiny_values_and_infinities_apart():
    ca = CA()
    P = A.signed_zero_projections()
    for first in range(0, 64, 16):  # every rank, 16 per call
        ranks = list(range(first, first + 16))
        got = ca.order_statistics(dev(P), ranks).cpu().numpy()
        ref = ca.model_quantiles(P, ranks)
        assert (got == ref).all()
        nz = ref[0] != 0.0
        assert np.array_equal(bits(got[0][nz]), bits(ref[0][nz]))  # everything but a zero is the stored value (a zero: either sign)
    assert ca.order_statistics(dev(P), [0]).tolist() == [[-np.inf], [0.0]] and ca.order_statistics(dev(P), [63]).tolist() == [[np.inf], [0.0]]


@pytest.mark.parametrize("nq", [1, 1000])
def test_nearest_with_one_query_and_with_many_row_chunks(nq):
    ca = CA()
    t = A.case_table("n4096_d32")  # 1000 queries: 125 query tiles, so two table tiles per row chunk; one query: one tile per chunk
    q = t[::4][:nq].astype(np.float64) + (0.05 * np.random.Generator(np.random.PCG64(6)).standard_normal((nq, 32)) if nq > 1 else 0.0)
    index, dist2 = ca.nearest_codes(dev(t), dev(q.reshape(nq, 32)))
    ref_index, ref_dist2 = ca.model_nearest(t, q)
    assert np.array_equal(index.cpu().numpy(), ref_index) and np.array_equal(bits(dist2), bits(ref_dist2))
    if nq == 1:
        assert index.tolist() == [0] and dist2.tolist() == [0.0]
    shaped = ca.nearest_codes(dev(t), dev(q.reshape(nq, 1, 32)))  # leading shape of the queries is kept
    assert shaped[0].shape == (nq, 1) and torch.equal(shaped[0].reshape(-1), index)


def test_two_rows():
    ca = CA()
    t = A.case_table("n2_d2")
    fit = device_fit("n2_d2")
    assert fit["explained_variance_ratio"][0].item() == pytest.approx(1.0, abs=1e-12)  # two rows: one direction
    got = ca.axis_quantiles(fit["projections"], [0.0, 0.5, 1.0]).cpu().numpy()
    P = fit["projections"].cpu().numpy()
    assert (got == np.stack([P.min(axis=0), P.min(axis=0), P.max(axis=0)], axis=1)).all()
    index, dist2 = ca.nearest_codes(dev(t), dev(t.astype(np.float64)))
    assert index.tolist() == [0, 1] and dist2.tolist() == [0.0, 0.0]


# -- (d) loud failures: argument checks and error words, never an out-of-range access ---------------------------------------------------
def test_loud_failures():
    ca = CA()
    t = A.case_table("n257_d33")
    q = A.case_queries("n257_d33")
    u = t.copy()
    u[123, 5] = np.nan
    u[200, 0] = np.inf  # a later bad row does not change the one that is named
    with pytest.raises(ValueError, match=r"non-finite entry in row 123$"):
        ca.fit_axes(dev(u))
    with pytest.raises(ValueError, match=r"non-finite entry in row 123$"):
        ca.nearest_codes(dev(u), dev(q))
    bad = q.copy()
    bad[5, 32] = np.nan
    bad[9, 0] = -np.inf
    with pytest.raises(ValueError, match=r"query 5 has a non-finite entry$"):
        ca.nearest_codes(dev(t), dev(bad))
    for shape in ((100, 1), (100, 65), (1, 32)):
        with pytest.raises(ValueError):
            ca.fit_axes(torch.zeros(shape, device="cuda"))
        with pytest.raises(ValueError):
            ca.nearest_codes(torch.zeros(shape, device="cuda"), torch.zeros((1, shape[1]), dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError):
            ca.axis_quantiles(torch.zeros(shape, dtype=torch.float64, device="cuda"), [0.5])
    with pytest.raises(RuntimeError, match="did not converge in 0 sweeps"):  # the error word, never a silently unconverged result
        ca.fit_axes(dev(t), max_sweeps=0)
    with pytest.raises(ValueError, match="no variance"):
        ca.fit_axes(torch.full((50, 32), 0.5, device="cuda"))
    P = device_fit("n257_d33")["projections"]
    for ranks in ([257], [-1], list(range(17)), []):
        with pytest.raises(ValueError):
            ca.order_statistics(P, ranks)
    with pytest.raises(ValueError):
        ca.nearest_codes(dev(t), torch.zeros((65537, 33), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ca.nearest_codes(dev(t), dev(q[:, :32]))
    with pytest.raises(TypeError):
        ca.fit_axes(dev(t.astype(np.float64)))


# -- (e) determinism -----------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    ca = CA()
    t = dev(A.case_table("n4096_d32"))
    a, b = ca.template_axes(t), ca.template_axes(t)
    for k in ("mean", "components", "explained_variance", "explained_variance_ratio", "projections"):
        assert np.array_equal(bits(a[0][k]), bits(b[0][k])), k
    assert np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[2]["points"]), bits(b[2]["points"]))
    assert torch.equal(a[3], b[3]) and np.array_equal(bits(a[4]), bits(b[4]))


# -- (f) both demo modes read the file the command line writes ---------------------------------------------------------------------------
def _train(tmp_path, name):
    from speechdrivestemplates_amd.config import get_cfg_defaults
    from speechdrivestemplates_amd.core.pipelines import get_pipeline
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(REPO, "configs", name + ".yaml"))
    cfg.merge_from_list(["DATASET.NAME", "SyntheticGestureDataset", "DATASET.SYNTHETIC_CLIPS", 8, "TRAIN.BATCH_SIZE", 4, "TEST.BATCH_SIZE", 4,
                         "TRAIN.NUM_EPOCHS", 1, "TRAIN.CHECKPOINT_INTERVAL", 1, "SYS.NUM_WORKERS", 0, "SYS.LOG_INTERVAL", 100,
                         "SYS.OUTPUT_DIR", str(tmp_path), "TRAIN.SAVE_VIDEO", False, "TEST.SAVE_VIDEO", False, "TEST.SAVE_NPZ", False,
                         "TRAIN.VALIDATE", False])
    cfg.freeze()
    torch.manual_seed(5)
    pipe = get_pipeline(cfg.PIPELINE_TYPE)(cfg)
    pipe.train(cfg, "t", None)
    pipe.close()
    return sorted(glob.glob(os.path.join(glob.glob(str(tmp_path / "*_t"))[0], "checkpoints", "checkpoint_epoch-1_*.pth")))[0]


def _demo_pipeline(tmp_path, name, opts):
    from scipy.io import wavfile

    from speechdrivestemplates_amd.config import get_cfg_defaults
    from speechdrivestemplates_amd.core.datasets.gesture_dataset import load_speaker_stats
    from speechdrivestemplates_amd.core.pipelines import get_pipeline
    load_speaker_stats(os.path.join(GOLDEN, "speaker_stat_oliver.npz"), "oliver")
    wav = str(tmp_path / "x.wav")
    wavfile.write(wav, 16000, (np.random.default_rng(2).standard_normal(int(16000 * 2.4)) * 2000).astype(np.int16))
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(REPO, "configs", name + ".yaml"))
    cfg.merge_from_list(["DATASET.SPEAKER", "oliver", "SYS.OUTPUT_DIR", str(tmp_path / "demo"), "TEST.SAVE_NPZ", False,
                         "TEST.SAVE_VIDEO", False] + opts)
    cfg.freeze()
    return get_pipeline(cfg.PIPELINE_TYPE)(cfg), cfg, wav


def test_pose2pose_demo_reads_the_file(tmp_path, capsys):
    ca = CA()
    ckpt = _train(tmp_path, "pose2pose")
    out = str(tmp_path / "axes.npz")
    assert ca.main(["--checkpoint", ckpt, "--out", out, "--axes", "3", "--steps", "5"]) == 0
    printed = capsys.readouterr().out
    z = np.load(out)
    assert z["v"].shape == (32, 32) and z["v"].dtype == np.float32 and z["code_index"].shape == (3, 5)
    assert "DEMO.CODE_PATH %s" % out in printed and "module.clip_code_mu (8, 32)" in printed
    assert "DEMO.CODE_INDEX %d DEMO.CODE_INDEX_B %d" % (z["code_index"][0, 0], z["code_index"][0, -1]) in printed
    demo, cfg, wav = _demo_pipeline(tmp_path, "pose2pose", ["DEMO.CODE_PATH", out, "DEMO.MULTIPLE", 3])
    outs = demo.demo(cfg, "demo", ckpt, wav)
    assert len(outs) == 3
    batch = next(iter(demo.test_dataloader))
    for i, o in enumerate(outs):
        p = o["poses_pred_batch"]
        assert p.shape == (1, cfg.DATASET.NUM_FRAMES, 2, 121) and p.dtype == torch.float64 and torch.isfinite(p).all()
        code = torch.tensor(z["v"][i] * 10, dtype=torch.float32, device="cuda").unsqueeze(0)
        assert torch.equal(o["clip_code_mu"], code)
        with torch.no_grad():  # the model's external-code path, directly
            pred, _, _ = demo.model.ae(None, cfg.DATASET.NUM_FRAMES, external_code=code)
        assert torch.equal(p, demo.test_dataset.get_final_results(pred.detach(), batch["speaker_stat"]))
    assert not torch.equal(outs[0]["poses_pred_batch"], outs[1]["poses_pred_batch"])
    demo.close()


def test_voice2pose_demo_reads_the_file(tmp_path):
    ca = CA()
    ckpt = _train(tmp_path, "voice2pose_sdt_bp")
    out = str(tmp_path / "axes.npz")
    assert ca.main(["--checkpoint", ckpt, "--out", out, "--table", "module.clips_code"]) == 0
    z = np.load(out)
    a, b = int(z["code_index"][0, 0]), int(z["code_index"][0, -1])
    assert z["code_index"].shape == (4, 7) and 0 <= a < 8 and 0 <= b < 8
    demo, cfg, wav = _demo_pipeline(tmp_path, "voice2pose_sdt_bp", ["DEMO.CODE_INDEX", a, "DEMO.CODE_INDEX_B", b, "DEMO.MULTIPLE", 2])
    outs = demo.demo(cfg, "demo", ckpt, wav)
    assert len(outs) == 2
    table = demo.model.clips_code.detach()
    assert torch.equal(outs[0]["condition_code"][0], table[a]) and torch.equal(outs[1]["condition_code"][0], table[b])
    # the file's own numbers: the rows it names are the nearest to its points
    index, dist2 = ca.model_nearest(table.cpu().numpy(), z["points"])
    assert np.array_equal(index.reshape(4, 7), z["code_index"]) and np.array_equal(bits(dist2.reshape(4, 7)), bits(z["code_dist2"]))
    demo.close()
