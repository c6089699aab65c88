"""The device FGD (csrc/fgd.hip, speechdrivestemplates_amd/fgd.py, SYS.DEVICE_FGD) on the GPU.

Bars.  Full-rank synthetic sets (tests/golden/synth_fgd_sets.py) against compute_fgd (scipy sqrtm, float64): 100 x the error of the numpy
restatement recorded in profiles/r09_fgd_host_error.txt, floor 1e-12 x (tr C_A + tr C_B + gap^2) -- the kernels differ from the restatement by
summation order and Jacobi-vs-LAPACK only (test_fgd_device_host.device_bar; factor and floor of tests/test_code_pca_gpu.py).  Rank-deficient
sets (the reference's fixture, 8 validation clips): 2e-6 |ref| + 1e-6, the bar tests/test_geometry.py holds compute_fgd to on that fixture
(sqrtm of a singular product is itself only good to about 1e-7).  Every measured figure is printed before its assertion
(profiles/r09_test_fgd_gpu.txt).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN, REPO
from test_fgd_device_host import FIXTURE_TAGS, contract_fgd_of_sets, device_bar, fixture, host_fgd, scale_of

sys.path.insert(0, GOLDEN)
import synth_fgd_sets as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def fixture_bar(ref):
    return 2e-6 * abs(ref) + 1e-6


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def held(name, got, want, bar, recorded=None):
    err = abs(got - want)
    print("  %-44s device %.12g want %.12g error %.3e%s bar %.3e" % (name, got, want, err, "" if recorded is None else " recorded %.3e" % recorded,
                                                                      bar))
    assert err <= bar, "%s: error %.3e > bar %.3e" % (name, err, bar)


def case_bar(case):
    from test_fgd_device_host import read_host_errors
    scale = scale_of(contract_fgd_of_sets(*S.case_pair(case)))
    return device_bar(case, scale), read_host_errors()[case]


def accumulator(a, b, cuts=None, dim=None):
    """an FGDAccumulator fed the float32 arrays a / b in calls of ``cuts`` rows (default: one call)"""
    from speechdrivestemplates_amd.fgd import FGDAccumulator
    acc = FGDAccumulator(a.shape[1] if dim is None else dim, DEV)
    ta, tb = dev(a), dev(b)
    lo = 0
    for n in cuts or (a.shape[0],):
        acc.add(ta[lo:lo + n], tb[lo:lo + n])
        lo += n
    assert lo == a.shape[0]
    return acc


# (a) ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.FULL_RANK)
def test_full_rank_sets_match_compute_fgd(case):
    from speechdrivestemplates_amd.fgd import compute_fgd_device, fgd_device_result
    a, b = S.case_pair(case)
    bar, rec = case_bar(case)
    held(case + " FGD vs compute_fgd", compute_fgd_device(a, b), host_fgd(case), bar, rec)
    res, want = fgd_device_result(a, b), contract_fgd_of_sets(a, b)
    assert res["err"] == 0 and res["rows_a"] == res["rows_b"] == a.shape[0] and res["first_bad_row_a"] == res["first_bad_row_b"] == -1
    for k in ("mean_gap_sq", "trace_a", "trace_b", "trace_sqrt"):
        held(case + " " + k + " vs restatement", res[k], want[k], bar)
    print("  %s sweeps %d / %d, off-diagonal norms %.3e / %.3e, smallest eigenvalues %.3e / %.3e"
          % (case, res["sweeps_a"], res["sweeps_m"], res["offdiag_a"], res["offdiag_m"], res["min_eig_a"], res["min_eig_m"]))
    assert res["offdiag_a"] <= 1e-15 * want["trace_a"] and res["min_eig_a"] > 0 and res["min_eig_m"] > 0  # (||C||_F <= tr C for a PSD matrix)


# (b) ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", FIXTURE_TAGS)
def test_reference_fixture(tag):
    from speechdrivestemplates_amd.fgd import compute_fgd_device
    g = fixture()
    ref = float(g[tag + "/fgd_ab"][0])
    held(tag + " FGD vs the reference's output", compute_fgd_device(g[tag + "/a"], g[tag + "/b"]), ref, fixture_bar(ref))
    held(tag + " FGD of identical sets", compute_fgd_device(g[tag + "/a"], g[tag + "/a"]), 0.0, 1e-5)


# (c) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_large_common_offset_loses_no_digits():
    from speechdrivestemplates_amd.fgd import compute_fgd_device
    a, b = S.case_pair("offset")
    bar, rec = case_bar("offset")
    held("offset FGD vs compute_fgd", compute_fgd_device(a, b), host_fgd("offset"), bar, rec)


# (d) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_chunking_and_merging():
    a, b = S.case_pair("chunks")
    bar, rec = case_bar("chunks")
    want = host_fgd("chunks")
    one = accumulator(a, b)
    cut = accumulator(a, b, cuts=(1, 31, 32, 136))
    r_one, r_cut = one.result(), cut.result()
    held("one add vs compute_fgd", r_one["fgd"], want, bar, rec)
    held("adds of 1, 31, 32, 136 rows vs compute_fgd", r_cut["fgd"], want, bar, rec)
    assert torch.equal(one.states(), cut.states())  # rows walked in order per entry: how they were cut into calls leaves no trace
    parts = [accumulator(a[lo:hi], b[lo:hi]) for lo, hi in ((0, 70), (70, 71), (71, 200))]  # three "ranks", three shifts
    r_parts = parts[0].result(gathered=parts)
    r_stack = parts[0].result(gathered=torch.stack([p.states() for p in parts]))
    held("three states finalized together vs compute_fgd", r_parts["fgd"], want, bar, rec)
    held("three states vs one add", r_parts["fgd"], r_one["fgd"], bar)
    assert r_parts == r_stack and r_parts["rows_a"] == r_parts["rows_b"] == 200
    # the same call sequence twice: the same bits, states and out
    again = accumulator(a, b, cuts=(1, 31, 32, 136))
    assert torch.equal(again.states(), cut.states()) and again.result() == r_cut
    parts2 = [accumulator(a[lo:hi], b[lo:hi]) for lo, hi in ((0, 70), (70, 71), (71, 200))]
    assert parts2[0].result(gathered=parts2) == r_parts
    # reset: back to the zeroed state
    cut.reset()
    assert not cut.states().any()
    cut.add(dev(a), dev(b))
    assert torch.equal(cut.states(), one.states())


# (e) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_leading_sub_block():
    a, b = S.case_pair("chunks")
    bar, rec = case_bar("chunks_mu")
    sub = accumulator(a, b).result(dim_used=32)
    mu_only = accumulator(a[:, :32], b[:, :32]).result()
    held("dim_used=32 of 64 vs a 32-wide accumulator", sub["fgd"], mu_only["fgd"], bar)
    held("dim_used=32 of 64 vs compute_fgd", sub["fgd"], host_fgd("chunks_mu"), bar, rec)
    assert sub["dim_used"] == 32 and mu_only["dim_used"] == 32


# (f) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_two_tensor_rows_equal_the_concatenation():
    from speechdrivestemplates_amd.fgd import FGDAccumulator
    a, b = S.case_pair("chunks")
    ta, tb = dev(a), dev(b)
    for d0 in (32, 1, 63):
        split, cat = FGDAccumulator(64, DEV), FGDAccumulator(64, DEV)
        split.add(ta[:, :d0].contiguous(), tb[:, :d0].contiguous(), ta[:, d0:].contiguous(), tb[:, d0:].contiguous())
        cat.add(torch.cat([ta[:, :d0], ta[:, d0:]], 1), torch.cat([tb[:, :d0], tb[:, d0:]], 1))
        assert torch.equal(split.states(), cat.states()), d0
        assert split.result() == cat.result()


# (g) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_loud_failures():
    from speechdrivestemplates_amd import fgd as F
    a, b = S.case_pair("chunks")
    bad = b.copy()
    bad[137, 5] = np.nan
    bad[150, 0] = np.inf
    acc = accumulator(a, bad, cuts=(100, 100))  # the bad row is row 37 of the second call: its global index is recorded
    with pytest.raises(FloatingPointError, match=r"side gt first at row 137"):
        acc.result()
    res = acc.result(strict=False)
    assert np.isnan(res["fgd"]) and res["err"] & F.ERR_NON_FINITE and res["first_bad_row_b"] == 137 and res["first_bad_row_a"] == -1
    assert "side gt first at row 137" in F.describe_error(res) and "pred" not in F.describe_error(res)
    first = a.copy()
    first[0, 3] = np.nan  # in the very row that fixes the shift
    res = accumulator(first, b).result(strict=False)
    assert np.isnan(res["fgd"]) and res["first_bad_row_a"] == 0 and res["first_bad_row_b"] == -1
    with pytest.raises(FloatingPointError, match=r"side pred first at row 0"):
        accumulator(first, b).result()
    one_row = accumulator(a[:1], b[:1])
    with pytest.raises(ValueError, match="at least 2 rows"):
        one_row.result()
    res = one_row.result(strict=False)
    assert np.isnan(res["fgd"]) and res["err"] == F.ERR_TOO_FEW_ROWS and res["rows_a"] == 1
    with pytest.raises(ValueError, match="at least 2 rows"):
        F.FGDAccumulator(64, DEV).result()  # nothing added at all
    dense = accumulator(a, b)
    res = dense.result(strict=False, max_sweeps=1)
    assert res["err"] == F.ERR_NOT_CONVERGED and res["sweeps_a"] == 1
    with pytest.raises(RuntimeError, match="did not converge"):
        dense.result(max_sweeps=1)
    assert dense.result()["err"] == 0  # the states are read, never written, by finalize
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dense.add(torch.zeros(4, 64), torch.zeros(4, 64))
    with pytest.raises(TypeError):
        dense.add(dev(a).double(), dev(b).double())
    with pytest.raises(ValueError):
        dense.add(dev(a[:, :32]), dev(b[:, :32]))
    with pytest.raises(ValueError):
        dense.result(dim_used=65)


# (h) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_add_is_capturable_in_a_graph():
    from speechdrivestemplates_amd.fgd import FGDAccumulator
    a, b = S.case_pair("full_d64")
    mu_p, lv_p, mu_g, lv_g = (dev(x) for x in (a[:32, :32], a[:32, 32:], b[:32, :32], b[:32, 32:]))
    eager, graphed = FGDAccumulator(64, DEV), FGDAccumulator(64, DEV)
    for _ in range(3):
        eager.add(mu_p, mu_g, lv_p, lv_g)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):  # a single branch on a stream of the test's own
        graphed.add(mu_p, mu_g, lv_p, lv_g)
    torch.cuda.synchronize()
    graphed.reset()  # (a capture runs nothing; the host-side row count restarts with the state)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.states(), eager.states())
    assert graphed.result() == eager.result() and eager.result()["rows_a"] == 96


# (i) ----------------------------------------------------------------------------------------------------------------------------------------------
def _validation_pipeline(extra_opts=(), n_val=8, batch=4, indices=None):
    from speechdrivestemplates_amd.core.datasets import gesture_dataset as gd
    from test_model_gpu import _make_pipeline
    pipe, cfg = _make_pipeline("voice2pose_sdt_bp", 16, 0.5, list(extra_opts))
    ds = gd.SyntheticGestureDataset(cfg=cfg, num_clips=n_val, split='val')
    pipe.test_dataset = ds if indices is None else torch.utils.data.Subset(ds, indices)
    pipe.test_dataloader = torch.utils.data.DataLoader(pipe.test_dataset, batch_size=batch, shuffle=False)
    pipe.num_test_samples, pipe.num_test_batches = len(pipe.test_dataset), len(pipe.test_dataloader)
    return pipe, cfg


def _set_key(cfg, on):
    cfg.defrost()
    cfg.SYS.DEVICE_FGD = bool(on)
    cfg.freeze()


def test_validate_with_the_key_on_matches_the_host_loop(monkeypatch):
    from oracle import sdt_oracle as O
    pipe, cfg = _validation_pipeline()
    losses, _ = pipe.forward_backward(O.make_batch(4, 16, step=0, seed=1))  # (BN running statistics of the pose encoder leave their init values)
    pipe.optimizer_updates(losses)
    calls, step_results, host_copies = [], [], []
    orig_eval, orig_step, orig_cpu = pipe.evaluate_epoch, pipe.test_step, torch.Tensor.cpu
    monkeypatch.setattr(pipe, "evaluate_epoch", lambda d: (calls.append(sorted(d)), orig_eval(d))[1])
    monkeypatch.setattr(pipe, "test_step", lambda *a, **k: (lambda r: (step_results.append(r[1]), r)[1])(orig_step(*a, **k)))
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (host_copies.append(tuple(t.shape)), orig_cpu(t, *a, **k))[1])
    assert cfg.SYS.DEVICE_FGD is False
    torch.manual_seed(5)
    off = pipe.validate(pipe.test_dataloader, 1)
    assert len(calls) == 1 and {"mu_pred", "mu_gt", "logvar_pred", "logvar_gt"} <= set(calls[0])
    assert all("mu_pred" in r for r in step_results) and (4, 32) in host_copies
    del calls[:], step_results[:], host_copies[:]
    _set_key(cfg, True)
    try:
        torch.manual_seed(5)
        on = pipe.validate(pipe.test_dataloader, 1)
        assert calls == [] and step_results == [{}, {}]
        assert not any(len(s) == 2 and s[1] == 32 for s in host_copies), host_copies  # no (batch, 32) feature or code tensor went to the host
        assert set(on) == set(off)
        for k in off:
            if k.startswith("FGD"):
                held("validate() %s, key on vs key off" % k, float(on[k]), float(off[k]), fixture_bar(float(off[k])))
            else:
                assert torch.equal(torch.as_tensor(on[k]), torch.as_tensor(off[k])), k
        # a second epoch starts from a reset state: the same value, not the moments of 16 rows
        torch.manual_seed(5)
        again = pipe.validate(pipe.test_dataloader, 1)
        assert float(again["FGD_mu"]) == float(on["FGD_mu"]) and pipe.device_fgd().result(strict=False)["rows_a"] == 8
    finally:
        _set_key(cfg, False)


# (k) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_command_line_prints_the_same_distance(tmp_path):
    from speechdrivestemplates_amd.fgd import compute_fgd_device
    a, b = S.case_pair("full_d32")
    pa, pb = str(tmp_path / "a.npy"), str(tmp_path / "b.npy")
    np.save(pa, a)
    np.save(pb, b)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "speechdrivestemplates_amd.fgd", pa, pb], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    fields = dict(ln.split(": ", 1) for ln in r.stdout.strip().splitlines() if ": " in ln)
    assert float(fields["fgd"]) == compute_fgd_device(a, b) and int(fields["rows_a"]) == 128 and int(fields["err"]) == 0
    np.savez(str(tmp_path / "r.npz"), mu_pred=a, mu_gt=b, logvar_pred=a)
    pz = str(tmp_path / "r.npz")
    r = subprocess.run([sys.executable, "-m", "speechdrivestemplates_amd.fgd", pz, pz, "--keys", "mu_pred", "mu_gt"], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert float(dict(ln.split(": ", 1) for ln in r.stdout.strip().splitlines() if ": " in ln)["fgd"]) == compute_fgd_device(a, b)


# (j) two ranks on one GPU (last: it spawns) ---------------------------------------------------------------------------------------------------------
GT_CODE = ("VOICE2POSE.GENERATOR.CLIP_CODE.TEST_WITH_GT_CODE", True)  # the code comes from the ground-truth poses: no random draw in a step


def _rank_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from test_dp_gpu import _share_the_gpu
    _share_the_gpu(world)
    pipe, cfg = _validation_pipeline(GT_CODE + ("SYS.DEVICE_FGD", True, "SYS.DISTRIBUTED", True), batch=2)
    sampler = torch.utils.data.distributed.DistributedSampler(pipe.test_dataset, num_replicas=world, rank=rank, shuffle=False)
    loader = torch.utils.data.DataLoader(pipe.test_dataset, batch_size=2, shuffle=False, sampler=sampler)
    out = pipe.validate(loader, 1)
    q.put((rank, float(out["FGD_mu"]), float(out["FGD_mu_logvar"]), list(sampler), pipe.device_fgd().result(strict=False)["rows_a"]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_ranks_report_the_whole_sets_distance():
    from test_dp_gloo import _collect, _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(_collect(procs, q, len(procs), 800), key=lambda t: t[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    (_, mu0, mulv0, idx0, rows0), (_, mu1, mulv1, idx1, rows1) = res
    assert sorted(idx0 + idx1) == list(range(8)) and rows0 == rows1 == 4  # each rank delivered its own 4 clips
    assert mu0 == mu1 and mulv0 == mulv1  # the same states merged in the same order on both ranks
    # one process over the same 8 clips, key on
    pipe, _ = _validation_pipeline(GT_CODE + ("SYS.DEVICE_FGD", True), batch=2)
    whole = pipe.validate(pipe.test_dataloader, 1)
    held("two ranks FGD_mu vs one process, 8 clips", mu0, float(whole["FGD_mu"]), fixture_bar(float(whole["FGD_mu"])))
    held("two ranks FGD_mu_logvar vs one process, 8 clips", mulv0, float(whole["FGD_mu_logvar"]), fixture_bar(float(whole["FGD_mu_logvar"])))
    # what the key-off path reports under two ranks: the distance of rank 0's shard alone
    pipe, _ = _validation_pipeline(GT_CODE, batch=2, indices=idx0)
    shard = pipe.validate(pipe.test_dataloader, 1)
    print("  FGD_mu of rank 0's 4 clips alone (key off) %.9g, of the 8 clips %.9g" % (float(shard["FGD_mu"]), mu0))
    assert abs(float(shard["FGD_mu"]) - mu0) > 100 * fixture_bar(mu0)
