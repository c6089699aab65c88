"""The per-clip validation metrics on the GPU (csrc/clip_metrics.hip, speechdrivestemplates_amd/clip_metrics.py, TEST.CLIP_METRICS; DESIGN.md
section 22) against the numpy contract model.

Bars.  Integers (hit counts, seen, copies, nonfinite, frames) are equal.  The float sums run the model's operations in the model's order, so
where this device's float64 square root is correctly rounded (``sqrt_is_exact`` asks the library on 200 000 values and on the test's own
inputs) they are bit-identical; otherwise they are held to (n + 2) 2^-52 relative, n the number of non-negative terms (the bar of
tests/test_clip_metrics_host.py).  The epoch stage has no square root: its vector equals ``epoch_model`` of the device's own table bit for bit.
Every comparison prints how many values were bit-identical before it asserts.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO
from speechdrivestemplates_amd import clip_metrics as cm
from test_clip_metrics_host import (SHAPES, ULP, alphas_for, copies_for, nan_case, part_table, poses, single_keypoint_case, tie_case)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(R, T, K, m) for R, T, K in SHAPES for m in copies_for(R)] + [(16, 3, 65, 16), (32, 2, 121, 16)]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def sqrt_is_exact():
    rng = np.random.Generator(np.random.PCG64(11))
    x = np.concatenate([rng.uniform(0, 4, 100000), np.exp(rng.uniform(-30, 30, 100000)), [0.0, 1.0, 2.0, 4.0, 2.0 ** -1040]])
    same = np.array_equal(cm.device_sqrt(dev(x)).cpu().numpy(), np.sqrt(x))
    print("  device sqrt(float64) equals numpy's on %d values: %s" % (x.size, same))
    return same


def terms_of(pred, gt):
    """every argument of a square root the kernels take on these inputs"""
    px, py, gx, gy = pred[:, :, 0], pred[:, :, 1], gt[:, :, 0], gt[:, :, 1]
    out = [(px - gx) ** 2 + (py - gy) ** 2]
    if pred.shape[1] > 1:
        vpx, vpy, vgx, vgy = px[:, 1:] - px[:, :-1], py[:, 1:] - py[:, :-1], gx[:, 1:] - gx[:, :-1], gy[:, 1:] - gy[:, :-1]
        out += [vpx * vpx + vpy * vpy, vgx * vgx + vgy * vgy, (vpx - vgx) ** 2 + (vpy - vgy) ** 2]
    return np.concatenate([o.ravel() for o in out])


def exact_on(pred, gt):
    x = terms_of(pred, gt)
    x = x[np.isfinite(x)]
    return sqrt_is_exact() and np.array_equal(cm.device_sqrt(dev(x)).cpu().numpy(), np.sqrt(x))


def held(name, got, want, exact, T, parts):
    """records ``got`` (device) against ``want`` (model): integers equal; floats bit-identical, or within (n + 2) 2^-52 where sqrt is not exact"""
    assert np.array_equal(got[:, cm.HIT0:], want[:, cm.HIT0:]), "%s: integer columns differ" % name
    gf, wf = got[:, :20].view(np.float64), want[:, :20].view(np.float64)
    same = int((got[:, :20] == want[:, :20]).sum())
    print("  %-40s %d of %d float sums bit-identical (sqrt exact on these inputs: %s)" % (name, same, gf.size, exact))
    if exact:
        assert same == gf.size, "%s: %d of %d float sums differ in bits" % (name, gf.size - same, gf.size)
        return
    m = want[:, cm.COPIES].reshape(-1, 1, 1)
    frames = np.array([T, T - 1, T - 1, T - 1, 0]).reshape(1, 5, 1) * m + np.array([0, 0, 0, 0, T]).reshape(1, 5, 1) * (m * (m - 1) // 2)
    n = (frames * np.array(cm.part_sizes(parts)).reshape(1, 1, 4)).reshape(gf.shape)  # the number of terms behind every sum
    ok = (np.abs(gf - wf) <= (n + 2) * ULP * np.abs(wf)) | ((gf != gf) & (wf != wf))
    assert ok.all(), "%s: error %s" % (name, np.abs(gf - wf).max())


def committed(pred, gt, parts, alphas, m, index=None, num_clips=None):
    B = pred.shape[0] // m
    acc = cm.ClipMetricsAccumulator(B if num_clips is None else num_clips, pred.shape[3], alphas, DEV, parts=parts)
    acc.add(dev(pred), dev(gt), torch.arange(B, dtype=torch.int64) if index is None else index, m)
    return acc


@functools.lru_cache(maxsize=None)
def model_records(R, T, K, m, n_alphas):
    pred, gt = poses(R, T, K)
    return cm.clip_metrics_model(pred, gt, part_table(K), alphas_for(n_alphas), m)


# (a) ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-m%d" % c)
def test_kernels_match_the_model(case):
    R, T, K, m = case
    n_alphas = 1 + (CASES.index(case) + K) % 4
    pred, gt = poses(R, T, K)
    want = model_records(R, T, K, m, n_alphas)
    acc = committed(pred, gt, part_table(K), alphas_for(n_alphas), m)
    got = acc.table().cpu().numpy()
    held("R=%d T=%d K=%d m=%d A=%d" % (R, T, K, m, n_alphas), got, want, exact_on(pred, gt), T, part_table(K))
    assert acc.state()[-1].cpu().tolist() == [0] * cm.COLS  # the header: no index error, nothing else written
    if m == 1:  # the row records alone are the clip records of one copy
        assert np.array_equal(acc.row_records(dev(pred), dev(gt)).cpu().numpy(), got)


# (b) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_ties_single_keypoint_and_nan_on_the_device():
    pred, gt, parts, alphas = tie_case()
    u = cm.unpack(committed(pred, gt, parts, alphas, 1).table().cpu().numpy())
    assert u['pck_hit'][0, 0].tolist() == [2, 1, 0, 1]
    pred, gt, parts, alphas = single_keypoint_case()
    got = committed(pred, gt, parts, alphas, 1).table().cpu().numpy()
    u = cm.unpack(got)
    assert u['pck_hit'][0, :2, :2].tolist() == [[1, 1], [1, 1]] and not u['pck_hit'][1].any()
    assert np.array_equal(got, cm.clip_metrics_model(pred, gt, parts, alphas))
    pred, gt, parts, alphas = nan_case()
    acc = committed(pred, gt, parts, alphas, 1)
    got = acc.table().cpu().numpy()
    clean = committed(np.nan_to_num(pred), gt, parts, alphas, 1).table().cpu().numpy()
    assert got[:, cm.NONFINITE].tolist() == [0, 1, 0]
    assert np.array_equal(got[[0, 2]], clean[[0, 2]])  # no bit of another clip's record changes
    want = cm.clip_metrics_model(pred, gt, parts, alphas)
    assert np.array_equal(got[:, cm.HIT0:], want[:, cm.HIT0:])
    assert np.array_equal(np.isnan(got[:, :20].view(np.float64)), np.isnan(want[:, :20].view(np.float64)))
    res = acc.result()
    assert res['clips_nonfinite'] == 1 and res['clips_seen'] == 3 and all(np.isfinite(v) for v in res.values())
    assert np.array_equal(acc.result_words(), cm.epoch_model([got], cm.part_sizes(parts), 2))
    # copies: a NaN in one copy of clip 1 flags clip 1 alone, its diversity included
    pred, gt = poses(6, 3, 5, seed=4)
    pred[3, 1, 1, 2] = np.nan  # row 3 = copy 1 of clip 1 (B = 2)
    got = committed(pred, gt, parts, alphas, 3).table().cpu().numpy()
    clean = committed(np.nan_to_num(pred), gt, parts, alphas, 3).table().cpu().numpy()
    assert got[:, cm.NONFINITE].tolist() == [0, 1] and np.array_equal(got[0], clean[0])


# (c) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_commit_writes_the_addressed_rows_and_counts_bad_indices():
    N, T, K, SENTINEL = 10, 3, 5, 0x5A5AA5A55A5AA5A5
    parts, alphas = part_table(K), [0.1, 0.2]
    pred, gt = poses(5, T, K, seed=5)
    acc = cm.ClipMetricsAccumulator(N, K, alphas, DEV, parts=parts)
    acc.state().fill_(SENTINEL)
    acc.state()[N].zero_()
    index = torch.tensor([7, 2, -1, N, 4], dtype=torch.int64)
    acc.add(dev(pred), dev(gt), index, 1)
    want = cm.clip_metrics_model(pred, gt, parts, alphas)
    state = acc.state().cpu().numpy()
    for row, b in ((7, 0), (2, 1), (4, 4)):
        assert np.array_equal(state[row], want[b]), row
    untouched = [r for r in range(N) if r not in (7, 2, 4)]
    assert (state[untouched] == SENTINEL).all()
    assert state[N, 0] == 2 and not state[N, 1:].any()  # the two bad indices are counted, and wrote nothing
    # a clip written twice: the second record replaces the first
    pred2, gt2 = poses(2, T, K, seed=6)
    acc.add(dev(pred2), dev(gt2), torch.tensor([2], dtype=torch.int64), 2)
    again = acc.state().cpu().numpy()
    assert np.array_equal(again[2], cm.clip_metrics_model(pred2, gt2, parts, alphas, 2)[0]) and again[2, cm.COPIES] == 2
    keep = [r for r in range(N + 1) if r != 2]
    assert np.array_equal(again[keep], state[keep])
    # a multiplied batch hands its index in multiplied: the first B entries are read
    acc.add(dev(pred2), dev(gt2), torch.tensor([3, 3], dtype=torch.int64), 2)
    assert np.array_equal(acc.table()[3].cpu().numpy(), again[2])
    acc.reset()
    assert not acc.state().any()


# (d) ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 200])
def test_epoch_is_the_same_however_the_records_arrive(N):
    T, K, m = 3, 5, 2
    parts, alphas = part_table(K), [0.1, 0.2]
    sizes = cm.part_sizes(parts)
    rng = np.random.Generator(np.random.PCG64(N))
    seen = np.array([0]) if N == 1 else np.sort(rng.permutation(N)[:max(1, 3 * N // 4)])  # holes: a quarter of the clips arrive nowhere
    n = len(seen)
    pred, gt = poses(m * n, T, K, seed=N)
    p5, g5 = pred.reshape(m, n, T, 2, K), gt.reshape(m, n, T, 2, K)

    def rows(a, sel):
        return dev(a[:, sel].reshape(m * len(sel), T, 2, K))

    def feed(acc, sel, spoil=False):
        acc.add(rows(p5 + 1.0 if spoil else p5, sel), rows(g5, sel), torch.from_numpy(seen[sel]), m)

    one = cm.ClipMetricsAccumulator(N, K, alphas, DEV, parts=parts)
    feed(one, rng.permutation(n))  # one add of all rows, shuffled
    words = one.result_words()
    table = one.table().cpu().numpy()
    assert np.array_equal(words, cm.epoch_model([table], sizes, 2))
    assert words[cm.OUT_SEEN] == n and words[cm.OUT_NONFINITE] == 0 and words[cm.OUT_PAIR_FRAMES] == n * T
    vals = one.result()
    assert {'diversity', 'diversity_hands'} <= set(vals) and all(np.isfinite(v) for v in vals.values()) and vals['clips_seen'] == n
    ragged = cm.ClipMetricsAccumulator(N, K, alphas, DEV, parts=parts)
    for sel in np.array_split(np.arange(n), min(7, n)):  # up to 7 adds of ragged sizes
        feed(ragged, sel)
    assert torch.equal(ragged.state(), one.state()) and np.array_equal(ragged.result_words(), words)
    # three per-rank tables with overlapping clips: the higher rank of an overlap holds another record, which must not be read
    ranks = [cm.ClipMetricsAccumulator(N, K, alphas, DEV, parts=parts) for _ in range(3)]
    for r in range(3):
        own = np.arange(n)[np.arange(n) % 3 == r]
        if len(own):
            feed(ranks[r], own)
        if r > 0:
            other = np.arange(n)[(np.arange(n) % 3 == r - 1) & (np.arange(n) % 2 == 0)]
            if len(other):
                feed(ranks[r], other, spoil=True)
    gathered = torch.stack([a.state() for a in ranks])
    assert np.array_equal(ranks[2].result_words(gathered), words) and np.array_equal(ranks[0].result_words(ranks), words)
    if n >= 6:
        assert not np.array_equal(ranks[0].result_words(ranks[::-1]), words)  # (rank order matters where records differ)
    # reset, then the same feed: the same bits
    one.reset()
    assert one.result()['clips_seen'] == 0
    feed(one, np.arange(n))
    assert np.array_equal(one.result_words(), words)


# (e) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_size_checks():
    with pytest.raises(ValueError, match="K = 129"):
        cm.ClipMetricsAccumulator(4, 129, [0.1], DEV, parts=[0] * 129)
    with pytest.raises(ValueError, match="alphas"):
        cm.ClipMetricsAccumulator(4, 5, [0.1] * 5, DEV, parts=part_table(5))
    acc = cm.ClipMetricsAccumulator(4, 5, [0.1], DEV, parts=part_table(5))
    x = torch.zeros((17, 2, 2, 5), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="17 copies"):
        acc.add(x, x, torch.zeros(1, dtype=torch.int64), 17)
    with pytest.raises(ValueError):
        acc.add(x, x, torch.zeros(1, dtype=torch.int64), 2)  # 17 rows are not 2 copies
    with pytest.raises(TypeError):
        acc.add(x.float(), x.float(), torch.zeros(17, dtype=torch.int64), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        acc.add(x.cpu(), x.cpu(), torch.zeros(17, dtype=torch.int64), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cm.ClipMetricsAccumulator(4, 5, [0.1], "cpu", parts=part_table(5))
    # the library checks the same sizes before any launch
    import ctypes as C
    from speechdrivestemplates_amd import _lib
    lib, p = _lib.load(), lambda t: C.c_void_p(t.data_ptr())
    w = torch.zeros(1 << 16, dtype=torch.int64, device=DEV)
    al = (C.c_double * 5)(*[0.1] * 5)
    assert lib.sdt_clip_metrics_rows_f64(p(w), p(w), p(w), al, 1, 1, 1, 129, p(w), p(w), None) == -1
    assert lib.sdt_clip_metrics_rows_f64(p(w), p(w), p(w), al, 5, 1, 1, 5, p(w), p(w), None) == -1
    assert lib.sdt_clip_metrics_rows_f64(p(w), p(w), p(w), al, 1, 1, 0, 5, p(w), p(w), None) == -1
    assert lib.sdt_clip_metrics_diversity_f64(p(w), p(w), 1, 17, 1, 5, p(w), None) == -1
    assert lib.sdt_clip_metrics_diversity_f64(p(w), p(w), 1, 1, 1, 5, p(w), None) == -1
    assert lib.sdt_clip_metrics_commit(p(w), p(w), p(w), 1, 17, 1, p(w), 4, None) == -1
    torch.cuda.synchronize()
    assert not w.any()


# (f) the pipeline -----------------------------------------------------------------------------------------------------------------------------------
NEW_KEYS = ["PCK_0.1", "PCK_0.2", "PCK", "PCK_hands", "L2_body", "L2_face", "L2_hands", "speed_ratio", "speed_ratio_hands", "vel_L2",
            "diversity", "diversity_hands", "clips_nonfinite"]


def _set_key(cfg, on, multiple=1):
    cfg.defrost()
    cfg.TEST.CLIP_METRICS, cfg.TEST.MULTIPLE = bool(on), multiple
    cfg.freeze()


def test_validate_with_the_key_off_and_on(monkeypatch, tmp_path):
    """Bar of the epoch values against the model of the captured poses where sqrt is not exact: a mean of n non-negative terms to
    (n + 2) 2^-52, a quotient of two such sums to twice that; n <= 2 copies x 64 frames x 121 keypoints x 8 clips (the diversity has fewer)."""
    from oracle import sdt_oracle as O
    from test_fgd_gpu import _validation_pipeline
    pipe, cfg = _validation_pipeline()
    losses, _ = pipe.forward_backward(O.make_batch(4, 16, step=0, seed=1))
    pipe.optimizer_updates(losses)
    _set_key(cfg, False, 2)
    torch.manual_seed(5)
    off = pipe.validate(pipe.test_dataloader, 1)
    assert {"L2_dist", "lip_sync_error_n", "FGD_mu", "FGD_mu_logvar"} <= set(off)
    assert pipe.clip_metrics() is None and not set(off) & set(NEW_KEYS)  # no accumulator exists, no new key
    calls = []
    orig_add = cm.ClipMetricsAccumulator.add
    monkeypatch.setattr(cm.ClipMetricsAccumulator, "add",
                        lambda self, p, g, idx, m=1: (calls.append((p.cpu().numpy(), g.cpu().numpy(), idx.cpu().numpy(), m)),
                                                      orig_add(self, p, g, idx, m))[1])
    _set_key(cfg, True, 2)
    pipe.base_path = str(tmp_path)
    try:
        torch.manual_seed(5)
        on = pipe.validate(pipe.test_dataloader, 1)
        new = NEW_KEYS
        assert list(on) == list(off) + new
        for k in off:
            assert torch.equal(torch.as_tensor(on[k]), torch.as_tensor(off[k])), k  # the parent's values keep their bits
        assert all(np.isfinite(float(on[k])) for k in new) and on["clips_nonfinite"] == 0
        assert on["PCK"] == (on["PCK_0.1"] + on["PCK_0.2"]) / 2
        assert 0 <= on["PCK_0.1"] <= on["PCK_0.2"] <= 1 and on["diversity"] >= 0 and on["speed_ratio"] > 0
        # the model on the poses test_step handed over
        assert len(calls) == 2 and all(c[0].shape == (8, 64, 2, 121) and c[3] == 2 for c in calls)
        parts = part_table(121)
        table = np.zeros((8, cm.COLS), dtype=np.int64)
        for p, g, idx, m in calls:
            assert idx.shape == (8,) and np.array_equal(idx[:4], idx[4:])
            table[idx[:4]] = cm.clip_metrics_model(p, g, parts, [0.1, 0.2], m)
        want = cm.epoch_values(cm.epoch_model([table], cm.part_sizes(parts), 2), (0.1, 0.2))
        acc = pipe.clip_metrics()
        got_table = acc.table().cpu().numpy()
        exact = all(exact_on(p, g) for p, g, _, _ in calls)
        held("validate(): the table against the model", got_table, table, exact, 64, parts)
        n = 2 * 64 * 121 * 8
        for k in new:
            err, bar = abs(float(on[k]) - want[k]), 0.0 if exact else 2 * (n + 2) * ULP * abs(want[k])
            print("  %-20s device %.17g model %.17g error %.3e bar %.3e" % (k, float(on[k]), want[k], err, bar))
            assert err <= bar, k
        with np.load(str(tmp_path / "results" / "epoch1-VAL-clip_metrics.npz")) as z:
            assert np.array_equal(z["table"], got_table) and tuple(z["columns"]) == cm.COLUMN_NAMES and z["alphas"].tolist() == [0.1, 0.2]
        # a second epoch starts from a reset table: the same values
        torch.manual_seed(5)
        again = pipe.validate(pipe.test_dataloader, 1)
        assert all(float(again[k]) == float(on[k]) for k in on) and pipe.clip_metrics() is acc
    finally:
        pipe.base_path = None
        _set_key(cfg, False, 1)


# (g) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_command_line_prints_the_values_of_the_device_route(tmp_path):
    files, sets = [], []
    for i in range(2):
        pred, gt = poses(2 + 2 * i, 4, 121, seed=20 + i)
        files.append(str(tmp_path / ("epoch0-TEST-step%d.npz" % i)))
        np.savez(files[-1], poses_pred_batch=pred, poses_gt_batch=gt, mu_pred=np.zeros((2, 4)))
        sets.append((pred, gt))
    acc = cm.ClipMetricsAccumulator(3, 121, [0.1, 0.3], DEV)
    acc.add(dev(sets[0][0]), dev(sets[0][1]), torch.tensor([0]), 2)
    acc.add(dev(sets[1][0]), dev(sets[1][1]), torch.tensor([1, 2]), 2)
    want = acc.result()
    out = str(tmp_path / "table.npz")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "speechdrivestemplates_amd.clip_metrics"] + files +
                       ["--alphas", "0.1", "0.3", "--multiple", "2", "--worst", "2", "--out", out], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    fields = dict(ln.split(": ", 1) for ln in lines if ": " in ln and not ln.startswith("worst"))
    assert list(fields) == list(want)
    for k, v in want.items():
        assert float(fields[k]) == v, k
    worst = [ln for ln in lines if ln.startswith("worst")]
    err = cm.hand_errors(acc.table().cpu().numpy(), cm.part_sizes(acc.parts))
    assert len(worst) == 2 and worst[0].startswith("worst: clip %d " % int(np.argmax(err))) and repr(float(err.max())) in worst[0]
    with np.load(out) as z:
        assert np.array_equal(z["table"], acc.table().cpu().numpy())


# (h) two ranks on one GPU (last: it spawns) ---------------------------------------------------------------------------------------------------------
GT_CODE = ("VOICE2POSE.GENERATOR.CLIP_CODE.TEST_WITH_GT_CODE", True)  # the code comes from the ground-truth poses: no random draw in a step


def _rank_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from test_dp_gpu import _share_the_gpu
    from test_fgd_gpu import _validation_pipeline
    _share_the_gpu(world)
    pipe, cfg = _validation_pipeline(GT_CODE + ("TEST.CLIP_METRICS", True, "SYS.DISTRIBUTED", True), batch=2)
    sampler = torch.utils.data.distributed.DistributedSampler(pipe.test_dataset, num_replicas=world, rank=rank, shuffle=False)
    loader = torch.utils.data.DataLoader(pipe.test_dataset, batch_size=2, shuffle=False, sampler=sampler)
    out = pipe.validate(loader, 1)
    q.put((rank, {k: float(v) for k, v in out.items()}, list(sampler), pipe.clip_metrics().table()[:, cm.SEEN].cpu().tolist()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_ranks_report_the_whole_sets_values():
    from test_dp_gloo import _collect, _free_port
    from test_fgd_gpu import _validation_pipeline
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
    (_, out0, idx0, seen0), (_, out1, idx1, seen1) = res
    assert sorted(idx0 + idx1) == list(range(8)) and sum(seen0) == sum(seen1) == 4  # each rank delivered its own 4 clips
    assert [a + b for a, b in zip(seen0, seen1)] == [1] * 8
    names = [k for k in NEW_KEYS if not k.startswith("diversity")]
    assert set(names) <= set(out0) and "diversity" not in out0  # (one copy: no diversity)
    assert all(out0[k] == out1[k] for k in names)  # the same tables, read in the same order, on both ranks
    # one process over the same 8 clips: the same set, batched differently.  The epoch stage is bit-identical for identical records (test (d));
    # the records themselves come from an fp32 network whose batches differ here, so the bar is the one the smoke test holds the fp32
    # prediction to (5e-5 relative) with 20 x headroom for hits that flip at a threshold: 1e-3 max(1, |value|)
    pipe, _ = _validation_pipeline(GT_CODE + ("TEST.CLIP_METRICS", True), batch=2)
    whole = pipe.validate(pipe.test_dataloader, 1)
    for k in names:
        print("  %-20s two ranks %.17g one process %.17g" % (k, out0[k], float(whole[k])))
        assert abs(out0[k] - float(whole[k])) <= 1e-3 * max(1.0, abs(float(whole[k]))), k
    assert pipe.clip_metrics().result()["clips_seen"] == 8
