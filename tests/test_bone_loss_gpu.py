"""ops.BoneLossFn (csrc/bone_loss.hip) against the float64 model of tests/test_bone_loss_host.py -- both losses and
the autograd gradient -- over the edge shapes, each term alone and both together, masks, part weights, degenerate limbs, garbage under
the mask and repeated calls; then Voice2PoseModel with the keys at their defaults (the old path, untouched) and switched on (eager and
replayed from a hipGraph).

Bars, from one fp32 rounding of a float64 value: a loss is within 2^-22 relative of the model's; a gradient element within
2^-22 |model| + 2^-40 sum|terms|, ``terms`` being the absolute edge contributions that were added up to that element (the model returns
their sum): the kernel adds them in another order than the model, and a root's element is a sum of its whole part's contributions that
nearly cancel, so the error of that sum scales with the terms, not with the result.  Where nothing was added (sum|terms| = 0: a dead or
unconnected keypoint, pred == gt) the model's 0 is structural and the kernel's must be exactly 0 as well; a sum of non-zero terms that
happens to come out as 0.0 in the model's order is held to the bound above like any other element."""
import numpy as np
import pytest
import torch

from test_bone_loss_host import _geometry, _length, bone_grad_f64, bone_loss_f64

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL, SLACK = 2.0 ** -22, 2.0 ** -40
LAM_LEN, LAM_DIR, MIN_CONF, MIN_LEN = 0.7, 0.3, 0.3, 1.0
G_LEN, G_DIR = 0.75, 1.5  # upstream gradients of the two losses (exact in fp32)

SHAPES = [(1, 1, 3, 2), (2, 3, 5, 4), (1, 2, 121, 108), (3, 64, 121, 108), (5, 65, 121, 108)]
_ids = lambda s: "B%d_T%d_K%d_E%d" % s  # noqa: E731
TERMS = {"length": (LAM_LEN, 0.0), "direction": (0.0, LAM_DIR), "both": (LAM_LEN, LAM_DIR)}
WEIGHTS = {"unit": None, "w_1_0.5_2": (1.0, 0.5, 2.0), "w_0_1_1": (0.0, 1.0, 1.0)}


@pytest.fixture(scope="module")
def ops():
    from speechdrivestemplates_amd import ops
    return ops


def _skeleton(K, E):
    """(edges, root): the 121-keypoint skeleton with its part roots; a three-keypoint chain; five keypoints of which 2 and 3 hang off 1, with
    the limbs (1, 2) from the root into its part and (4, 2) from outside into it"""
    from speechdrivestemplates_amd.core.datasets.gesture_dataset import PoseTransforms
    if K == 121:
        return PoseTransforms.skeleton_edges(), PoseTransforms.part_roots(True)
    if K == 3:
        return [(0, 1), (1, 2)], [-1, -1, -1]
    assert (K, E) == (5, 4)
    return [(0, 1), (1, 2), (2, 3), (4, 2)], [-1, -1, 1, 1, -1]


def _edge_w(parts, edges, K):
    if parts is None:
        return None
    from speechdrivestemplates_amd.core.datasets.gesture_dataset import PoseTransforms
    table = PoseTransforms.part_table() if K == 121 else [k % 3 for k in range(K)]
    return [parts[table[a]] for a, _ in edges]


def _data(shape, seed=0):
    B, T, K, _ = shape
    gen = torch.Generator().manual_seed(1000 * seed + 97 * B + 13 * T + K)
    pred, gt = torch.randn(B, T, 2, K, generator=gen), torch.randn(B, T, 2, K, generator=gen)
    mean = 20.0 * torch.randn(B, 2 * K, generator=gen, dtype=torch.float64)
    std = 2.0 + 28.0 * torch.rand(B, 2 * K, generator=gen, dtype=torch.float64)
    score = torch.rand(B, T, 1, K, generator=gen).expand(B, T, 2, K).contiguous()  # the confidence of a keypoint, repeated over x / y
    return pred, gt, mean, std, score


def _kernel(ops, pred, gt, mean, std, score, edges, root, edge_w, lams=(LAM_LEN, LAM_DIR), min_len=MIN_LEN, min_conf=MIN_CONF):
    table = ops.BoneTable(edges, root, edge_w)
    p = pred.to(DEV).requires_grad_(True)
    bone, bdir = ops.BoneLossFn.apply(p, gt.to(DEV), mean.to(DEV), std.to(DEV), None if score is None else score.to(DEV), table,
                                      lams[0], lams[1], None if score is None else min_conf, min_len)
    torch.autograd.backward([bone, bdir], [torch.tensor(G_LEN, device=DEV), torch.tensor(G_DIR, device=DEV)])
    torch.cuda.synchronize()
    return bone.detach().cpu(), bdir.detach().cpu(), p.grad.cpu()


def _close_loss(name, got, want):
    got = float(got)
    print("  %-4s kernel %.9g  float64 %.17g  rel.err %.3g" % (name, got, want, abs(got - want) / abs(want) if want else abs(got)))
    if want == 0.0:
        assert got == 0.0, "%s: expected exactly 0, got %r" % (name, got)
    else:
        assert abs(got - want) <= REL * abs(want), "%s: kernel %.9g vs float64 %.17g" % (name, got, want)


def _close_grad(got, want, terms):
    assert torch.isfinite(got).all()
    empty = terms == 0
    assert not want[empty].any()
    assert torch.equal(got[empty], torch.zeros_like(got[empty])), "non-zero gradient where nothing contributes"
    err = (got.double() - want).abs()
    bound = REL * want.abs() + SLACK * terms
    live = ~empty
    ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
    rel = float((err[live] / terms[live]).max()) if live.any() else 0.0
    print("  grad: %d elements, %d without a term, worst error / bound %.3g, worst error / sum|terms| %.3g"
          % (got.numel(), int(empty.sum()), ratio, rel))
    assert bool((err <= bound).all()), ratio


def _check(ops, pred, gt, mean, std, score, edges, root, edge_w, lams=(LAM_LEN, LAM_DIR), min_len=MIN_LEN):
    mc = None if score is None else MIN_CONF
    bone, bdir, grad = _kernel(ops, pred, gt, mean, std, score, edges, root, edge_w, lams, min_len)
    bone64, bdir64 = (float(x) for x in bone_loss_f64(pred, gt, mean, std, edges, root, score, mc, edge_w, lams[0], lams[1], min_len))
    grad64, terms = bone_grad_f64(pred, gt, mean, std, edges, root, score, mc, edge_w, lams[0], lams[1], min_len, G_LEN, G_DIR)
    _close_loss("bone", bone, bone64)
    _close_loss("dir", bdir, bdir64)
    _close_grad(grad, grad64, terms)
    return bone64, bdir64, grad64, terms


@pytest.mark.parametrize("weights", list(WEIGHTS))
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("terms", list(TERMS))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_shapes_and_options(ops, shape, terms, masked, weights):
    pred, gt, mean, std, score = _data(shape)
    edges, root = _skeleton(shape[2], shape[3])
    assert len(edges) == shape[3]
    bone64, bdir64, grad64, _ = _check(ops, pred, gt, mean, std, score if masked else None, edges, root,
                                       _edge_w(WEIGHTS[weights], edges, shape[2]), TERMS[terms])
    if not masked or shape[2] == 121:  # (the mask may leave nothing of the two small skeletons)
        assert (bone64 > 0) == (terms != "direction") and (bdir64 > 0) == (terms != "length") and bool(grad64.any())


def test_one_consumed_output_and_none(ops):
    """backward with only one of the two losses consumed (the other's upstream gradient is None), and with neither (no launch)"""
    shape = (2, 3, 5, 4)
    pred, gt, mean, std, score = _data(shape, seed=6)
    edges, root = _skeleton(5, 4)
    table = ops.BoneTable(edges, root)
    for which in (0, 1):
        p = pred.to(DEV).requires_grad_(True)
        out = ops.BoneLossFn.apply(p, gt.to(DEV), mean.to(DEV), std.to(DEV), score.to(DEV), table, LAM_LEN, LAM_DIR, MIN_CONF, MIN_LEN)
        out[which].backward()
        torch.cuda.synchronize()
        g = [0.0, 0.0]
        g[which] = 1.0
        grad64, terms = bone_grad_f64(pred, gt, mean, std, edges, root, score, MIN_CONF, None, LAM_LEN, LAM_DIR, MIN_LEN, *g)
        _close_grad(p.grad.cpu(), grad64, terms)
    p = pred.to(DEV).requires_grad_(True)
    out = ops.BoneLossFn.apply(p, gt.to(DEV), mean.to(DEV), std.to(DEV), None, table, LAM_LEN, LAM_DIR, None, MIN_LEN)
    (p.sum() * 2.0).backward()
    assert float(out[0]) > 0 and torch.equal(p.grad, torch.full_like(p, 2.0))


def test_no_edges(ops):
    pred, gt, mean, std, score = _data((2, 3, 5, 0), seed=7)
    bone, bdir, grad = _kernel(ops, pred, gt, mean, std, score, [], [-1, -1, 1, 1, -1], None)
    assert float(bone) == 0.0 and float(bdir) == 0.0 and not grad.any()


def _live_keypoints(score, root):
    """(B, T, K): the keypoints whose own scores and whose root's scores are above the threshold"""
    s = score > MIN_CONF
    own = s[:, :, 0] & s[:, :, 1]
    root = torch.tensor(root)
    return own & ((root < 0) | own[..., root.clamp(min=0)])


def _mask_scores(kind, shape, root):
    B, T, K, _ = shape
    gen = torch.Generator().manual_seed(5)
    live = MIN_CONF + 0.01 + 0.6 * torch.rand(B, T, 1, K, generator=gen)  # everything above the threshold
    if kind == "random30":
        s = torch.rand(B, T, 1, K, generator=gen)  # about 30 % at or below 0.3
    elif kind == "all_masked":
        s = torch.zeros(B, T, 1, K)
    elif kind == "one_keypoint":
        s = live.clone()
        s[..., K // 2] = 0.0
    elif kind == "masked_root":
        s = live.clone()
        s[..., max(root)] = 0.0  # (the head root of the skeleton; keypoint 1 of the five)
    elif kind == "at_threshold":
        s = live.clone()
        s[torch.rand(B, T, 1, K, generator=gen) < 0.25] = MIN_CONF  # stored as fp32(0.3): equal, and the comparison is strict
    return s.expand(B, T, 2, K).contiguous()


@pytest.mark.parametrize("kind", ["random30", "all_masked", "one_keypoint", "masked_root", "at_threshold"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 4), (3, 64, 121, 108)], ids=_ids)
def test_mask_patterns(ops, shape, kind):
    pred, gt, mean, std, _ = _data(shape, seed=1)
    K = shape[2]
    edges, root = _skeleton(K, shape[3])
    score = _mask_scores(kind, shape, root)
    bone64, bdir64, grad64, terms = _check(ops, pred, gt, mean, std, score, edges, root, _edge_w((1.0, 0.5, 2.0), edges, K))
    live = _live_keypoints(score, root)
    assert not grad64[~live[:, :, None].expand_as(grad64)].any()
    if kind == "random30":
        assert 0.3 * live.numel() < int(live.sum()) < 0.8 * live.numel() and bone64 > 0 and bdir64 > 0
    if kind == "all_masked":
        assert not live.any() and bone64 == 0.0 and bdir64 == 0.0 and not terms.any()
    if kind == "one_keypoint":
        assert int((~live).sum()) == live.numel() // K and bone64 > 0
    if kind == "masked_root":  # the whole part goes dead with its root
        r = max(root)
        part = [k for k in range(K) if root[k] == r]
        assert part and not live[..., part + [r]].any() and bool(live[..., [k for k in range(K) if k not in part + [r]]].all())
        assert not terms[..., part].any() and (bone64 > 0) == (K == 121)  # (every limb of the five touches the part of 1)
    if kind == "at_threshold":
        at = (score == torch.tensor(MIN_CONF, dtype=torch.float32))[:, :, 0]
        assert at.any() and not (live & at).any() and bone64 > 0


@pytest.mark.parametrize("shape", [(2, 3, 5, 4), (3, 64, 121, 108)], ids=_ids)
def test_degenerate_limbs(ops, shape):
    """pred == gt on a block (length term and its gradient exactly 0 there); a predicted limb of zero length (unit std and zero mean make
    the two ends equal to the bit: no length gradient, no direction term); true limbs under the floor of the divisor"""
    B, T, K, E = shape
    edges, root = _skeleton(K, E)
    pred, gt, mean, std, score = _data(shape, seed=2)
    mean, std = torch.zeros_like(mean), torch.ones_like(std)
    pred[0] = gt[0]  # clip 0
    a, b = edges[-2]  # (2, 3) of the five, both in the part of 1; a finger segment of the right hand
    assert root[a] == root[b]
    pred[1, :, :, b] = pred[1, :, :, a]
    for sc in (None, score):
        bone64, bdir64, grad64, terms = _check(ops, pred, gt, mean, std, sc, edges, root, _edge_w((1.0, 0.5, 2.0), edges, K))
        assert not grad64[0].any() and not terms[0].any() and bool(grad64[1].any()) and bone64 > 0
    m, vp, vg, _, _, _, _, _ = _geometry(pred, gt, mean, std, edges, root, None, None)
    assert not _length(vp)[1, :, E - 2].any() and bool(_length(vp)[1, :, :E - 2].all())
    # the floor: with min_len = 2 a good share of the true limbs (unit std: lengths around 1.8) divides by the floor instead
    lg = _length(vg)
    assert 0.2 * lg.numel() < int((lg < 2.0).sum()) < 0.9 * lg.numel()
    pred2 = _data(shape, seed=3)[0]
    with_floor = _check(ops, pred2, gt, mean, std, score, edges, root, None, min_len=2.0)
    without = bone_loss_f64(pred2, gt, mean, std, edges, root, score, MIN_CONF, None, LAM_LEN, LAM_DIR, 2.0 ** -20)
    assert with_floor[0] < float(without[0]) and with_floor[1] == float(without[1])


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_nothing_under_the_mask_leaks(ops):
    """No tolerance here.  pred, gt and the scores at the dead keypoints are overwritten with 1e6, then with NaN: both losses and every
    bit of dpred must be those of the unperturbed call (a dead limb is selected away; 0 * NaN would be NaN).  And a second call of the
    same inputs gives the same bits."""
    shape = (3, 64, 121, 108)
    pred, gt, mean, std, score = _data(shape, seed=3)
    edges, root = _skeleton(121, 108)
    w = _edge_w((1.0, 0.5, 2.0), edges, 121)
    dead = ~_live_keypoints(score, root)[:, :, None].expand_as(pred)
    assert 0.2 * dead.numel() < int(dead.sum()) < 0.8 * dead.numel()
    base = _kernel(ops, pred, gt, mean, std, score, edges, root, w)
    assert all(torch.isfinite(t).all() for t in base) and float(base[0]) > 0 and float(base[1]) > 0 and not base[2][dead].any()
    again = _kernel(ops, pred, gt, mean, std, score, edges, root, w)
    for name, x, y in zip(("bone", "dir", "dpred"), again, base):
        assert torch.equal(_bits(x), _bits(y)), "%s differs between two calls" % name
    own_dead = ~(score > MIN_CONF)
    for junk in (1e6, float("nan")):
        p2, g2, s2 = pred.clone(), gt.clone(), score.clone()
        p2[dead], g2[dead] = junk, junk
        if junk != junk:
            s2[own_dead] = junk  # NaN > c is false: still dead
        got = _kernel(ops, p2, g2, mean, std, s2, edges, root, w)
        for name, x, y in zip(("bone", "dir", "dpred"), got, base):
            assert torch.equal(_bits(x), _bits(y)), "%s changed with %r under the mask" % (name, junk)


def test_two_calls_give_the_same_bits(ops):
    shape = (5, 65, 121, 108)
    pred, gt, mean, std, score = _data(shape, seed=4)
    edges, root = _skeleton(121, 108)
    a = _kernel(ops, pred, gt, mean, std, score, edges, root, None)
    b = _kernel(ops, pred, gt, mean, std, score, edges, root, None)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


# =============================================================================================================================
# model level: the tiny voice2pose_sdt_bp set-up of tests/test_optim_guard_gpu.py (4 synthetic clips), batches of 2
# =============================================================================================================================
KEYS_ON = ["VOICE2POSE.GENERATOR.LAMBDA_BONE", 0.5, "VOICE2POSE.GENERATOR.LAMBDA_BONE_DIR", 0.25, "VOICE2POSE.GENERATOR.BONE_MIN_LENGTH", 2.0,
           "VOICE2POSE.GENERATOR.REG_MIN_CONFIDENCE", 0.3, "VOICE2POSE.GENERATOR.REG_PART_WEIGHTS", [1.0, 0.5, 2.0]]


def _scored_batch(step, seed):
    """the batch of ``step`` with scores and speaker statistics drawn from ``seed``"""
    from test_optim_guard_gpu import _batch
    b = _batch(step, b=2)
    rng = np.random.Generator(np.random.PCG64([79, seed]))
    b["poses_score"] = torch.from_numpy(np.repeat(rng.uniform(0, 1, (2, 64, 1, 121)).astype(np.float32), 2, axis=2))
    stat = dict(b["speaker_stat"])
    stat["mean"] = torch.from_numpy(rng.standard_normal((2, 242)) * 20.0)
    stat["std"] = torch.from_numpy(rng.uniform(2.0, 30.0, (2, 242)))
    b["speaker_stat"] = stat
    return b


def _to_device(b, dev):
    b = {k: (v.to(dev) if torch.is_tensor(v) and k != "num_frames" else v) for k, v in b.items()}
    b["speaker_stat"] = {k: v.to(dev) for k, v in b["speaker_stat"].items()}
    return b


def test_default_keys_never_enter_the_op(ops, monkeypatch):
    from test_optim_guard_gpu import _batch, _pipe

    def boom(*a, **k):
        raise AssertionError("the default step entered ops.BoneLossFn")

    pipe = _pipe()
    assert pipe.model.bone_opts is None and pipe.model.bone_table is None
    monkeypatch.setattr(ops.BoneLossFn, "apply", boom)
    losses, _ = pipe.forward_backward(_batch(0, b=2))
    assert list(losses) == ["G_reg_loss", "G_clipcode_kl_loss", "G_loss", "L2_dist", "lip_sync_error_n"]
    torch.cuda.synchronize()
    pipe.close()


def test_model_step_with_the_keys_on(ops):
    from speechdrivestemplates_amd.core.datasets.gesture_dataset import PoseTransforms
    from test_optim_guard_gpu import _pipe
    pipe = _pipe(KEYS_ON)
    optg = pipe.optimizers["optimizerG"]
    batch = _scored_batch(0, 0)

    def step(b):
        losses, results = pipe.forward_backward(b)
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in losses.items()}, optg.flat_grad.detach().clone(), results

    l0, g0, results = step(batch)
    assert list(l0) == ["G_reg_loss", "G_bone_loss", "G_bone_dir_loss", "G_clipcode_kl_loss", "G_loss", "L2_dist", "lip_sync_error_n"]
    assert float(l0["G_bone_loss"]) > 0 and float(l0["G_bone_dir_loss"]) > 0 and torch.isfinite(g0).all() and bool(g0.any())
    total = ((l0["G_reg_loss"] + l0["G_bone_loss"]) + l0["G_bone_dir_loss"]) + l0["G_clipcode_kl_loss"]
    assert torch.equal(_bits(l0["G_loss"]), _bits(total))
    # the two terms are those of the float64 model on this step's prediction
    pred = results["poses_pred_normalized"].detach().cpu()
    edges = PoseTransforms.skeleton_edges()
    bone64, bdir64 = bone_loss_f64(pred, batch["poses"], batch["speaker_stat"]["mean"], batch["speaker_stat"]["std"], edges,
                                   PoseTransforms.part_roots(True), batch["poses_score"], 0.3, _edge_w((1.0, 0.5, 2.0), edges, 121),
                                   0.5, 0.25, 2.0)
    _close_loss("bone", l0["G_bone_loss"], float(bone64))
    _close_loss("dir", l0["G_bone_dir_loss"], float(bdir64))
    # the same step again: the same bits
    l1, g1, _ = step(batch)
    names = ("G_reg_loss", "G_bone_loss", "G_bone_dir_loss", "G_loss")
    assert torch.equal(_bits(g1), _bits(g0)) and all(torch.equal(_bits(l1[k]), _bits(l0[k])) for k in names)
    pipe.close()


def test_hipgraph_replay_follows_speaker_stat_and_scores(ops):
    """SYS.HIP_GRAPH with the limb losses on: one eager warm-up step, the capture, then replays with two more sets of speaker statistics
    and scores; every step's losses carry the bits of the eager run on the same inputs (both are static inputs of the graph)."""
    from speechdrivestemplates_amd.graph import GraphedStep
    from test_optim_guard_gpu import _pipe
    names = ("G_reg_loss", "G_bone_loss", "G_bone_dir_loss", "G_loss")
    runs = []
    for use_graph in (False, True):
        pipe = _pipe(KEYS_ON + ["SYS.HIP_GRAPH", True])
        dev = pipe.model._device()
        gs = GraphedStep(pipe, warmup=1)
        hist = []
        for step in range(4):
            b = _to_device(_scored_batch(step % 2, seed=step), dev)  # (steps 2 and 3: the batches of steps 0 and 1 with other statistics)
            if use_graph:
                losses = gs.run(b)
            else:
                losses, _ = pipe.forward_backward(b)
                pipe.optimizer_updates(losses)
            torch.cuda.synchronize()
            hist.append({k: losses[k].detach().clone() for k in names})
        if use_graph:
            assert gs.segments is not None and [k for k, _ in gs.segments] == ["graph"]
            assert all(t.is_cuda and t.dtype == torch.float64 for t in (gs.static["speaker_stat"]["mean"], gs.static["speaker_stat"]["std"]))
        runs.append(hist)
        pipe.close()
    for i, (a, b) in enumerate(zip(*runs)):
        print("  step %d eager %s  graph %s" % (i, [float(a[k]) for k in names], [float(b[k]) for k in names]))
    for i, (a, b) in enumerate(zip(*runs)):
        for k in names:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (i, k, float(a[k]), float(b[k]))
    assert not torch.equal(_bits(runs[1][1]["G_bone_loss"]), _bits(runs[1][3]["G_bone_loss"]))  # (the replays did see different inputs)
