"""Optimiser-side safeguards on the GPU (csrc/optim_guard.hip, optim.StepGuard, FlatAdam's EMA): the ordered
float64 sum of squares against its numpy contract model, the guarded Adam step against sdt_adam_step_f32 (bit for bit when nothing is
asked of it) and against a float64 torch.optim.Adam + clip_grad_norm_ oracle, the skipped step, the EMA, and the pipeline level:
logged norm, checkpoint / resume, evaluation on the EMA weights, hipGraph replay and two ranks.

Bar of every float64 comparison: rel-max-err < 1e-6, what tests/test_edge_shapes_gpu.py holds sdt_adam_step_f32 to."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO

pytestmark = pytest.mark.gpu

DEV = "cuda"
ADAM_TOL = 1e-6
SIZES = [1, 3, 4, 5, 255, 256, 257, "block+1", "sumsq_pass+1", "adam_pass+1"]


@pytest.fixture(scope="module")
def ops():
    from speechdrivestemplates_amd import ops as o
    return o


def _n(ops, spec):
    """buffer lengths: one more than a full block of float4s, one more than what one grid pass of each launch as built covers"""
    if spec == "block+1":
        return 256 * 4 + 1
    if spec == "sumsq_pass+1":
        return ops.optim_guard_pass_elems("sumsq") + 1
    if spec == "adam_pass+1":
        return ops.optim_guard_pass_elems("adam") + 1
    return int(spec)


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "non-finite values in kernel output"
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def check(name, got, ref, tol=ADAM_TOL):
    e = rel_err(got, ref)
    print("  %-52s rel-max-err %.3e (tol %.1e)" % (name, e, tol))
    assert e < tol, "%s: %.3e >= %.1e" % (name, e, tol)


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64).cpu()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# =============================================================================================================================
# kernel level
# =============================================================================================================================
def _sumsq(ops, g, partial):
    ops.grad_sumsq(g, partial)
    torch.cuda.synchronize()
    return partial[0:1].clone()


def _wide_values(n, seed):
    """fp32 values over forty decades; 1e-30 and 1e19 among them (their squares underflow / overflow fp32)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = (rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))).astype(np.float32)
    variants = [rng.standard_normal(n).astype(np.float32) + np.float32(3)]  # every element counts in the last bits: the ORDER is tested here
    if n >= 2:
        g[0], g[-1] = np.float32(1e-30), np.float32(1e19)
        variants.append(g)
    else:
        variants += [np.array([1e-30], dtype=np.float32), np.array([1e19], dtype=np.float32)]
    return variants


@pytest.mark.parametrize("spec", SIZES)
def test_sum_of_squares_is_the_contract_models_bits(ops, spec):
    from speechdrivestemplates_amd import optim
    n = _n(ops, spec)
    partial = torch.full((ops.grad_sumsq_partials(),), float("nan"), device=DEV, dtype=torch.float64)  # contents must not matter
    for g in _wide_values(n, 100 + n % 1000):
        buf = torch.full(((n + 3) // 4 * 4 + 4,), float("inf"), device=DEV)  # anything read past n would make the sum non-finite
        buf[:n] = torch.from_numpy(g).to(DEV)
        a = _sumsq(ops, buf[:n], partial)
        b = _sumsq(ops, buf[:n], partial)
        model = torch.from_numpy(np.array([optim.sumsq_model(g)]))
        print("  n=%d sum of squares %.17e (model %.17e)" % (n, a.item(), model.item()))
        assert np.isfinite(model.item()) and model.item() > 0
        assert same_bits(a, b), "two calls differ"
        assert same_bits(a, model), "kernel %r, contract model %r" % (a.item(), model.item())
        if g.min() == np.float32(1e-30) or g.max() == np.float32(1e19):  # (an fp32 accumulator gives 0 / inf here)
            assert a.item() != float(np.sum(g.astype(np.float32) ** 2, dtype=np.float32))
    # a NaN, then a +inf, at the first element, the last vector element and the last tail element
    base = torch.ones(n, device=DEV)
    spots = {0}
    if n >= 4:
        spots.add(4 * (n // 4) - 1)
    if n % 4:
        spots.add(n - 1)
    for bad in (float("nan"), float("inf")):
        for pos in sorted(spots):
            buf = torch.ones((n + 3) // 4 * 4, device=DEV)
            buf[pos] = bad
            assert not np.isfinite(_sumsq(ops, buf[:n], partial).item()), (n, pos, bad)
    assert _sumsq(ops, base, partial).item() == float(n)


class Group:
    """A step group of flat buffers driven through the raw entry points: sdt_grad_sumsq_f64 per buffer, sdt_optim_guard_prep once,
    sdt_adam_step_guarded_f32 per buffer.  Buffers are padded with sentinels: a write past n fails ``check_padding``."""
    FILL = {"p": 7.0, "g": 11.0, "m": 5.0, "v": 3.0, "ema": 13.0}

    def __init__(self, ops, p0s, ema=False):
        self.ops, self.ns, self.bufs = ops, [p.numel() for p in p0s], []
        for p0 in p0s:
            n = p0.numel()
            b = {k: torch.full(((n + 3) // 4 * 4 + 8,), s, device=DEV) for k, s in self.FILL.items()}
            b["p"][:n] = p0.to(DEV)
            b["m"][:n] = 0.0
            b["v"][:n] = 0.0
            b["ema"][:n] = p0.to(DEV)  # the EMA starts as the parameters
            b["state"] = torch.zeros(2, dtype=torch.int64, device=DEV)
            b["partial"] = torch.zeros(ops.grad_sumsq_partials(), dtype=torch.float64, device=DEV)
            self.bufs.append(b)
        self.use_ema = ema
        self.lr = torch.zeros(1, device=DEV)
        self.record = torch.zeros(ops.GUARD_WORDS, dtype=torch.int64, device=DEV)

    def step(self, grads, lr=1e-3, grad_scale=1.0, max_norm=0.0, skip=False, eps=1e-8, decay=0.0):
        self.lr.fill_(lr)
        for b, n, g in zip(self.bufs, self.ns, grads):
            b["g"][:n] = g.to(DEV)
            self.ops.grad_sumsq(b["g"][:n], b["partial"])
        self.ops.optim_guard_prep([b["partial"] for b in self.bufs], self.record, grad_scale, max_norm, skip)
        for b, n in zip(self.bufs, self.ns):
            self.ops.adam_step_guarded(b["p"][:n], b["g"][:n], b["m"][:n], b["v"][:n], self.lr, b["state"], self.record, eps=eps,
                                       ema=b["ema"][:n] if self.use_ema else None, ema_decay=decay)
        torch.cuda.synchronize()

    def snapshot(self):
        return [{k: b[k][:n].clone() if k != "state" else b[k].clone() for k in ("p", "m", "v", "ema", "state")} for b, n in zip(self.bufs, self.ns)]

    def norm(self):
        return self.record.view(torch.float64)[0].item()

    def skipped(self):
        return int(self.record[2].item())

    def steps(self):
        return [int(b["state"][0].item()) for b in self.bufs]

    def check_padding(self):
        for b, n in zip(self.bufs, self.ns):
            for k, s in self.FILL.items():
                if k == "g":
                    continue
                assert bool((b[k][n:] == s).all()), "the guarded step wrote past n into the %s buffer" % k


def _data(n, steps, seed, scales=None):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (1.0 if scales is None else scales[i]) for i in range(steps)]
    return p0, grads


@pytest.mark.parametrize("spec", SIZES)
def test_guarded_step_that_guards_nothing_is_the_plain_step_bit_for_bit(ops, spec):
    n = _n(ops, spec)
    p0, grads = _data(n, 3, 200 + n % 1000)
    for gscale in (1.0, 0.5):
        grp = Group(ops, [p0])
        plain = {k: torch.zeros((n + 3) // 4 * 4, device=DEV) for k in ("p", "g", "m", "v")}
        plain["p"][:n] = p0.to(DEV)
        lr, state = torch.full((1,), 1e-3, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
        for g in grads:
            grp.step([g], grad_scale=gscale, max_norm=0.0)
            plain["g"][:n] = g.to(DEV)
            ops.adam_step(plain["p"][:n], plain["g"][:n], plain["m"][:n], plain["v"][:n], lr, state, grad_scale=gscale)
        torch.cuda.synchronize()
        got = grp.snapshot()[0]
        for k in ("p", "m", "v"):
            assert same_bits(got[k], plain[k][:n]), (k, n, gscale)
        assert same_bits(got["state"], state) and grp.steps() == [3] and grp.skipped() == 0
        grp.check_padding()


class Oracle:
    """float64 CPU statement: torch.optim.Adam over the group's tensors, torch.nn.utils.clip_grad_norm_ over all of them, the EMA."""

    def __init__(self, p0s, lr=1e-3, eps=1e-8, decay=None):
        self.ps = [p.double().clone().requires_grad_(True) for p in p0s]
        self.opt = torch.optim.Adam(self.ps, lr=lr, eps=eps)
        self.decay = decay
        self.ema = [p.detach().clone() for p in self.ps]

    def step(self, grads, grad_scale=1.0, max_norm=None):
        for p, g in zip(self.ps, grads):
            p.grad = g.double() * grad_scale  # the gradient Adam consumes
        norm = torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1) for p in self.ps])).item()
        if max_norm:
            torch.nn.utils.clip_grad_norm_(self.ps, max_norm, norm_type=2, error_if_nonfinite=False)
        self.opt.step()
        if self.decay is not None:
            self.ema = [self.decay * e + (1 - self.decay) * p.detach() for e, p in zip(self.ema, self.ps)]
        return norm


CLIP_NS, CLIP_SCALES, MAX_NORM, CLIP_EPS = (257, 5), (3.0, 1.5, 0.2), 10.0, 1e-2


@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_clipping_matches_clip_grad_norm_and_adam_in_float64(ops, gscale):
    """eps = 1e-2: Adam is invariant to the gradient's scale up to eps, so a small eps would hide a wrong clip coefficient"""
    max_norm = MAX_NORM * gscale
    data = [_data(n, 3, 300 + n, CLIP_SCALES) for n in CLIP_NS]
    p0s, grads = [d[0] for d in data], [[d[1][s] for d in data] for s in range(3)]
    ref, unclipped = Oracle(p0s, eps=CLIP_EPS), Oracle(p0s, eps=CLIP_EPS)
    grp = Group(ops, p0s)
    norms = []
    for s in range(3):
        norm = ref.step(grads[s], gscale, max_norm)
        unclipped.step(grads[s], gscale, None)
        norms.append(norm)
        assert abs(norm - max_norm) >= 0.1 * max_norm, "the oracle's norm %.4f is too close to max_norm %.4f" % (norm, max_norm)
        grp.step(grads[s], grad_scale=gscale, max_norm=max_norm, eps=CLIP_EPS)
        print("  step %d: norm oracle %.9f kernel %.9f (max_norm %.2f)" % (s + 1, norm, grp.norm(), max_norm))
        assert abs(grp.norm() - norm) <= 1e-6 * norm
    assert norms[0] > 1.1 * max_norm and norms[2] < 0.9 * max_norm  # step 1 clips, step 3 does not
    for i, snap in enumerate(grp.snapshot()):
        check("clipped Adam n=%d grad_scale=%g" % (CLIP_NS[i], gscale), snap["p"], ref.ps[i].detach())
    assert rel_err(unclipped.ps[0].detach(), ref.ps[0].detach()) > 1e-5  # the clip moves the result by far more than the bar
    assert grp.steps() == [3, 3] and grp.skipped() == 0
    grp.check_padding()


def test_a_non_finite_step_is_skipped_whole(ops):
    data = [_data(n, 3, 400 + n) for n in CLIP_NS]
    p0s, grads = [d[0] for d in data], [[d[1][s] for d in data] for s in range(3)]
    grads[1][1] = grads[1][1].clone()
    grads[1][1][2] = float("inf")  # one inf, in the second buffer: the first buffer's step is skipped with it
    grp = Group(ops, p0s, ema=True)
    ref = Oracle(p0s, decay=0.5)
    grp.step(grads[0], skip=True, decay=0.5)
    ref.step(grads[0])
    after1 = grp.snapshot()
    grp.step(grads[1], skip=True, decay=0.5)
    assert not np.isfinite(grp.norm()) and grp.skipped() == 1 and grp.steps() == [1, 1]
    for a, b in zip(after1, grp.snapshot()):
        for k in ("p", "m", "v", "ema", "state"):
            assert same_bits(a[k], b[k]), "the skipped step changed %s" % k
    grp.step(grads[2], skip=True, decay=0.5)
    ref.step(grads[2])  # the oracle never saw step 2: its bias correction is that of the second applied step
    assert grp.steps() == [2, 2] and grp.skipped() == 1 and np.isfinite(grp.norm())
    for i, snap in enumerate(grp.snapshot()):
        check("after a skipped step n=%d p" % CLIP_NS[i], snap["p"], ref.ps[i].detach())
        check("after a skipped step n=%d ema" % CLIP_NS[i], snap["ema"], ref.ema[i])
    grp.check_padding()
    # the key off: the same input makes the parameters non-finite, as torch's do
    loose = Group(ops, p0s)
    torch_ref = Oracle(p0s)
    for s in range(2):
        loose.step(grads[s], skip=False)
        torch_ref.step(grads[s])
    assert loose.skipped() == 0 and loose.steps() == [2, 2]
    assert not torch.isfinite(torch_ref.ps[1]).all() and not torch.isfinite(loose.snapshot()[1]["p"]).all()


@pytest.mark.parametrize("decay", [0.5, 0.999])
@pytest.mark.parametrize("spec,skip_mid", [(5, False), (257, False), (257, True), ("adam_pass+1", False)])
def test_ema_in_the_same_pass(ops, decay, spec, skip_mid):
    n = _n(ops, spec)
    p0, grads = _data(n, 3, 500 + n % 1000)
    if skip_mid:
        grads[1][n - 1] = float("nan")
    grp = Group(ops, [p0], ema=True)
    ref = Oracle([p0], decay=decay)
    assert same_bits(grp.snapshot()[0]["ema"], p0.to(DEV))  # the EMA equals the parameters before the first step
    for s, g in enumerate(grads):
        before = grp.snapshot()[0]["ema"]
        grp.step([g], skip=True, decay=decay)
        if skip_mid and s == 1:
            assert same_bits(before, grp.snapshot()[0]["ema"]) and grp.skipped() == 1
        else:
            ref.step([g])
    snap = grp.snapshot()[0]
    check("EMA d=%g n=%d" % (decay, n), snap["ema"], ref.ema[0])
    check("EMA d=%g n=%d parameters" % (decay, n), snap["p"], ref.ps[0].detach())
    assert rel_err(snap["ema"], snap["p"]) > 1e-5  # (an average, not a copy)
    grp.check_padding()


# =============================================================================================================================
# pipeline level: the tiny voice2pose_sdt_bp set-up (4 synthetic clips)
# =============================================================================================================================
N_CLIPS = 4


def _cfg(extra=()):
    from speechdrivestemplates_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(REPO, "configs", "voice2pose_sdt_bp.yaml"))
    cfg.merge_from_list(["DATASET.NAME", "SyntheticGestureDataset", "DATASET.SYNTHETIC_CLIPS", N_CLIPS, "SYS.LOG_INTERVAL", 10 ** 9,
                         "TRAIN.BATCH_SIZE", 4, "TEST.BATCH_SIZE", 4, "SYS.NUM_WORKERS", 0, "TRAIN.LR_SCHEDULER", False,
                         "TRAIN.SAVE_VIDEO", False, "TEST.SAVE_VIDEO", False, "TEST.SAVE_NPZ", False] + list(extra))
    cfg.freeze()
    return cfg


def _pipe(extra=(), n_clips=N_CLIPS):
    """pipeline on the oracle's seeded initial state (as __graft_entry__.make_pipeline builds it)"""
    from oracle import sdt_oracle as O
    from speechdrivestemplates_amd.core.datasets import gesture_dataset as gd
    from speechdrivestemplates_amd.core.pipelines import get_pipeline
    cfg = _cfg(["DATASET.SYNTHETIC_CLIPS", n_clips] + list(extra))
    pipe = get_pipeline(cfg.PIPELINE_TYPE)(cfg)
    pipe.num_train_samples = n_clips
    pipe.train_dataset = gd.SyntheticGestureDataset(cfg=cfg, num_clips=n_clips)
    state = O.make_voice2pose_state(O.cfg_named("voice2pose_sdt_bp"), n_clips, seed=0, code_std=0.5)
    pipe.setup_model(cfg, state_dict={"module." + k: v for k, v in state.items()})
    pipe.setup_optimizer()
    pipe.model.train()
    return pipe


def _batch(step, n_clips=N_CLIPS, b=4, inf_audio=False):
    from oracle import sdt_oracle as O
    batch = O.make_batch(b, n_clips, step=step, seed=1)
    if inf_audio:
        batch["audio"][b - 1, 1000] = float("inf")
    return batch


def test_defaults_build_no_guard_and_no_ema():
    pipe = _pipe()
    assert pipe.step_guards == {} and all(o.guard is None and o.ema is None for o in pipe.optimizers.values())
    losses, _ = pipe.forward_backward(_batch(0))
    pipe.optimizer_updates(losses)
    assert not any(k.startswith(("grad_norm", "skipped_steps")) for k in losses)
    assert "model_ema_state_dict" not in pipe.checkpoint_dict(1, 1)
    pipe.close()


def test_logged_norm_and_clipped_update():
    clip = 1e-5  # far below the observed norm: the clipped gradient's elements come down to Adam's eps, where the scale counts
    pipe = _pipe(["TRAIN.GRAD_CLIP_NORM", clip])
    optg, optc = pipe.optimizers["optimizerG"], pipe.optimizers["optimizerClipCode"]
    losses, _ = pipe.forward_backward(_batch(0))
    torch.cuda.synchronize()
    params = list(pipe.model.netG.parameters()) + [pipe.model.clips_code]
    g64 = torch.cat([p.grad.detach().double().reshape(-1) for p in params]).cpu()
    norm = torch.linalg.vector_norm(g64).item()
    ref = {}
    for name, opt in (("G", optg), ("C", optc)):
        p = opt.flat_param.detach().double().cpu().requires_grad_(True)
        p.grad = opt.flat_grad.detach().double().cpu()
        ref[name] = (p, torch.optim.Adam([p], lr=opt.param_groups[0]["lr"]))
    unclipped = optg.flat_param.detach().double().cpu().requires_grad_(True)
    unclipped.grad = optg.flat_grad.detach().double().cpu()
    torch.optim.Adam([unclipped], lr=optg.param_groups[0]["lr"]).step()
    torch.nn.utils.clip_grad_norm_([ref["C"][0], ref["G"][0]], clip)
    for p, o in ref.values():
        o.step()
    pipe.optimizer_updates(losses)
    torch.cuda.synchronize()
    got = float(losses["grad_norm_G"])
    print("  grad_norm_G %.9e, float64 norm of the p.grad %.9e" % (got, norm))
    assert norm > 100 * clip and abs(got - norm) <= 1e-6 * norm
    assert int(losses["skipped_steps_G"]) == 0
    moved = rel_err(unclipped.detach(), ref["G"][0].detach())
    print("  an unclipped step would differ from the oracle by %.3e" % moved)
    assert moved > 5 * ADAM_TOL  # (the check below tells a clipped step from an unclipped one)
    check("netG after the clipped step", optg.flat_param, ref["G"][0].detach())
    check("clips_code after the clipped step", optc.flat_param, ref["C"][0].detach())
    pipe.close()


def test_checkpoint_resume_and_evaluation_on_the_ema(tmp_path):
    opts = ["TRAIN.EMA_DECAY", 0.5, "SYS.EVAL_WITH_EMA", True, "SYS.OUTPUT_DIR", str(tmp_path)]
    pipe = _pipe(opts)
    pipe.setup_dataset(pipe.cfg, "train")  # (the validation split with it)
    optg = pipe.optimizers["optimizerG"]
    assert same_bits(optg.ema, optg.flat_param)  # initialised to the parameters
    assert "optimizerD_pose" not in pipe.optimizers and pipe.optimizers["optimizerClipCode"].ema is not None
    for step in range(2):
        losses, _ = pipe.forward_backward(_batch(step))
        pipe.optimizer_updates(losses)
    torch.cuda.synchronize()
    assert not same_bits(optg.ema, optg.flat_param)
    ckpt = pipe.checkpoint_dict(1, 2)
    assert list(ckpt["model_ema_state_dict"]) == list(ckpt["model_state_dict"])
    differ = [k for k in ckpt["model_state_dict"] if not torch.equal(ckpt["model_state_dict"][k], ckpt["model_ema_state_dict"][k])]
    averaged = ["module." + n for n, _ in pipe.model.named_parameters() if n.startswith("netG.") or n == "clips_code"]
    assert differ and set(differ) <= set(averaged), set(differ) - set(averaged)
    os.makedirs(str(tmp_path / "run"), exist_ok=True)
    path = str(tmp_path / "run" / "checkpoint_epoch-1_step-2.pth")
    torch.save(ckpt, path)
    # save -> resume restores the EMA bit for bit
    from speechdrivestemplates_amd.core.pipelines import get_pipeline
    resumed = get_pipeline(pipe.cfg.PIPELINE_TYPE)(pipe.cfg)
    resumed.setup_experiment(True, "resume", resume_from=path)
    for name, opt in pipe.optimizers.items():
        assert same_bits(resumed.optimizers[name].ema, opt.ema), name
        assert same_bits(resumed.optimizers[name].flat_param, opt.flat_param), name
    resumed.close()
    # validate() reads the EMA weights and puts the training weights back
    snap = {k: o.flat_param.detach().clone() for k, o in pipe.optimizers.items()}
    ema_snap = {k: o.ema.detach().clone() for k, o in pipe.optimizers.items()}
    torch.manual_seed(0)
    out = pipe.validate(epoch=1)
    torch.cuda.synchronize()
    for k, o in pipe.optimizers.items():
        assert same_bits(o.flat_param, snap[k]) and same_bits(o.ema, ema_snap[k]), k
    plain = get_pipeline(pipe.cfg.PIPELINE_TYPE)(_cfg(["SYS.OUTPUT_DIR", str(tmp_path)]))
    plain.setup_dataset(plain.cfg, "train")
    plain.setup_model(plain.cfg, state_dict=ckpt["model_ema_state_dict"])
    torch.manual_seed(0)
    ref_out = plain.validate(epoch=1)
    plain_w = get_pipeline(pipe.cfg.PIPELINE_TYPE)(_cfg(["SYS.OUTPUT_DIR", str(tmp_path)]))
    plain_w.setup_dataset(plain_w.cfg, "train")
    plain_w.setup_model(plain_w.cfg, state_dict=ckpt["model_state_dict"])
    torch.manual_seed(0)
    train_out = plain_w.validate(epoch=1)
    for k in ("G_reg_loss", "G_loss", "L2_dist", "lip_sync_error_n"):
        a, b, c = float(out[k]), float(ref_out[k]), float(train_out[k])
        print("  validate %-18s on the EMA %.8f, model loaded from model_ema_state_dict %.8f, training weights %.8f" % (k, a, b, c))
        assert abs(a - b) <= 2e-6 * abs(b) + 1e-6, k  # the smoke test's bar for a forward pass on identical weights
    assert float(out["G_reg_loss"]) != float(train_out["G_reg_loss"])  # (not the training weights)
    # ... also when test_step raises

    def boom(*a, **kw):
        raise RuntimeError("test_step failed")

    pipe.test_step = boom
    with pytest.raises(RuntimeError, match="test_step failed"):
        pipe.validate(epoch=1)
    for k, o in pipe.optimizers.items():
        assert same_bits(o.flat_param, snap[k]) and same_bits(o.ema, ema_snap[k]), k
    pipe.close()


ALL_ON = ["TRAIN.GRAD_CLIP_NORM", 1.0, "TRAIN.SKIP_NONFINITE_STEP", True, "TRAIN.EMA_DECAY", 0.9]


def test_hipgraph_replay_of_the_guarded_step_matches_eager():
    """as test_model_gpu.test_hipgraph_replay_matches_eager (same bars): one eager warm-up step, then three replayed steps; the batch
    of the second replayed step carries an inf audio sample: its loss is non-finite and the step is skipped on both paths"""
    from speechdrivestemplates_amd.graph import GraphedStep
    runs = []
    for use_graph in (False, True):
        pipe = _pipe(ALL_ON + ["SYS.HIP_GRAPH", True], n_clips=16)
        dev = pipe.model._device()
        gs = GraphedStep(pipe, warmup=1)
        hist = []
        for step in range(4):
            b = _batch(step, n_clips=16, inf_audio=(step == 2))
            b = {k: (v.to(dev) if torch.is_tensor(v) and k != "num_frames" else v) for k, v in b.items()}
            b["speaker_stat"] = {k: v.to(dev) for k, v in b["speaker_stat"].items()}
            if use_graph:
                losses = gs.run(b)
            else:
                losses, _ = pipe.forward_backward(b)
                pipe.optimizer_updates(losses)
            torch.cuda.synchronize()
            hist.append((float(losses["G_loss"].detach()), float(losses["L2_dist"]), float(losses["grad_norm_G"]), int(losses["skipped_steps_G"])))
        if use_graph:
            assert gs.segments is not None and [k for k, _ in gs.segments] == ["graph"]
        optg = pipe.optimizers["optimizerG"]
        runs.append((hist, optg.flat_param.detach().clone(), optg.ema.detach().clone(), int(optg.state_dev[0]),
                     int(pipe.optimizers["optimizerClipCode"].state_dev[0])))
        pipe.close()
    (h0, w0, e0, s0, c0), (h1, w1, e1, s1, c1) = runs
    print("  eager ", h0)
    print("  graph ", h1)
    assert s0 == s1 == 3 and c0 == c1 == 3  # four steps, one skipped
    for i, (a, b) in enumerate(zip(h0, h1)):
        if i == 2:
            assert not np.isfinite(a[0]) and not np.isfinite(b[0]) and not np.isfinite(a[2]) and not np.isfinite(b[2])
            assert a[3] == b[3] == 1
            continue
        tol = 2e-5 if i == 0 else 2e-4
        assert abs(a[0] - b[0]) <= tol * abs(a[0]) and abs(a[1] - b[1]) <= tol * abs(a[1]), (h0, h1)
        assert np.isfinite(a[2]) and np.isfinite(b[2]) and a[2] > 0 and b[2] > 0, (h0, h1)
        assert a[3] == b[3] == (0 if i < 2 else 1)
    assert torch.isfinite(w0).all() and torch.isfinite(w1).all() and torch.isfinite(e0).all() and torch.isfinite(e1).all()
    assert (w1 - w0).abs().max().item() <= 2 * 1e-4 * 4
    assert (e1 - e0).abs().max().item() <= 2 * 1e-4 * 4


def _rank_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from test_dp_gpu import _share_the_gpu, _slice
    _share_the_gpu(world)
    pipe = _pipe(ALL_ON, n_clips=16)
    assert pipe.reducer.active and pipe.optimizers["optimizerG"].grad_scale == 0.5
    hist = []
    for step in range(2):
        full = _batch(step, n_clips=16, inf_audio=(step == 1))  # the inf sample is the LAST clip: rank 1's half
        losses, _ = pipe.forward_backward(_slice(full, rank * 2, (rank + 1) * 2))
        pipe.optimizer_updates(losses)
        torch.cuda.synchronize()
        hist.append((float(losses["G_loss"].detach()), float(losses["grad_norm_G"]), int(losses["skipped_steps_G"])))
    optg = pipe.optimizers["optimizerG"]
    q.put((rank, hist, optg.flat_param.detach().cpu().numpy(), optg.ema.detach().cpu().numpy(), int(optg.state_dev[0])))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_take_the_same_skip_decision():
    from test_dp_gloo import _collect, _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    (_, h0, w0, e0, s0), (_, h1, w1, e1, s1) = sorted(_collect(procs, q, 2, 500), key=lambda t: t[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    print("  rank 0", h0)
    print("  rank 1", h1)
    assert np.isfinite(h0[1][0]) and not np.isfinite(h1[1][0])  # only rank 1's own loss is non-finite ...
    assert np.isfinite(h0[0][1]) and h0[0][1] == h1[0][1]  # ... the exchanged gradient's norm is the same number on both ranks,
    assert not np.isfinite(h0[1][1]) and not np.isfinite(h1[1][1])  # non-finite on both at step 2,
    assert [h[2] for h in h0] == [h[2] for h in h1] == [0, 1] and s0 == s1 == 1  # both skip it,
    assert np.isfinite(w0).all() and np.array_equal(w0, w1) and np.array_equal(e0, e1)  # and the parameters stay bit-identical
