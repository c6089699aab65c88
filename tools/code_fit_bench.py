"""Time the code fit (csrc/code_fit.hip, code_fit.py) by HIP events and around one test_step.  JSON lines, B = 32, T = 64, D = 32:
    iteration   one iteration of the fit as bare launches on persistent tensors -- forward_tail (chain1d forward + head), sdt_code_fit_loss_f32,
                autograd.grad (head input gradient + chain1d backward with need_dx0), sdt_code_fit_step_f32 -- median and minimum of --reps
                windows of 10 iterations, alternating window by window with
    window      the same forward_tail + autograd.grad with a constant output gradient and no kernel of the fit: what the chain, the head and
                autograd cost on their own -- only code that existed before the fit, so the same function runs at the parent commit
                (--parent-window, which times nothing else and imports nothing of the fit) -- and
    kernels     the loss and the step kernel alone (windows of 20 calls); their share of an iteration
    test_step   one Voice2Pose.test_step on a synthetic batch with TEST.FIT_CODE off and on at STEPS = 100 (host clock around the call and a
                device synchronisation), alternating
Appends to profiles/r28_code_fit_bench.jsonl.

    python tools/code_fit_bench.py [--reps 20] [--parent-window] [--out profiles/r28_code_fit_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools._timing import gpu_ms_alternating  # noqa: E402

B, T, D, N_CLIPS = 32, 64, 32, 64


def pipeline():
    from __graft_entry__ import make_pipeline
    from oracle import sdt_oracle as O
    ocfg = O.cfg_named("voice2pose_sdt_bp")
    state = O.make_voice2pose_state(ocfg, N_CLIPS, seed=0, code_std=0.5)
    pipe, cfg = make_pipeline("voice2pose_sdt_bp", N_CLIPS, state=state)
    pipe.model.eval()
    for p in pipe.model.parameters():
        p.requires_grad_(False)
    return pipe, cfg, O.make_batch(B, N_CLIPS, step=0, seed=1)


def tail_of(netG):
    """the generator's Conv1d stage and head on (B, T, 256 + D); at the parent commit the same lines sit inside SequenceGeneratorCNN.forward"""
    if hasattr(netG, "forward_tail"):
        return netG.forward_tail
    from speechdrivestemplates_amd import ops
    from speechdrivestemplates_amd.core.networks.building_blocks import conv_head

    def tail(h):
        spec, weights, slope = netG._chain()
        assert ops.chain1d_usable(h, spec, weights)
        return conv_head(ops.Chain1dFn.apply(h, spec, slope, *weights), netG.decoder[4])
    return tail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-window", action="store_true", help="time only the chain + head window (runs at the parent commit too)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r28_code_fit_bench.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    pipe, cfg, batch = pipeline()
    netG = pipe.model.netG
    tail = tail_of(netG)
    h = torch.randn(B, T, 256 + D, device="cuda").requires_grad_(True)
    gt = batch["poses"].cuda().reshape(B, T, -1).contiguous()
    const_grad = torch.full_like(gt, 1.0 / gt[0].numel())
    recs = []

    def window():
        with torch.enable_grad():
            y = tail(h)
            torch.autograd.grad(y, h, const_grad)

    if a.parent_window:
        (med, lo), = gpu_ms_alternating([window], a.reps, 10)
        recs.append({"bench": "window_only", "B": B, "T": T, "D": D, "window_ms_median": med, "window_ms_min": lo, "has_code_fit": hasattr(netG, "forward_tail")})
    else:
        from speechdrivestemplates_amd import code_fit as cf
        st = cf.FitState(torch.zeros(B, D, device="cuda"), 8, 0.05)
        loss, dpred = torch.empty(B, device="cuda", dtype=torch.float64), torch.empty_like(gt)
        dh = torch.randn(B, T, 256 + D, device="cuda") * 1e-3

        def iteration():
            with torch.enable_grad():
                y = tail(h)
                cf.clip_loss(y.detach(), gt, loss, dpred)
                (g,) = torch.autograd.grad(y, h, dpred)
            st.step(g, loss, h.detach(), 256)

        y0 = tail(h).detach()
        (it, it_lo), (win, win_lo) = gpu_ms_alternating([iteration, window], a.reps, 10)
        (kl, kl_lo), (ks, ks_lo) = gpu_ms_alternating([lambda: cf.clip_loss(y0, gt, loss, dpred), lambda: st.step(dh, loss, h.detach(), 256)], a.reps, 20)
        recs.append({"bench": "iteration", "B": B, "T": T, "D": D, "iteration_ms_median": it, "iteration_ms_min": it_lo, "window_ms_median": win,
                     "window_ms_min": win_lo, "loss_kernel_ms_median": kl, "loss_kernel_ms_min": kl_lo, "step_call_ms_median": ks,
                     "step_call_ms_min": ks_lo, "new_kernels_share_of_iteration": (kl + ks) / it, "iteration_minus_window_ms": it - win})
        for p in pipe.model.parameters():
            p.requires_grad_(True)
        pipe.test_dataset = pipe.train_dataset
        times = {False: [], True: []}
        for rep in range(1 + max(2, a.reps // 5)):
            for on in (False, True):
                cfg.defrost()
                cfg.TEST.FIT_CODE.ENABLE, cfg.TEST.FIT_CODE.STEPS = on, 100
                cfg.freeze()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipe.test_step({k: (dict(v) if isinstance(v, dict) else v) for k, v in batch.items()}, 1, 1)
                torch.cuda.synchronize()
                if rep:  # (the first pair warms up)
                    times[on].append((time.perf_counter() - t0) * 1e3)
        recs.append({"bench": "test_step", "B": B, "T": T, "steps": 100, "off_ms_median": float(np.median(times[False])),
                     "on_ms_median": float(np.median(times[True])), "off_ms_min": float(np.min(times[False])), "on_ms_min": float(np.min(times[True])),
                     "fit_ms_per_iteration": (float(np.median(times[True])) - float(np.median(times[False]))) / 100})
    with open(a.out, "a") as f:
        for r in recs:
            r["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
