"""Every validation metric at once: SYS.DEVICE_FGD, TEST.CLIP_METRICS, TEST.FIT_CODE, TEST.SYNC_METRICS and TEST.MOTION_DIST in one
``validate()`` give, key by key, the bits each of them gives alone, in the documented key order.  Each accumulator writes only its own
table and the fit consumes no random number, so the order of the launches within a step must not show in any value.

The test goes through ``validate()``, the config keys and the four accessors only.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _set_keys(cfg, fgd=False, clip=False, fit=False, sync=False, motion=False):
    cfg.defrost()
    cfg.SYS.DEVICE_FGD, cfg.TEST.CLIP_METRICS, cfg.TEST.SYNC_METRICS, cfg.TEST.MOTION_DIST = fgd, clip, sync, motion
    cfg.TEST.FIT_CODE.ENABLE, cfg.TEST.FIT_CODE.STEPS, cfg.TEST.MULTIPLE = fit, 3, 1
    cfg.freeze()


def test_all_keys_on_give_the_bits_of_each_key_alone():
    """FGD_mu / FGD_mu_logvar are held to the run with SYS.DEVICE_FGD alone, like every other group to its own run: the device route and
    the host loop of the all-off run agree to the bar of test_fgd_gpu.py, not bit for bit.  The per-step values of TEST.FIT_CODE are means
    of the loop, so they stand among the losses, before the FGD; they and the _fit clip keys are held to the run with TEST.FIT_CODE and
    TEST.CLIP_METRICS alone."""
    from oracle import sdt_oracle as O
    from test_clip_metrics_gpu import NEW_KEYS as CLIP_KEYS
    from test_code_fit_gpu import FIT_KEYS
    from test_fgd_gpu import _validation_pipeline
    from test_motion_dist_gpu import NEW_KEYS as MOTION_KEYS
    from test_sync_metrics_gpu import NEW_KEYS as SYNC_KEYS
    pipe, cfg = _validation_pipeline()
    losses, _ = pipe.forward_backward(O.make_batch(4, 16, step=0, seed=1))
    pipe.optimizer_updates(losses)

    def run(**keys):
        _set_keys(cfg, **keys)
        torch.manual_seed(5)
        return pipe.validate(pipe.test_dataloader, 1)

    clip_keys = [k for k in CLIP_KEYS if not k.startswith("diversity")]  # (one copy: no diversity)
    fit_clip_keys = [k + "_fit" for k in clip_keys]
    fgd_keys = ["FGD_mu", "FGD_mu_logvar"]
    try:
        off = run()
        assert all(acc() is None for acc in (pipe.device_fgd, pipe.clip_metrics, pipe.sync_metrics, pipe.motion_dist))
        loss_keys = [k for k in off if k not in fgd_keys]
        assert list(off) == loss_keys + fgd_keys
        alone = {"fgd": run(fgd=True), "clip": run(clip=True), "fit": run(clip=True, fit=True), "sync": run(sync=True),
                 "motion": run(motion=True)}
        assert list(alone["fgd"]) == list(off)
        assert list(alone["clip"]) == list(off) + clip_keys
        assert list(alone["fit"]) == loss_keys + FIT_KEYS + fgd_keys + clip_keys + fit_clip_keys
        assert list(alone["sync"]) == list(off) + SYNC_KEYS
        assert list(alone["motion"]) == list(off) + MOTION_KEYS
        accs = [pipe.device_fgd(), pipe.clip_metrics(), pipe.sync_metrics(), pipe.motion_dist()]
        assert all(acc is not None for acc in accs)

        on = run(fgd=True, clip=True, fit=True, sync=True, motion=True)
        assert list(on) == loss_keys + FIT_KEYS + fgd_keys + clip_keys + fit_clip_keys + SYNC_KEYS + MOTION_KEYS
        for group, keys in (("fgd", fgd_keys), ("clip", clip_keys), ("fit", FIT_KEYS + fit_clip_keys), ("sync", SYNC_KEYS),
                            ("motion", MOTION_KEYS)):
            for k in keys:
                print("  %-24s all on %.17g alone %.17g" % (k, float(on[k]), float(alone[group][k])))
                assert float(on[k]) == float(alone[group][k]), k
        for k in loss_keys:  # the all-off run's values keep their bits
            assert torch.equal(torch.as_tensor(on[k]), torch.as_tensor(off[k])), k
        # the accumulators the single runs built took the all-on epoch, each over the 8 clips
        assert all(a is b for a, b in zip([pipe.device_fgd(), pipe.clip_metrics(), pipe.sync_metrics(), pipe.motion_dist()], accs))
        assert accs[0].result(strict=False)["rows_a"] == 8 and accs[1].result()["clips_seen"] == 8
        assert accs[2].result()["sync_clips_seen"] == 8 and accs[3].result()["motion_clips_seen"] == 8
    finally:
        _set_keys(cfg)
