"""Validation observers: what a pipeline accumulates on the device next to the per-step losses (DESIGN.md section 22 states the protocol).

An observer has an ``acc`` (the accumulator; None until a step has built it) and four methods.  ``enabled(cfg)`` is asked on every ``validate()``
and every ``test_step`` (``key``: the section and entry of the configuration that switches it on).  ``reset()`` clears the accumulator.
``step(ctx)`` takes what ``test_step`` has in hand: ``ctx.batch``, ``fin_p``, ``fin_g``, ``results``, ``losses``, ``multiple``, ``device``, and
``fit_p`` once ``fit_code_step`` has run.  ``epoch(epoch, tag)`` returns the epoch values and is COLLECTIVE: every rank calls it, in list order."""
import logging
import os

from types import SimpleNamespace

import torch

from ... import clip_metrics, motion_dist, ops, prdc, sync_metrics
from ..datasets.gesture_dataset import PoseTransforms


def gather_states(cfg, state):
    """the ranks' copies of an accumulator's state tensor in rank order (every rank calls it), or None without SYS.DISTRIBUTED"""
    if not cfg.SYS.DISTRIBUTED:
        return None
    gathered = [torch.empty_like(state) for _ in range(torch.distributed.get_world_size())]
    torch.distributed.all_gather(gathered, state)  # (the list form: nccl and gloo both have it)
    return gathered


class _Observer:
    def __init__(self, pipe):
        self.pipe, self.acc = pipe, None

    def enabled(self, cfg):
        return bool(getattr(cfg[self.key[0]], self.key[1], False))

    def reset(self):
        if self.acc is not None:
            self.acc.reset()


class DeviceFGD(_Observer):
    """SYS.DEVICE_FGD with a pose encoder: the mu ++ logvar rows go into moment states on the device (fgd.FGDAccumulator)"""
    key = ('SYS', 'DEVICE_FGD')

    def enabled(self, cfg):
        return _Observer.enabled(self, cfg) and cfg.VOICE2POSE.POSE_ENCODER.NAME is not None

    def step(self, ctx):
        r = ctx.results
        ops.join_side_stream()
        if self.acc is None:  # (the first step knows the code width and the device)
            from ...fgd import FGDAccumulator
            self.acc = FGDAccumulator(2 * r['mu_pred'].shape[1], r['mu_pred'].device)
        self.acc.add(r['mu_pred'], r['mu_gt'], r['logvar_pred'], r['logvar_gt'])

    def epoch(self, epoch, tag):
        """FGD_mu (the leading block of the moments) and FGD_mu_logvar over the rows every rank delivered, merged in rank order: the same value
        on every rank.  A non-finite feature is a warning and a NaN metric, not the end of a training run."""
        from ...fgd import describe_error
        if self.acc is None:  # no validation step ran
            return {}
        gathered = gather_states(self.pipe.cfg, self.acc.states())
        out = {}
        for key, dim_used in (('FGD_mu', self.acc.dim // 2), ('FGD_mu_logvar', self.acc.dim)):
            res = self.acc.result(dim_used=dim_used, gathered=gathered, strict=False)
            if res['err']:
                logging.warning('[VAL] %s: %s' % (key, describe_error(res)))
            out[key] = res['fgd']
        return out


class ClipTable(_Observer):
    """What the record-table metrics share: one row per clip of the validation set, addressed by the batch's 'clip_index', built by the first
    step (which knows the keypoint count and the device).  A family names its ``module``, the ``label`` of its warning and file, the ``prefix``
    of its bookkeeping entries and the ``suffix`` of its keys, and has ``enabled``, ``step`` and ``save_args`` (for ``module.save_table``)."""
    prefix = suffix = ''

    def num_clips(self):
        ds = self.pipe.test_dataset
        return len(getattr(ds, 'dataset', ds))  # (a Subset keeps the indices of the set it was cut from)

    def epoch(self, epoch, tag):
        """the values over the clips every rank delivered: clip by clip the lowest rank that has a record gives it, so every rank reports the
        same bits.  A clip with a non-finite sum or an index outside the table is left out, counted and warned about."""
        acc, pipe, module, prefix = self.acc, self.pipe, self.module, self.prefix
        if acc is None:  # no validation step ran
            return {}
        gathered = gather_states(pipe.cfg, acc.state())
        res = acc.result(gathered)
        if res[prefix + 'clips_nonfinite'] or res[prefix + 'index_errors']:
            logging.warning('[VAL] %s metrics: %d clip(s) left out for a non-finite sum, %d clip index(es) outside the table of %d'
                            % (self.label, res[prefix + 'clips_nonfinite'], res[prefix + 'index_errors'], acc.num_clips))
        if pipe.is_master_process() and pipe.cfg.TEST.SAVE_NPZ and pipe.base_path is not None:
            d = os.path.join(pipe.base_path, 'results')
            os.makedirs(d, exist_ok=True)
            tables = [acc.table()] if gathered is None else [g[:acc.num_clips] for g in gathered]
            module.save_table('%s/epoch%d-%s-%s_metrics.npz' % (d, epoch, tag, self.label), module.merge_tables([t.cpu().numpy() for t in tables]),
                              *self.save_args())
        out = {k + self.suffix: v for k, v in res.items() if k not in module.BOOKKEEPING}
        out.update(self.intervals(res, gathered, epoch, tag))
        return out

    def intervals(self, res, gathered, epoch, tag):
        """what a family adds from the gathered states it already has, after its own keys (nothing, unless it says otherwise)"""
        return {}


class FeatureSets(ClipTable):
    """TEST.PRDC: precision / recall / density / coverage between the set of generated and the set of real pose-encoder features (prdc.py)"""
    key = ('TEST', 'PRDC')

    def enabled(self, cfg):
        return bool(cfg.TEST.PRDC.ENABLE)

    def step(self, ctx):
        r = ctx.results
        ops.join_side_stream()  # (the features come from the side stream, as in DeviceFGD.step)
        if self.acc is None or self.acc.copies != ctx.multiple:  # (a record is laid out for its number of copies)
            from ...config import check_prdc
            self.acc = prdc.FeatureSetAccumulator(self.num_clips(), 2 * r['mu_pred'].shape[1], ctx.multiple,
                                                  check_prdc(self.pipe.cfg)['k'], r['mu_pred'].device)
        self.acc.add(r['mu_pred'], r['logvar_pred'], r['mu_gt'], r['logvar_gt'], ctx.batch['clip_index'])

    def epoch(self, epoch, tag):
        """the sixteen values over the clips every rank delivered (the mu columns, then all columns; each with its floor) and
        prdc_clips_nonfinite: the same bits on every rank.  Too few clips for K is a warning and NaN values, not the end of a training run."""
        acc, pipe = self.acc, self.pipe
        if acc is None:  # no validation step ran
            return {}
        gathered = gather_states(pipe.cfg, acc.state())
        out, res = {}, None
        for sfx, dim_used in (('_mu', acc.dim // 2), ('_mu_logvar', acc.dim)):
            res = acc.result(dim_used=dim_used, gathered=gathered)
            out.update({v + sfx + floor: res[v + floor] for floor in ('', '_floor') for v in prdc.VALUES})
        if res['clips_nonfinite'] or res['index_errors']:
            logging.warning('[VAL] feature-set metrics: %d clip(s) left out for a non-finite feature, %d clip index(es) outside the table of %d'
                            % (res['clips_nonfinite'], res['index_errors'], acc.num_clips))
        if pipe.is_master_process() and pipe.cfg.TEST.SAVE_NPZ and pipe.base_path is not None:  # (the rows of the last result: all columns)
            d = os.path.join(pipe.base_path, 'results')
            os.makedirs(d, exist_ok=True)
            prdc.save_rows('%s/epoch%d-%s-prdc.npz' % (d, epoch, tag), acc.rows(), res, acc.k)
        out['prdc_clips_nonfinite'] = res['clips_nonfinite']
        return out


class ClipMetrics(ClipTable):
    """TEST.CLIP_METRICS: PCK, part errors, speed ratio, velocity error and diversity (clip_metrics.py)"""
    key, label, module = ('TEST', 'CLIP_METRICS'), 'clip', clip_metrics

    def step(self, ctx):
        if self.acc is None:
            from ...config import check_clip_metrics
            self.acc = clip_metrics.ClipMetricsAccumulator(self.num_clips(), ctx.fin_p.shape[3], check_clip_metrics(self.pipe.cfg),
                                                          ctx.fin_p.device, parts=PoseTransforms.part_table())
        self.acc.add(ctx.fin_p, ctx.fin_g, ctx.batch['clip_index'], ctx.multiple)

    def save_args(self):
        return (self.acc.alphas,)

    def reset(self):
        ClipTable.reset(self)
        self.resampled = None  # after an epoch with TEST.BOOTSTRAP: (the gathered states,), for the paired run of FitClipMetrics

    def intervals(self, res, gathered, epoch, tag):
        """TEST.BOOTSTRAP: <key>_lo / <key>_hi for every metric key of ``res``, from the states the epoch has gathered (bootstrap.py)"""
        from ...config import check_bootstrap
        opts, pipe = check_bootstrap(self.pipe.cfg), self.pipe
        if opts is None:
            return {}
        from ... import bootstrap
        self.resampled = (gathered,)
        run = dict(replicates=opts['replicates'], level=opts['level'], seed=opts['seed'])
        stages = {}
        ci = bootstrap.clip_metric_intervals(self.acc, gathered=gathered, stages=stages, **run)
        if not ci:
            logging.warning('[VAL] %s metrics: no live clip, no bootstrap intervals' % self.label)
            return {}
        if pipe.is_master_process() and pipe.cfg.TEST.SAVE_NPZ and pipe.base_path is not None:
            bootstrap.save_replicates('%s/results/epoch%d-%s-%s_bootstrap.npz' % (pipe.base_path, epoch, tag, self.label), stages,
                                      self.acc.alphas, clip_metrics.part_sizes(self.acc.parts), **run)
        out = {}
        for k in res:
            if k in ci:
                out[k + self.suffix + '_lo'], out[k + self.suffix + '_hi'] = ci[k][1], ci[k][2]
        return out


class FitClipMetrics(ClipMetrics):
    """with TEST.FIT_CODE: a second table for the fitted predictions ``fit_code_step`` left in ``ctx.fit_p``, one copy per clip; keys end in _fit"""
    label, suffix = 'clip_fit', '_fit'

    def enabled(self, cfg):
        return ClipMetrics.enabled(self, cfg) and bool(cfg.TEST.FIT_CODE.ENABLE)

    def step(self, ctx):
        ClipMetrics.step(self, SimpleNamespace(batch=ctx.batch, fin_p=ctx.fit_p, fin_g=ctx.fin_g, multiple=1))

    def intervals(self, res, gathered, epoch, tag):
        """the _fit keys' own intervals, then one paired run of the fitted against the plain prediction over the clips live in both tables:
        <key>_fit_gain_lo / _hi, the interval of fitted minus plain"""
        out = ClipMetrics.intervals(self, res, gathered, epoch, tag)
        plain = getattr(self.pipe, 'clip_observer', None)
        if not out or plain is None or plain.acc is None or getattr(plain, 'resampled', None) is None:
            return out
        from ... import bootstrap
        from ...config import check_bootstrap
        opts = check_bootstrap(self.pipe.cfg)
        gain = bootstrap.clip_metric_paired(self.acc, plain.acc, replicates=opts['replicates'], level=opts['level'], seed=opts['seed'],
                                            gathered_a=gathered, gathered_b=plain.resampled[0])
        for k in bootstrap.GAIN_KEYS:
            if k in gain:
                out[k + '_fit_gain_lo'], out[k + '_fit_gain_hi'] = gain[k]['diff_lo'], gain[k]['diff_hi']
        return out


class SyncMetrics(ClipTable):
    """TEST.SYNC_METRICS: audio onsets against the beats of both pose tensors (sync_metrics.py)"""
    key, label, prefix, module = ('TEST', 'SYNC_METRICS'), 'sync', 'sync_', sync_metrics

    def step(self, ctx):
        if self.acc is None:
            from ...config import check_sync_metrics
            opts = check_sync_metrics(self.pipe.cfg)
            self.acc = sync_metrics.SyncAccumulator(self.num_clips(), ctx.fin_p.shape[3], opts['tol_ticks'], opts['sigma'], ctx.fin_p.device,
                                                   parts=PoseTransforms.part_table())
        self.acc.add(ctx.fin_p, ctx.fin_g, ctx.batch['audio'].to(ctx.device, non_blocking=True).float(), ctx.batch['clip_index'], ctx.multiple)

    def save_args(self):
        return self.acc.tol, self.acc.sigma


class MotionDist(ClipTable):
    """TEST.MOTION_DIST: speed / acceleration / jerk histograms (motion_dist.py); with SYS.TENSORBOARD the master also writes the merged ones"""
    key, label, prefix, module = ('TEST', 'MOTION_DIST'), 'motion', 'motion_', motion_dist

    def step(self, ctx):
        if self.acc is None:
            from ...config import check_motion_dist
            self.acc = motion_dist.MotionDistAccumulator(self.num_clips(), ctx.fin_p.shape[3], check_motion_dist(self.pipe.cfg)['edges'],
                                                         ctx.fin_p.device, parts=PoseTransforms.part_table())
        self.acc.add(ctx.fin_p, ctx.fin_g, ctx.batch['clip_index'], ctx.multiple)

    def save_args(self):
        return self.acc.edges, self.acc.histograms()

    def epoch(self, epoch, tag):
        out = ClipTable.epoch(self, epoch, tag)
        tb, md = getattr(self.pipe, 'tb_writer', None), motion_dist
        if self.acc is not None and tb is not None and self.pipe.is_master_process():
            hist = self.acc.histograms()  # (the merged histograms of the result() above)
            for s, source in enumerate(md.SOURCES):
                for o, order in enumerate(md.ORDERS):
                    for p, part in enumerate(md.PARTS):
                        tb.add_histogram_raw('%s/motion/%s_%s_%s' % (tag.lower(), order, source, part),
                                             *md.tb_histogram_fields(hist[s, o, p], self.acc.edges[o]), step=epoch)
            tb.flush()
        return out
