"""Training-loop shell around ``train_step`` (core/pipelines/trainer.py): rank helpers (:29-45), dataset /
dataloader setup (:64-145), experiment setup with resume / pretrain (:162-224), step logging (:242-263),
checkpoint wire format (:305-321), epoch loop (:367-405) and validation (:407-427).  Scalars go to the Python logger and, with
SYS.TENSORBOARD, to a TensorBoard event file under the reference's tags (tb_events.py; :242-303).  Pose videos and long images are drawn on
the GPU (render.py) and written by video.VideoWriter when SYS.RENDER_VIDEO is set (opt-in; default: npz only).  The per-epoch
clip-code figure (:404-405, 281-283) is drawn on the GPU (code_pca.py) and written as a PNG when SYS.EPOCH_FIGURES is set."""
import contextlib
import logging
import os
import time
from datetime import datetime

import numpy as np
import torch
from torch.utils.data import DataLoader

from ..datasets import get_dataset
from ..datasets.gesture_dataset import register_configured_speaker_stats


def _collate_stat(samples):
    """default_collate of the nested speaker_stat dict gives float64 (B,242)/(B,) tensors (gesture_dataset.py:107-119)."""
    return torch.utils.data.default_collate(samples)


class Trainer(object):
    def __init__(self, cfg) -> None:
        self.cfg = cfg
        self.model = None
        self.optimizers = {}
        self.schedulers = {}
        self.train_dataloader = None
        self.test_dataloader = None
        self.train_dataset = None
        self.test_dataset = None
        self.num_train_samples = None
        self.result_saving_interval_train = 1 << 60
        self.result_saving_interval_test = 1 << 60
        self.base_path = None
        self.step_tic = time.time()
        if not torch.cuda.is_available():
            raise RuntimeError('this engine needs an AMD GPU (no CPU fallback); torch.cuda.is_available() is False')
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', self.get_rank() % max(1, torch.cuda.device_count()))))
        from ...config import (check_audio_strip, check_augment, check_bootstrap, check_clip_metrics, check_fit_code, check_histograms,
                               check_long_demo, check_motion_dist, check_prdc, check_sync_metrics)
        check_histograms(cfg)  # SYS.HISTOGRAM_INTERVAL without SYS.TENSORBOARD: there is nowhere to write
        check_clip_metrics(cfg)  # TEST.CLIP_METRICS / TEST.PCK_ALPHAS (a Voice2Pose key)
        check_sync_metrics(cfg)  # TEST.SYNC_METRICS / SYNC_TOLERANCE / SYNC_SIGMA (a Voice2Pose key)
        check_motion_dist(cfg)  # TEST.MOTION_DIST / MOTION_DIST_EDGES (a Voice2Pose key)
        check_fit_code(cfg)  # TEST.FIT_CODE: oracle-code validation (a Voice2Pose key)
        check_prdc(cfg)  # TEST.PRDC: precision / recall / density / coverage of the generated feature set (a Voice2Pose key)
        check_bootstrap(cfg)  # TEST.BOOTSTRAP: percentile intervals of the clip metrics (needs TEST.CLIP_METRICS)
        check_long_demo(cfg)  # DEMO.LONG_FORM and its window / smoothing / segment keys (a Voice2Pose key)
        check_augment(cfg)  # TRAIN.AUGMENT: audio augmentation inside the train step (a Voice2Pose key)
        self.strip_opts = check_audio_strip(cfg)  # SYS.AUDIO_STRIP: the audio band under the rendered pictures (None = off)

    # -- process-group helpers (trainer.py:29-45) ---------------------------------------------------------
    def get_rank(self):
        return torch.distributed.get_rank() if torch.distributed.is_initialized() else 0

    def get_world_size(self):
        return torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1

    def is_master_process(self):
        return self.get_rank() == 0

    # -- data ------------------------------------------------------------------------------------------
    def setup_dataset(self, cfg, split, demo_input=None):
        ws = self.get_world_size()
        register_configured_speaker_stats(cfg)  # DATASET.SPEAKER_STAT_FILE, before any dataset looks its speaker up
        ds_cls = get_dataset(cfg.DATASET.NAME)
        if split == 'train':
            self.train_dataset = ds_cls(cfg.DATASET.ROOT_DIR if cfg.DATASET.NAME == 'GestureDataset' else None,
                                        cfg.DATASET.SPEAKER, 'train', cfg)
            sampler = torch.utils.data.distributed.DistributedSampler(self.train_dataset) if cfg.SYS.DISTRIBUTED else None
            self.train_sampler = sampler
            self.train_dataloader = DataLoader(self.train_dataset, batch_size=cfg.TRAIN.BATCH_SIZE // ws, shuffle=sampler is None,
                                               num_workers=cfg.SYS.NUM_WORKERS // ws, sampler=sampler, drop_last=True)
            self.num_train_samples = len(self.train_dataset)
            self.num_train_batches = len(self.train_dataloader)
            self.result_saving_interval_train = max(1, self.num_train_batches // cfg.TRAIN.NUM_RESULT_SAMPLE)
            if cfg.TRAIN.VALIDATE:
                self._setup_eval(cfg, ds_cls, 'val', ws)
        elif split == 'test':
            self.num_train_samples = None
            self._setup_eval(cfg, ds_cls, 'val', ws)
        elif split == 'demo':  # one clip per step, variable length (trainer.py:124-132)
            self.num_train_samples = None
            self.test_dataset = get_dataset('GestureDataset')(cfg.DATASET.ROOT_DIR, cfg.DATASET.SPEAKER, 'demo', cfg, demo_input=demo_input)
            self.test_dataloader = DataLoader(self.test_dataset, batch_size=1, shuffle=False, num_workers=0)
            self.num_test_samples = len(self.test_dataset)
            self.num_test_batches = len(self.test_dataloader)
        else:
            raise Exception('Unknown data split.')

    def _setup_eval(self, cfg, ds_cls, split, ws):
        self.test_dataset = ds_cls(cfg.DATASET.ROOT_DIR if cfg.DATASET.NAME == 'GestureDataset' else None,
                                   cfg.DATASET.SPEAKER, split, cfg)
        sampler = torch.utils.data.distributed.DistributedSampler(self.test_dataset, shuffle=False) if cfg.SYS.DISTRIBUTED else None
        self.test_dataloader = DataLoader(self.test_dataset, batch_size=cfg.TEST.BATCH_SIZE // ws, shuffle=False,
                                          num_workers=cfg.SYS.NUM_WORKERS // ws, sampler=sampler)
        self.num_test_samples = len(self.test_dataset)
        self.num_test_batches = len(self.test_dataloader)
        self.result_saving_interval_test = max(1, self.num_test_batches // cfg.TEST.NUM_RESULT_SAMPLE)  # trainer.py:96-97

    def mutiply_batch(self, batch, multiple):
        """TEST.MULTIPLE copies of every sample, batch-major (trainer.py:343-353; name as in the reference)."""
        if isinstance(batch, dict):
            for k, v in batch.items():
                batch[k] = self.mutiply_batch(v, multiple)
            return batch
        if isinstance(batch, list):
            return batch * multiple
        if isinstance(batch, torch.Tensor):
            return batch.unsqueeze(0).repeat_interleave(multiple, dim=0).reshape(multiple * batch.shape[0], *batch.shape[1:])
        raise NotImplementedError

    def setup_model(self, cfg, state_dict=None):
        raise NotImplementedError

    def setup_optimizer(self, checkpoint=None, last_epoch=-1):
        raise NotImplementedError

    # -- experiment / checkpoints (trainer.py:162-224, 305-321) ------------------------------------------
    def setup_experiment(self, is_training, exp_tag, resume_from=None, checkpoint=None, demo_input=None):
        dt = str(datetime.now()).replace('.', '-').replace(':', '-').replace(' ', '_')
        exp_tag = '_'.join([dt, exp_tag])
        if not is_training:
            self.setup_dataset(self.cfg, 'test' if demo_input is None else 'demo', demo_input=demo_input)
            base_path = os.path.join(self.cfg.SYS.OUTPUT_DIR, exp_tag)
            if self.is_master_process():
                os.makedirs(base_path, exist_ok=True)
            if checkpoint is None:
                raise Exception('Checkpoint file is not provided.')
            assert checkpoint.split('.')[-1] == 'pth', 'file type not supported: %s' % checkpoint
            ckpt = torch.load(checkpoint, map_location='cpu')
            key = 'model_state_dict'
            if getattr(self.cfg.SYS, 'EVAL_WITH_EMA', False):  # test() / demo() build no optimiser: the EMA weights are loaded directly
                if 'model_ema_state_dict' not in ckpt:
                    raise ValueError("SYS.EVAL_WITH_EMA: the checkpoint %s carries no 'model_ema_state_dict' (it was not written by a "
                                     "run with TRAIN.EMA_DECAY)" % checkpoint)
                key = 'model_ema_state_dict'
            self.setup_model(self.cfg, state_dict=ckpt[key])
            self._model_holds_ema = key == 'model_ema_state_dict'
            return base_path
        self.setup_dataset(self.cfg, 'train')
        if resume_from is not None:
            assert resume_from.split('.')[-1] == 'pth', 'file type not supported: %s' % resume_from
            assert os.path.exists(resume_from), 'file not exists: %s' % resume_from
            ckpt = torch.load(resume_from, map_location='cpu')
            epoch, global_step = ckpt['epoch'], ckpt['step']
            base_path = os.path.split(resume_from)[0]
            self.setup_model(self.cfg, state_dict=ckpt['model_state_dict'])
            self.setup_optimizer(checkpoint=ckpt, last_epoch=epoch)
            return base_path, epoch, global_step
        base_path = os.path.join(self.cfg.SYS.OUTPUT_DIR, exp_tag)
        if self.is_master_process():
            os.makedirs(base_path, exist_ok=True)
        if self.cfg.TRAIN.PRETRAIN_FROM is not None:
            ckpt = torch.load(self.cfg.TRAIN.PRETRAIN_FROM, map_location='cpu')
            self.setup_model(self.cfg, state_dict=ckpt['model_state_dict'])
        else:
            self.setup_model(self.cfg)
        self.setup_optimizer()
        return base_path, 0, 0

    def checkpoint_dict(self, epoch, global_step):
        """{'epoch','step','model_state_dict' (keys prefixed 'module.'), '<optimizer>_state_dict'...} (trainer.py:313-319)."""
        ckpt = {'epoch': epoch, 'step': global_step,
                'model_state_dict': {'module.' + k: v.detach().clone().contiguous() for k, v in self.model.state_dict().items()}}
        for k, v in self.optimizers.items():
            ckpt['%s_state_dict' % k] = v.state_dict()
        ema = self.ema_model_state()
        if ema is not None:
            ckpt['model_ema_state_dict'] = ema
        return ckpt

    # -- optimiser-side safeguards (TRAIN.GRAD_CLIP_NORM / SKIP_NONFINITE_STEP / EMA_DECAY, SYS.EVAL_WITH_EMA) ------
    def setup_step_guards(self, groups, ema_names, checkpoint=None):
        """``groups``: {'G': [optimiser names stepped together], 'D': [...]} -> one optim.StepGuard per group when clipping or the
        non-finite skip is configured (self.step_guards, else empty: the step calls what it always called); ``ema_names``: the
        optimisers whose parameters get an EMA with TRAIN.EMA_DECAY, restored from ``checkpoint['model_ema_state_dict']`` on resume
        (a checkpoint without it: the EMA starts from the loaded weights).  Call after the replicas are synchronised."""
        from ...config import check_optim_guard
        from ...optim import StepGuard
        cfg = self.cfg
        check_optim_guard(cfg, checkpoint is not None and 'model_ema_state_dict' in checkpoint)
        self.step_guards = {}
        clip, skip = cfg.TRAIN.GRAD_CLIP_NORM, bool(cfg.TRAIN.SKIP_NONFINITE_STEP)
        if clip is not None or skip:
            for tag, names in groups.items():
                opts = [self.optimizers[n] for n in names if n in self.optimizers]
                if opts:
                    self.step_guards[tag] = StepGuard(opts, max_norm=clip, skip_nonfinite=skip)
        if cfg.TRAIN.EMA_DECAY is not None:
            for n in ema_names:
                if n in self.optimizers:
                    self.optimizers[n].enable_ema(cfg.TRAIN.EMA_DECAY)
            if checkpoint is not None and 'model_ema_state_dict' in checkpoint:
                self.load_ema_model_state(checkpoint['model_ema_state_dict'])

    def guarded_steps(self, tag, opts, losses):
        """guard (norm -> record) -> steps of one step group, after its gradient exchange; the device scalars join the loss dict"""
        guard = getattr(self, 'step_guards', {}).get(tag)
        if guard is not None:
            guard.prepare()
            losses['grad_norm_' + tag], losses['skipped_steps_' + tag] = guard.norm(), guard.skipped()
        for opt in opts:
            opt.step()

    def _owned_params(self, ema_only=False):
        """[(state_dict key, optimiser, index)] of every parameter an optimiser owns (``ema_only``: that has an EMA)"""
        owner = {id(p): (opt, i) for opt in self.optimizers.values() if opt.ema is not None or not ema_only
                 for i, p in enumerate(opt.params)}
        return [(name,) + owner[id(p)] for name, p in self.model.named_parameters() if id(p) in owner]

    def _ema_params(self):
        """[(state_dict key, optimiser, index)] of every parameter that has an EMA"""
        return self._owned_params(ema_only=True)

    def ema_model_state(self):
        """``model_state_dict`` with the averaged parameters replaced by their EMA (same keys; None: no optimiser keeps an EMA)"""
        ema = self._ema_params()
        if not ema:
            return None
        out = {'module.' + k: v.detach().clone().contiguous() for k, v in self.model.state_dict().items()}
        for name, opt, i in ema:
            out['module.' + name] = opt._per_param(opt.ema, i).detach().clone().contiguous()
        return out

    def load_ema_model_state(self, sd):
        sd = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in sd.items()}
        with torch.no_grad():
            for name, opt, i in self._ema_params():
                if name in sd:
                    opt._per_param(opt.ema, i).copy_(sd[name])

    @contextlib.contextmanager
    def eval_weights(self):
        """SYS.EVAL_WITH_EMA: the EMA weights are in the parameter buffers inside the block and the training weights are back, bit
        for bit, after it -- also when the block raises.  Without the key: nothing happens."""
        if not getattr(self.cfg.SYS, 'EVAL_WITH_EMA', False) or getattr(self, '_model_holds_ema', False):
            yield
            return
        opts = [opt for opt in self.optimizers.values() if opt.ema is not None]
        if not opts:
            raise ValueError('SYS.EVAL_WITH_EMA needs an EMA to evaluate: set TRAIN.EMA_DECAY (or test / demo from a checkpoint that '
                             "carries 'model_ema_state_dict')")
        for opt in opts:
            opt.swap_ema()  # (marks the weight mirrors dirty)
        try:
            yield
        finally:
            for opt in opts:
                opt.swap_ema()

    @staticmethod
    def check_kernels():
        """Raise if a persistent stream-K convolution launch reported a lost partner since the last check (its tile was stored as NaN).
        Called on log steps, after validation and before every checkpoint: a run never logs, validates or saves numbers that such
        a launch produced (VERDICT r3 / ADVICE r3: the error word used to be read by tests and bench.py only)."""
        from ... import ops
        ops.check_streamk()

    def check_kernels_all_ranks(self, flagged=None):
        """``check_kernels`` for data-parallel runs: every rank learns whether ANY rank's persistent launch lost a partner and all of them raise
        together -- before rank 0 logs NaN losses or writes a checkpoint of weights that the summing all-reduce has already poisoned on every
        rank (rank 0's own word is clean when the launch failed on rank 3).  COLLECTIVE: every rank must call it at the same
        point (log steps via dp.reduce_scalars' piggy-backed flag -> ``flagged``; before a checkpoint; after validation)."""
        from ... import dp, ops
        if flagged is None:
            if not (self.cfg.SYS.DISTRIBUTED and dp.world_size() > 1):
                return self.check_kernels()
            flagged = dp.any_rank_flag(ops.kernel_error_flag())
        if flagged:
            self.check_kernels()  # the rank(s) that own the error word raise with its decoded contents
            raise RuntimeError("a persistent launch on %d other rank(s) gave up waiting for a partner workgroup: the gradients exchanged since the "
                               "last check are invalid on every rank (see that rank's message)" % int(flagged))

    def close(self):
        """Give back what this pipeline holds process-wide (the data-parallel reducer's workgroup-slot reserve, dp.GradReducer.close)
        and drain the asynchronous video writer."""
        r = getattr(self, 'reducer', None)
        if r is not None:
            r.close()
        vw = getattr(self, 'video_writer', None)
        if vw is not None:
            vw.close()
            self.video_writer = None
        tb = getattr(self, 'tb_writer', None)
        if tb is not None:  # (after the video writer: its worker may still add a GIF)
            tb.close()
            self.tb_writer = None

    # -- videos (trainer.py:374,437,467; voice2pose.py:318-331,372-378,404-410,448-459) -----------------------------------
    def rendering(self):
        """SYS.RENDER_VIDEO: TRAIN/TEST.SAVE_VIDEO and the demo write videos / long images (drawn on the GPU; the writer encodes them on the
        GPU too with SYS.DEVICE_JPEG or the 'avi' token of SYS.VIDEO_FORMAT, video.py)"""
        return bool(getattr(self.cfg.SYS, 'RENDER_VIDEO', False))

    def setup_video_writer(self):
        if self.rendering() and self.is_master_process() and getattr(self, 'video_writer', None) is None:
            from ...video import VideoWriter
            self.video_writer = VideoWriter(self.cfg)
        return getattr(self, 'video_writer', None)

    def setup_tb_writer(self):
        """SYS.TENSORBOARD, master process: one event file in the run's directory (trainer.py:373,436,466)"""
        if getattr(self.cfg.SYS, 'TENSORBOARD', False) and self.is_master_process() and getattr(self, 'tb_writer', None) is None \
                and self.base_path is not None:
            from ...tb_events import EventWriter
            self.tb_writer = EventWriter(self.base_path)
        return getattr(self, 'tb_writer', None)

    def generate_video_pair(self, relative_poses_pred, relative_poses_gt):
        from ... import render
        return render.render_pose_pair_clip(relative_poses_pred, relative_poses_gt, tuple(self.cfg.SYS.CANVAS_SIZE),
                                            self.cfg.SYS.VISUALIZATION_SCALING)

    def generate_video(self, relative_poses):
        from ... import render
        return render.render_pose_clip(relative_poses, tuple(self.cfg.SYS.CANVAS_SIZE), self.cfg.SYS.VISUALIZATION_SCALING)

    def write_pair_video(self, tag, pred, gt, t_step, epoch, global_step=None, audio=None):
        """clip 0's prediction beside its ground truth, with clip 0's audio (final poses, (T, 2, K))"""
        vid_batch = self.generate_video_pair(pred, gt)
        if self.strip_opts is not None and audio is not None:  # SYS.AUDIO_STRIP
            vid_batch, _ = self.add_audio_strip(vid_batch, None, audio[0], pred, gt)
        self.setup_video_writer().save_video(self.cfg, tag, vid_batch, t_step, epoch, global_step,
                                             audio=None if audio is None else audio[0], writer=getattr(self, 'tb_writer', None),
                                             base_path=self.base_path)

    def write_demo_video(self, pred, t_step, epoch, audio=None, extra_id=None):
        from ... import render
        vid_batch = self.generate_video(pred)
        long_img = render.render_long_image(pred)
        if self.strip_opts is not None and audio is not None:  # SYS.AUDIO_STRIP
            vid_batch, long_img = self.add_audio_strip(vid_batch, long_img, audio[0], pred, None)
        self.setup_video_writer().save_video(self.cfg, 'DEMO', vid_batch, t_step, epoch, long_img=long_img,
                                             audio=None if audio is None else audio[0], base_path=self.base_path, extra_id=extra_id)

    def add_audio_strip(self, frames, long_img, audio, pred, gt):
        """SYS.AUDIO_STRIP: the band of one clip's audio under its frames and (demo) its long image (audio_strip.py).
        ``audio`` (L,) as the loader delivered it: the mel is the model's own front end on that clean audio; with MARKS the onsets and the
        beats of part 'all' come from sync_metrics, unchanged.  -> (frames, long image or None)"""
        from ... import audio_strip
        o = self.strip_opts
        x = audio.detach().to(device=frames.device, dtype=torch.float32).contiguous()
        mel = self.model.mel_transfm(x[None])[0]
        marks = audio_strip.clip_marks(x, pred, gt) if o['marks'] else None
        out = audio_strip.strip_for_clip(frames, x, mel, marks, o['height'], o['span_s'], o['db_range'])
        if long_img is not None:
            long_img = audio_strip.strip_for_long_image(long_img, x, mel, int(pred.shape[0]), marks, o['height'], o['db_range'])
        return out, long_img

    # -- epoch figures (trainer.py:227-231,404-405; voice2pose.py:479-510; pose2pose.py:314-345) --------------------------------
    def draw_figure_epoch(self):
        """{name: (H, W, 3) uint8 RGB device image} drawn at the end of an epoch; a pipeline that draws also leaves
        ``self.figure_meta[name]`` (the numbers a figure with axes would show).  The base pipeline draws nothing (trainer.py:227-231)."""
        return {}

    def _clip_code_figure(self, codes):
        from ... import code_pca
        image, meta = code_pca.clip_code_figure(codes.detach(), return_meta=True)
        self.figure_meta = {'clip_code': meta}
        return {'clip_code': image}

    def write_epoch_figures(self, epoch):
        """SYS.EPOCH_FIGURES, master process, end of an epoch: <base>/figures/epoch<E>-<name>.png and one log line (the reference hands
        the figures to TensorBoard, trainer.py:281-283).  Eager launches on the current stream, between steps; no collective."""
        from ... import code_pca
        try:
            figures = self.draw_figure_epoch()
        except ValueError as e:  # the TABLE cannot be drawn (a non-finite entry, all rows equal): say so and go on training
            logging.error('[TRAIN] epoch plotting: no figure for epoch %d: %s' % (epoch, e))
            return
        msg = '[TRAIN] epoch plotting: '
        tb = getattr(self, 'tb_writer', None)
        for name, image in figures.items():
            meta = getattr(self, 'figure_meta', {}).get(name)
            path = code_pca.save_png(os.path.join(self.base_path, 'figures', 'epoch%d-%s.png' % (epoch, name)), image, meta)
            if tb is not None:  # (trainer.py:281-283: add_figure stores a PNG image summary)
                with open(path, 'rb') as f:
                    tb.add_image_bytes('train/%s' % name, f.read(), int(image.shape[0]), int(image.shape[1]), epoch)
            msg += '%s, %s  ' % (name.replace('_', ' ').title(), code_pca.describe(meta) if meta else '')
        logging.info(msg)

    def _set_reducer(self, reducer):
        self.close()  # a second setup_optimizer on this pipeline: the old reducer's reserve goes back first
        self.reducer = reducer

    def apply_knobs(self):
        """storage / chain mode of THIS pipeline's configuration become the process-wide kernel routing for the step that follows"""
        from ... import ops
        ops.apply_knobs(getattr(self, 'knobs', None))

    def graphed_or_eager_step(self, batch, eager_ok=True, want_final=False):
        """forward + backward + gradient exchange + optimiser updates of one train step: replayed from a hipGraph when SYS.HIP_GRAPH is set (single
        GPU and data-parallel alike, graph.GraphedStep), enqueued launch by launch otherwise.  Returns (losses, results)."""
        if getattr(self.cfg.SYS, 'HIP_GRAPH', False) and eager_ok:
            if getattr(self, '_graphed', None) is None:
                from ...graph import GraphedStep
                self._graphed = GraphedStep(self, warmup=2)
            losses = self._graphed.run(batch)
            return losses, self._graphed.results
        losses, results = self.forward_backward(batch, want_final=want_final)
        self.optimizer_updates(losses)
        return losses, results

    def save_checkpoint(self, epoch, global_step):
        self.check_kernels()
        d = os.path.join(self.base_path, 'checkpoints')
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, 'checkpoint_epoch-%d_step-%d.pth' % (epoch, global_step))
        logging.info('Saving checkpoint to: %s' % path)
        torch.save(self.checkpoint_dict(epoch, global_step), path)
        return path

    def save_results(self, tag, step, epoch, base_path, results_dict, extra_id=None):
        """<base>/results/epoch<E>-<TAG>-step<S>[-<extra>].npz, the reference's naming (voice2pose.py:461-477)."""
        d = os.path.join(base_path, 'results')
        os.makedirs(d, exist_ok=True)
        path = '%s/epoch%d-%s-step%s.npz' % (d, epoch, tag, step) if extra_id is None \
            else '%s/epoch%d-%s-step%s-%d.npz' % (d, epoch, tag, step, extra_id)
        if os.path.exists(path):
            os.remove(path)
        np.savez(path, **results_dict)

    # -- logging (trainer.py:242-263) --------------------------------------------------------------------
    def logger_writer_step(self, tag, losses, step, epoch=None, global_step=None):
        self.check_kernels()
        toc = (time.time() - self.step_tic) / self.cfg.SYS.LOG_INTERVAL
        self.step_tic = time.time()
        msg = '[%s] epoch: %s/%d  step: %d  global_step: %s  time: %.3f  ' % (tag, epoch, self.cfg.TRAIN.NUM_EPOCHS, step, global_step, toc)
        for k, v in self.optimizers.items():
            msg += 'lr_%s: %.1e  ' % (k, v.param_groups[0]['lr'])
        vals = torch.stack([v.detach().double().reshape(()) for v in losses.values()]).cpu().tolist()  # one D2H copy
        msg += ''.join('%s: %.5f  ' % (k, x) for k, x in zip(losses.keys(), vals))
        logging.info(msg)
        tb = getattr(self, 'tb_writer', None)
        if tb is not None and tag == 'TRAIN':  # (trainer.py:250-263: the learning rate of every parameter group, then the losses)
            for k, v in self.optimizers.items():
                for i, group in enumerate(v.param_groups):
                    tb.add_scalar('train/lr_%s' % k if i == 0 else 'train/lr_%s_%d' % (k, i), group['lr'], global_step)
            for k, x in zip(losses.keys(), vals):
                tb.add_scalar('train/%s' % k, x, global_step)
            tb.flush()

    # -- per-tensor histograms (SYS.HISTOGRAM_INTERVAL) ----------------------------------------------------------
    def write_histograms(self, global_step):
        """SYS.HISTOGRAM_INTERVAL N, master process, train steps with global_step % N == 0: weights/<name>, grads/<name> (and ema/<name>)
        histograms, weight_norm/<name> and grad_norm/<name> scalars (the square root of the histogram's own sum of squares) and
        nonfinite/<name> (the number of NaN and inf entries of the weights and the gradient, only when there are any) for every
        parameter an optimiser owns.  Called after ``graphed_or_eager_step`` has returned: eager launches on the current stream, outside
        any captured graph and after ops.join_side_stream(); no collective.  flat_grad still holds this step's exchanged gradient here:
        zero_grad runs at the start of the NEXT step.  One device-to-host copy per optimiser buffer."""
        n = getattr(self.cfg.SYS, 'HISTOGRAM_INTERVAL', None)
        tb = getattr(self, 'tb_writer', None)
        if n is None or tb is None or global_step % n != 0 or not self.is_master_process():
            return
        from ... import ops, tensor_hist
        ops.join_side_stream()
        names = {}
        for name, opt, i in self._owned_params():
            names.setdefault(id(opt), (opt, {}))[1][i] = name
        packed = []
        for opt, _ in names.values():  # every launch first, then the copies
            for prefix, which in (('weights', 'param'), ('grads', 'grad'), ('ema', 'ema')):
                if which == 'ema' and opt.ema is None:
                    continue
                counts, tallies, stats = tensor_hist.optimizer_histograms(opt, which)
                packed.append((opt, prefix, torch.cat([counts, tallies, stats.view(torch.int64)], dim=1)))
        nonfinite = {}
        for opt, prefix, dev_rows in packed:
            rows = dev_rows.cpu().numpy()  # (the one copy of this buffer's results)
            nb = tensor_hist.NUM_BUCKETS
            for i, name in sorted(names[id(opt)][1].items()):
                counts, tallies, stats = rows[i, :nb], rows[i, nb:nb + 3], rows[i, nb + 3:].view(np.float64)
                fields = tensor_hist.to_proto_fields(counts, tallies, stats)
                if fields is not None:  # (a tensor without a finite element has no histogram: its tallies say why)
                    tb.add_histogram_raw('%s/%s' % (prefix, name), *fields, step=global_step)
                if prefix != 'ema':
                    tb.add_scalar('%s_norm/%s' % (prefix[:-1], name), float(np.sqrt(stats[3])), global_step)
                    nonfinite[name] = nonfinite.get(name, 0) + int(tallies[1] + tallies[2])
        for name, bad in nonfinite.items():
            if bad:
                tb.add_scalar('nonfinite/%s' % name, bad, global_step)
        tb.flush()

    def tb_epoch_scalars(self, prefix, values, epoch):
        """SYS.TENSORBOARD: ``<prefix>/<k>`` at step = epoch (trainer.py:279-280, 291-294)"""
        tb = getattr(self, 'tb_writer', None)
        if tb is not None:
            for k, v in values.items():
                tb.add_scalar('%s/%s' % (prefix, k), float(v), epoch)
            tb.flush()

    def train_step(self, batch, t_step, global_step, epoch):
        raise NotImplementedError

    def test_step(self, batch, t_step, epoch=0):
        raise NotImplementedError

    def evaluate_epoch(self, results_dict):
        return {}

    def val_observers(self):
        """the ordered list of what this pipeline accumulates on the device at validation (val_observers.py); the base pipeline: nothing"""
        return []

    # -- loops (trainer.py:367-427) ----------------------------------------------------------------------
    def train(self, cfg, exp_tag, resume_from=None):
        """``pipeline.train(cfg, exp_tag, args.resume_from)`` as main.py:51 calls it (trainer.py:367).  ``cfg`` is the object
        the pipeline was constructed with; like the reference, the loop reads ``self.cfg``."""
        self.base_path, epoch_start, global_step = self.setup_experiment(True, exp_tag, resume_from=resume_from)
        self.setup_video_writer()  # (trainer.py:374; only with SYS.RENDER_VIDEO, on the master process)
        self.setup_tb_writer()  # (trainer.py:373; only with SYS.TENSORBOARD, on the master process)
        if self.cfg.SYS.DISTRIBUTED:
            torch.distributed.barrier()
        for epoch in range(epoch_start, self.cfg.TRAIN.NUM_EPOCHS):
            self.model.train()
            tic = time.time()
            if getattr(self, 'train_sampler', None) is not None:
                self.train_sampler.set_epoch(epoch + 1)  # the reference counts epochs from 1 (trainer.py:379,384)
            for t_step, batch in enumerate(self.train_dataloader):
                global_step += 1
                self.train_step(batch, t_step + 1, global_step, epoch + 1)
            if (epoch + 1) % self.cfg.TRAIN.CHECKPOINT_INTERVAL == 0:  # validation rides on the checkpoint interval (:389-394)
                self.check_kernels_all_ranks()  # collective: no rank's lost partner may reach the file rank 0 writes
                if self.is_master_process():
                    self.save_checkpoint(epoch + 1, global_step)
                if self.cfg.TRAIN.VALIDATE:
                    self.validate(self.test_dataloader, epoch + 1)
            for s in self.schedulers.values():
                s.step()
            if self.is_master_process():
                epoch_toc = (time.time() - tic) / 3600
                logging.info('[TRAIN] epoch_time: %.2f hours' % epoch_toc)
                # (trainer.py:399-402: the reference's mean runs over this epoch alone)
                self.tb_epoch_scalars('train', {'epoch_time': epoch_toc, 'ETA': (self.cfg.TRAIN.NUM_EPOCHS - epoch - 1) * epoch_toc}, epoch + 1)
                if getattr(self.cfg.SYS, 'EPOCH_FIGURES', False):
                    self.write_epoch_figures(epoch + 1)  # (trainer.py:404-405)

    @torch.no_grad()
    def validate(self, test_dataloader=None, epoch=0, tag='VAL'):
        """trainer.py:407-427 (same positional signature).  Data-parallel runs first take rank 0's buffers (dp.sync_buffers):
        eval-mode BatchNorm then reads the same running statistics on every rank, as under DDP's per-forward buffer
        broadcast."""
        with self.eval_weights():
            return self._validate(test_dataloader, epoch, tag)

    def _validate(self, test_dataloader, epoch, tag):
        from ... import dp
        test_dataloader = self.test_dataloader if test_dataloader is None else test_dataloader
        self.apply_knobs()
        if self.cfg.SYS.DISTRIBUTED:
            dp.sync_buffers(self.model)
        self.model.eval()
        tic = time.time()
        sums, coll = {}, {}
        observers = [o for o in self.val_observers() if o.enabled(self.cfg)]
        for o in observers:
            o.reset()
        for t_step, batch in enumerate(test_dataloader):
            losses, res = self.test_step(batch, t_step + 1, epoch)
            for k, v in losses.items():
                sums[k] = sums.get(k, 0) + v
            for k, v in res.items():
                coll.setdefault(k, []).append(v)
        self.check_kernels_all_ranks()
        out = {k: v / self.num_test_samples for k, v in sums.items()}
        if coll and self.is_master_process():  # (nothing was collected when the features stayed on the device)
            out.update(self.evaluate_epoch({k: np.concatenate(v, axis=0) for k, v in coll.items()}))
        for o in observers:  # collective: every rank takes part in the all-gather of the states and gets the whole set's values
            out.update(o.epoch(epoch, tag))
        if self.is_master_process():
            logging.info('[VAL] epoch: %d  val_time: %.1f min  ' % (epoch, (time.time() - tic) / 60) +
                         ''.join('%s: %.5f  ' % (k, float(v)) for k, v in out.items()))
            self.tb_epoch_scalars(tag.lower(), out, epoch)  # (val/<k> from train(), test/<k> from test())
        return out

    def test(self, cfg, exp_tag, checkpoint):
        """``pipeline.test(cfg, exp_tag, args.checkpoint)`` (main.py:48, trainer.py:429)."""
        self.base_path = self.setup_experiment(False, exp_tag, checkpoint=checkpoint)
        self.setup_video_writer()
        self.setup_tb_writer()
        return self.validate(self.test_dataloader, 0, tag='TEST')

    @torch.no_grad()
    def demo(self, cfg, exp_tag, checkpoint, demo_input):
        """``pipeline.demo(cfg, exp_tag, args.checkpoint, args.demo_input)`` (main.py:45, trainer.py:459).  Variable-length inference on wav input (trainer.py:459-484): one demo_step per clip, or DEMO.MULTIPLE steps with the
        code interpolation coefficient swept over [0, 1].  Returns the list of results dicts (the reference only writes
        videos / npz files)."""
        self.base_path = self.setup_experiment(False, exp_tag, checkpoint=checkpoint, demo_input=demo_input)
        self.setup_video_writer()
        self.setup_tb_writer()
        self.model.eval()
        with self.eval_weights():
            return self._demo_steps()

    def _demo_steps(self):
        out = []
        for t_step, batch in enumerate(self.test_dataloader):
            m = self.cfg.DEMO.MULTIPLE
            if m > 1:
                for i in range(m):
                    out.append(self.demo_step(batch, t_step + 1, epoch=0, extra_id=i, interpolation_coeff=i / (m - 1)))
            else:
                out.append(self.demo_step(batch, t_step + 1, epoch=0))
        return out
