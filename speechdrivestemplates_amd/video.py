"""Video / long-image writer (core/utils/video_processing.py:13-138): the reference's signature, file names and SYS.VIDEO_FORMAT
semantics, fed by the GPU renderer (render.py).

  'mp4'         <base>/videos/epoch<E>-<TAG>-step<S>[-<id>].mp4 with the clip's audio, and the .wav beside it.  An ``ffmpeg``
                executable on PATH is called with an argument list (no ffmpeg-python).  Without one, the %06d.jpg frames stay in
                <base>/videos/epoch<E>-<TAG>-step<S>[-<id>]/ next to the wav and this is logged once.
  'img'         <base>/imgs/epoch<E>-DEMO-step<S>[-<id>].jpg, the long image, DEMO only, JPEG quality 95 (cv2.imwrite's default).
  'tensorboard' not available in this engine: warned once and skipped.

Frames arrive as (T, H, W, 3) uint8 BGR device tensors (or numpy arrays); the device -> host copy goes through pinned memory, and
the JPEGs are written from RGB (PIL).  SYS.ASYNC_VIDEO_SAVING: one worker thread encodes, ``close()`` drains it.
``last_timing`` holds the seconds of the last save's device -> host copy and encode.
"""
import logging
import os
import queue
import shutil
import subprocess
import threading
import time

import numpy as np
import torch

_once = set()


def _log_once(key, msg, level=logging.WARNING):
    if key not in _once:
        _once.add(key)
        logging.log(level, msg)


def to_host(x):
    """device tensor -> numpy through a pinned staging buffer; numpy / CPU tensors pass through."""
    if x is None or isinstance(x, np.ndarray):
        return x
    if not x.is_cuda:
        return x.detach().numpy()
    buf = torch.empty(x.shape, dtype=x.dtype, pin_memory=True)
    buf.copy_(x, non_blocking=True)
    torch.cuda.current_stream(x.device).synchronize()
    return buf.numpy()


def _audio_np(audio):
    if audio is None:
        return None
    if torch.is_tensor(audio):
        audio = audio.detach().cpu().numpy()
    return np.asarray(audio)


def _stem(epoch, tag, step, extra_id):
    return 'epoch%d-%s-step%s' % (epoch, tag, step) if extra_id is None else 'epoch%d-%s-step%s-%d' % (epoch, tag, step, extra_id)


def write_jpg(path, bgr, quality=95):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(path, quality=quality)


class VideoWriter(object):
    def __init__(self, cfg) -> None:
        super().__init__()
        self.q = None
        self.thread = None
        self.last_timing = {}
        if cfg.SYS.ASYNC_VIDEO_SAVING:
            self.q = queue.Queue()
            self.thread = threading.Thread(target=self.worker, daemon=True)
            self.thread.start()

    def worker(self):
        while True:
            item = self.q.get()
            try:
                if item is None:
                    return
                func, args = item
                func(*args)
            except Exception:  # a failed encode must not kill the worker (the training loop goes on)
                logging.exception('video writer: saving failed')
            finally:
                self.q.task_done()

    def close(self):
        """wait for every queued save, then stop the worker thread"""
        if self.q is not None and self.thread is not None:
            self.q.put(None)
            self.q.join()
            self.thread.join()
            self.thread = None

    def _run(self, func, args, cfg):
        if self.q is not None and self.thread is not None:
            self.q.put((func, args))
        else:
            func(*args)

    def save_video(self, cfg, tag, frames, step, epoch, global_step=None, long_img=None, audio=None, writer=None, base_path=None,
                   extra_id=None):
        formats = cfg.SYS.VIDEO_FORMAT
        if 'tensorboard' in formats:
            _log_once('tensorboard', 'SYS.VIDEO_FORMAT: tensorboard output is not provided by this engine; skipped')
        tic = time.time()
        frames_h = to_host(frames) if 'mp4' in formats and frames is not None else None
        long_h = to_host(long_img) if 'img' in formats and long_img is not None and tag == 'DEMO' else None
        self.last_timing = {'d2h': time.time() - tic}
        if frames_h is not None:
            self._run(self.save_video_in_mp4, (cfg, tag, frames_h, step, epoch, global_step, _audio_np(audio), base_path, extra_id), cfg)
        if 'img' in formats:
            self._run(self.save_video_in_long_img, (cfg, tag, long_h, step, epoch, global_step, base_path, extra_id), cfg)

    def save_video_in_long_img(self, cfg, tag, long_img, step, epoch, global_step, base_path, extra_id=None):
        vid_tic = time.time()
        if tag != 'DEMO' or long_img is None:
            return
        img_dir = os.path.join(base_path, 'imgs')
        os.makedirs(img_dir, exist_ok=True)
        img_path = os.path.join(img_dir, _stem(epoch, tag, step, extra_id) + '.jpg')
        if os.path.exists(img_path):
            os.remove(img_path)
        write_jpg(img_path, long_img)
        vid_toc = time.time() - vid_tic
        self.last_timing['encode_img'] = vid_toc
        logging.info('[%s] epoch: %d/%d  step: %s  Saved %s in %.3f seconds.' % (tag, epoch, cfg.TRAIN.NUM_EPOCHS, step, 'long image', vid_toc))

    def save_video_in_mp4(self, cfg, tag, frames, step, epoch, global_step, audio, base_path, extra_id=None):
        vid_tic = time.time()
        vid_dir = os.path.join(base_path, 'videos')
        stem = _stem(epoch, tag, step, extra_id)
        ffmpeg = shutil.which('ffmpeg')
        frame_dir = os.path.join(vid_dir, 'tmp', '%f' % time.time()) if ffmpeg else os.path.join(vid_dir, stem)
        os.makedirs(frame_dir, exist_ok=True)
        for idx, frame in enumerate(frames):
            write_jpg(os.path.join(frame_dir, '%06d.jpg' % idx), frame)
        wav_path = None
        if audio is not None:
            from scipy.io.wavfile import write
            wav_path = os.path.join(vid_dir, stem + '.wav')
            write(wav_path, cfg.DATASET.AUDIO_SR, audio)
        if ffmpeg:
            vid_path = os.path.join(vid_dir, stem + '.mp4')
            if os.path.exists(vid_path):
                os.remove(vid_path)
            cmd = [ffmpeg, '-y', '-loglevel', 'error', '-framerate', str(cfg.DATASET.FPS), '-i', os.path.join(frame_dir, '%06d.jpg')]
            if wav_path is not None:
                cmd += ['-i', wav_path]
            cmd += ['-vf', 'pad=ceil(iw/2)*2:ceil(ih/2)*2', '-pix_fmt', 'yuv420p', vid_path]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode == 0:
                shutil.rmtree(frame_dir, ignore_errors=True)
            else:
                keep = os.path.join(vid_dir, stem)
                shutil.rmtree(keep, ignore_errors=True)
                shutil.move(frame_dir, keep)
                logging.error('ffmpeg failed (%d): %s; frames kept in %s' % (r.returncode, r.stderr.strip()[-500:], keep))
        else:
            _log_once('ffmpeg', 'no ffmpeg executable on PATH: video frames are kept as JPEGs in %s/<name>/ next to the .wav' % vid_dir,
                      logging.INFO)
        vid_toc = time.time() - vid_tic
        self.last_timing['encode'] = vid_toc
        logging.info('[%s] epoch: %d/%d  step: %s  Saved %s videos in %.3f seconds.' % (tag, epoch, cfg.TRAIN.NUM_EPOCHS, step, 'mp4', vid_toc))
