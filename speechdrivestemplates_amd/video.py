"""Video / long-image writer (core/utils/video_processing.py:13-138): the reference's signature, file names and SYS.VIDEO_FORMAT
semantics, fed by the GPU renderer (render.py).

  'mp4'         <base>/videos/epoch<E>-<TAG>-step<S>[-<id>].mp4 with the clip's audio, and the .wav beside it.  An ``ffmpeg``
                executable on PATH is called with an argument list (no ffmpeg-python).  Without one, the %06d.jpg frames stay in
                <base>/videos/epoch<E>-<TAG>-step<S>[-<id>]/ next to the wav and this is logged once.
  'img'         <base>/imgs/epoch<E>-DEMO-step<S>[-<id>].jpg, the long image, DEMO only, JPEG quality 95 (cv2.imwrite's default).
  'avi'         <base>/videos/epoch<E>-<TAG>-step<S>[-<id>].avi, Motion-JPEG with the clip's audio as PCM (avi.py): needs no ffmpeg.
                Not in the default list.  Device frames are encoded on the GPU (jpeg.py), numpy frames with PIL.
  'tensorboard' with a ``writer`` (tb_events.EventWriter; the Trainer passes its own when SYS.TENSORBOARD is set): the clip shrunk by 0.4 as an
                animated GIF in an image summary, which is what the reference's ``add_video`` stores: tag ``train/video`` at global_step
                for TRAIN, ``<tag>/video/<step>`` at the epoch for VAL / TEST, ``/<extra_id>`` appended; nothing for DEMO.  Device frames
                are shrunk, quantised and LZW-coded on the GPU (gif.py), numpy frames by gif.model_downscale and
                PIL.  Without a writer: warned once and skipped.

Frames arrive as (T, H, W, 3) uint8 BGR device tensors (or numpy arrays); the device -> host copy goes through pinned memory, and
the JPEGs are written from RGB (PIL).  With SYS.DEVICE_JPEG, device frames and the device long image are encoded to JPEG on the GPU
(jpeg.encode_frames): only compressed bytes are copied and the writers below only write files; numpy frames
keep the PIL route.  SYS.ASYNC_VIDEO_SAVING: one worker thread encodes, ``close()`` drains it.
``last_timing`` holds the seconds of the last save's device -> host copy (with SYS.DEVICE_JPEG: GPU encode + compressed copy) and encode.
"""
import io
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
    if isinstance(extra_id, str):  # (a long demo's segment: 'part01', or '<id>-part01')
        return 'epoch%d-%s-step%s-%s' % (epoch, tag, step, extra_id)
    return 'epoch%d-%s-step%s' % (epoch, tag, step) if extra_id is None else 'epoch%d-%s-step%s-%d' % (epoch, tag, step, extra_id)


def write_jpg(path, bgr, quality=95):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(path, quality=quality)


def _jpg_bytes(bgr, quality=95):
    """write_jpg's file, in memory"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, 'JPEG', quality=quality)
    return buf.getvalue()


def _on_device(x):
    return torch.is_tensor(x) and x.is_cuda


def _device_jpegs(x, quality=95):
    """device frames (T, H, W, 3) or one image (H, W, 3) -> list of complete JPEG files, encoded on the GPU"""
    from . import jpeg
    return jpeg.encode_frames(x.contiguous(), quality)


def _put_jpg(path, frame):
    """``frame``: a BGR array (PIL route) or an already encoded file (SYS.DEVICE_JPEG)"""
    if isinstance(frame, bytes):
        with open(path, 'wb') as f:
            f.write(frame)
    else:
        write_jpg(path, frame)


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
        if 'tensorboard' in formats and writer is None:
            _log_once('tensorboard', 'SYS.VIDEO_FORMAT: tensorboard output needs an event writer (SYS.TENSORBOARD); skipped')
        device_jpeg = bool(getattr(cfg.SYS, 'DEVICE_JPEG', False))
        tic = time.time()
        frames_h = long_h = avi_frames = None
        jpegs = None  # the frames as JPEG files from the GPU encoder, shared by 'mp4' (SYS.DEVICE_JPEG) and 'avi'
        if frames is not None and _on_device(frames) and (('mp4' in formats and device_jpeg) or 'avi' in formats):
            jpegs = _device_jpegs(frames)
        if 'mp4' in formats and frames is not None:
            frames_h = jpegs if jpegs is not None and device_jpeg else to_host(frames)
        if 'avi' in formats and frames is not None:
            avi_frames = jpegs if jpegs is not None else (frames_h if frames_h is not None else to_host(frames))
        if 'img' in formats and long_img is not None and tag == 'DEMO':
            long_h = _device_jpegs(long_img)[0] if device_jpeg and _on_device(long_img) else to_host(long_img)
        self.last_timing = {'d2h': time.time() - tic}
        if frames_h is not None:
            self._run(self.save_video_in_mp4, (cfg, tag, frames_h, step, epoch, global_step, _audio_np(audio), base_path, extra_id), cfg)
        if avi_frames is not None:
            size = (int(frames.shape[1]), int(frames.shape[2]))
            self._run(self.save_video_in_avi, (cfg, tag, avi_frames, size, step, epoch, global_step, _audio_np(audio), base_path, extra_id), cfg)
        if 'tensorboard' in formats and writer is not None and frames is not None and tag != 'DEMO':
            if _on_device(frames):  # encoded here, on the caller's stream; the worker only appends the record
                from . import gif
                size = gif.out_size(int(frames.shape[1]), int(frames.shape[2]))
                clip = gif.encode_gif(frames.contiguous(), cfg.DATASET.FPS)
            else:
                size, clip = None, frames_h if isinstance(frames_h, np.ndarray) else to_host(frames)
            self._run(self.save_video_in_tensorboard, (cfg, tag, clip, size, step, epoch, global_step, writer, extra_id), cfg)
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
        _put_jpg(img_path, long_img)
        vid_toc = time.time() - vid_tic
        self.last_timing['encode_img'] = vid_toc
        logging.info('[%s] epoch: %d/%d  step: %s  Saved %s in %.3f seconds.' % (tag, epoch, cfg.TRAIN.NUM_EPOCHS, step, 'long image', vid_toc))

    def save_video_in_tensorboard(self, cfg, tag, frames, size, step, epoch, global_step, writer, extra_id=None):
        """``frames``: the GIF file from the GPU encoder with its ``size`` = (h, w), or a (T, H, W, 3) BGR array that is shrunk and
        encoded here (core/utils/video_processing.py:72-98)"""
        vid_tic = time.time()
        if tag == 'TRAIN':
            clip_tag, tb_step = 'train/video', global_step
        elif tag in ('VAL', 'TEST'):
            clip_tag, tb_step = '%s/video/%d' % (tag.lower(), step), epoch
        elif tag == 'DEMO':
            return
        else:
            raise Exception('Unknown tag: %s' % tag)
        if extra_id is not None:
            clip_tag += '/%s' % extra_id
        if not isinstance(frames, bytes):
            from PIL import Image

            from . import gif
            rgb = gif.model_downscale(frames)
            size = rgb.shape[1:3]
            images = [Image.fromarray(f) for f in rgb]
            buf = io.BytesIO()
            images[0].save(buf, 'GIF', save_all=True, append_images=images[1:], duration=int(round(1000.0 / cfg.DATASET.FPS)), loop=0)
            frames = buf.getvalue()
        writer.add_image_bytes(clip_tag, frames, int(size[0]), int(size[1]), 0 if tb_step is None else tb_step)
        writer.flush()
        vid_toc = time.time() - vid_tic
        self.last_timing['encode_tensorboard'] = vid_toc
        logging.info('[%s] epoch: %d/%d  step: %s  Saved %s videos in %.3f seconds.' % (tag, epoch, cfg.TRAIN.NUM_EPOCHS, step, 'tensorboard', vid_toc))

    def save_video_in_avi(self, cfg, tag, frames, size, step, epoch, global_step, audio, base_path, extra_id=None):
        """``frames``: JPEG files from the GPU encoder, or a (T, H, W, 3) BGR array that PIL encodes here; ``size`` = (H, W)"""
        from . import avi
        vid_tic = time.time()
        vid_dir = os.path.join(base_path, 'videos')
        os.makedirs(vid_dir, exist_ok=True)
        jpegs = [frame if isinstance(frame, bytes) else _jpg_bytes(frame) for frame in frames]
        vid_path = os.path.join(vid_dir, _stem(epoch, tag, step, extra_id) + '.avi')
        avi.write_avi(vid_path, jpegs, cfg.DATASET.FPS, size[1], size[0], audio=audio, sample_rate=cfg.DATASET.AUDIO_SR)
        vid_toc = time.time() - vid_tic
        self.last_timing['encode_avi'] = vid_toc
        logging.info('[%s] epoch: %d/%d  step: %s  Saved %s videos in %.3f seconds.' % (tag, epoch, cfg.TRAIN.NUM_EPOCHS, step, 'avi', vid_toc))

    def save_video_in_mp4(self, cfg, tag, frames, step, epoch, global_step, audio, base_path, extra_id=None):
        vid_tic = time.time()
        vid_dir = os.path.join(base_path, 'videos')
        stem = _stem(epoch, tag, step, extra_id)
        ffmpeg = shutil.which('ffmpeg')
        frame_dir = os.path.join(vid_dir, 'tmp', '%f' % time.time()) if ffmpeg else os.path.join(vid_dir, stem)
        os.makedirs(frame_dir, exist_ok=True)
        for idx, frame in enumerate(frames):
            _put_jpg(os.path.join(frame_dir, '%06d.jpg' % idx), frame)
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
