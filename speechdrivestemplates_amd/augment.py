"""Audio augmentation inside the train step: gain, white noise, shift, polarity and mel masks (TRAIN.AUGMENT).

Everything random is a word of Philox4x32-10 with the key (SEED low 32 bits, SEED high 32 bits) and the counter
(block j, purpose, clip index low 32 bits, step low 32 bits), so what a clip hears depends on (seed, step, clip) only -- not on the rank, the
clip's row in the batch or the batch size.  Purpose 0 holds the clip's parameters (block 0, words w0 .. w3) and its mel masks (blocks 1 .. nf
the frequency bands, 5 .. 4 + nt the time spans); purpose 1 holds the noise: sample n takes block n >> 1, words 2 (n & 1) and 2 (n & 1) + 1.

    gain      ig = w0 >> 24, dB = -G + 2 G (ig + 0.5) / 256, g = float32(10 ** (dB / 20)) from a 256-entry table (computed here in float64)
    SNR       is = w1 >> 24, dB = lo + (hi - lo) (is + 0.5) / 256, a = 10 ** (-dB / 20) from a 256-entry float64 table;
              the noise is on iff (w3 >> 8) < floor(NOISE_PROB 2^24)
    shift     S = floor(SHIFT_MS AUDIO_SR / 1000), s = (w2 mod (2 S + 1)) - S, x_s[n] = x[n - s] inside [0, L), else +0.0
    polarity  w3 & 1 negates g
    noise     z[n] = (h0 + h1 + h2 + h3 - 131070) C over the four 16-bit halves of the sample's two words, C = 0x1.bb67ae86627e7p-16:
              a centred four-term Irwin-Hall variate of unit variance
    sigma     sqrt(ss / L) a in float64, ss the sum of the squares of the L unshifted samples in the order ``sumsq_model`` states; 0.0 with the
              noise off
    output    y[n] = float32(float64(g) (float64(x_s[n]) + sigma z[n])), every operation rounded on its own; with the noise off no noise term
              is formed: y[n] = float32(float64(g) float64(x_s[n])), so a -0.0 keeps its sign and neutral options return the input's bits
    mel mask  mask i of a dimension of size D, largest width w: width = w0 mod (w + 1) clipped to D, start = w1 mod (D - width + 1); the
              rectangle spans the whole other dimension and is set to +0.0 in place

The moduli are biased: a residue's probability is off by at most (2 S + 1) 2^-32, (w + 1) 2^-32 resp. D 2^-32 -- accepted.

Two routes that run the same operations in the same order.  ``philox4x32`` / ``sumsq_model`` / ``clip_params_model`` / ``audio_model`` /
``mel_mask_model`` are the contract in numpy; ``sumsq`` / ``augment_audio`` / ``mel_mask`` run csrc/augment.hip on CUDA tensors.  There is no
CPU fallback.  ``Augmenter`` is what ``Voice2PoseModel.forward`` uses.

    python -m speechdrivestemplates_amd.augment IN.wav OUT.wav --step N --clip I [--seed ..] [--gain-db ..] [--snr lo hi] [--shift-ms ..]
                                                                [--polarity]

writes what the model would hear of IN.wav as clip I at step N (on the GPU) and prints the record.
"""
import math

import numpy as np

from ._exact_model import _butterfly_wave

REC_COLS = 32  # words of a clip's record (SDT_AUGMENT_REC_COLS)
IG, IS, SHIFT, POLARITY, NOISE_ON, SIGMA, SS, NONFINITE, FREQ0, TIME0, NF, NT = 0, 1, 2, 3, 4, 5, 6, 7, 8, 16, 24, 25
CHUNK, LANES, MAX_MASKS, MAX_L, MAX_B = 1024, 64, 4, 1 << 24, 65535
NOISE_SCALE = float.fromhex('0x1.bb67ae86627e7p-16')  # 1 / sqrt(4 (65536^2 - 1) / 12)
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xffffffff)
_NO_GPU = 'the augmentation is computed on the GPU (csrc/augment.hip); there is no CPU fallback (audio_model / mel_mask_model are the numpy ' \
          'contract)'
NEUTRAL = {'seed': 0, 'gain_db': 0.0, 'snr': None, 'noise_prob': 1.0, 'shift_ms': 0.0, 'shift': 0, 'polarity': False, 'freq_masks': (0, 0),
           'time_masks': (0, 0)}


def options(**kw):
    """the options dict ``config.check_augment`` returns, from keywords (the rest neutral); 'shift' is in samples"""
    unknown = set(kw) - set(NEUTRAL)
    if unknown:
        raise ValueError('unknown augmentation option(s): %s' % ', '.join(sorted(unknown)))
    out = dict(NEUTRAL, **kw)
    out['snr'] = None if out['snr'] is None else (float(out['snr'][0]), float(out['snr'][1]))
    out['freq_masks'], out['time_masks'] = tuple(int(v) for v in out['freq_masks']), tuple(int(v) for v in out['time_masks'])
    if not 0 <= int(out['seed']) < 1 << 64:
        raise ValueError('the seed must lie in [0, 2^64), got %r' % (out['seed'],))
    if not 0 <= int(out['shift']) <= MAX_L:
        raise ValueError('the largest shift must lie in [0, 2^24] samples, got %r' % (out['shift'],))
    for name in ('freq_masks', 'time_masks'):
        if len(out[name]) != 2 or not 0 <= out[name][0] <= MAX_MASKS or out[name][1] < 0:
            raise ValueError('%s must be (n, w) with n from 0 to 4 and w >= 0, got %r' % (name, out[name]))
    return out


# ---- the numpy contract models ---------------------------------------------------------------------------------------------------------------
def philox4x32(counter, key):
    """Philox4x32-10: ``counter`` (..., 4) and ``key`` (2,) of 32-bit words -> (..., 4) uint32"""
    c = np.asarray(counter, dtype=np.uint64) & _MASK32
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = (int(k) & 0xffffffff for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _MASK32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _MASK32
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _key(seed):
    return int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff


def _words(block, purpose, clip, step, seed):
    """the four words of one block as Python ints"""
    return [int(w) for w in philox4x32([int(block), int(purpose), int(clip) & 0xffffffff, int(step) & 0xffffffff], _key(seed))]


def gain_table(gain_db):
    """256 float32 factors: level ig is -G + 2 G (ig + 0.5) / 256 dB"""
    G = float(gain_db)
    return np.array([10.0 ** ((-G + 2.0 * G * (i + 0.5) / 256.0) / 20.0) for i in range(256)], dtype=np.float64).astype(np.float32)


def snr_table(snr):
    """256 float64 factors a = 10 ** (-dB / 20): level is is lo + (hi - lo) (is + 0.5) / 256 dB (ones without noise)"""
    if snr is None:
        return np.ones(256, dtype=np.float64)
    lo, hi = float(snr[0]), float(snr[1])
    return np.array([10.0 ** (-(lo + (hi - lo) * (i + 0.5) / 256.0) / 20.0) for i in range(256)], dtype=np.float64)


def noise_prob24(opts):
    """the noise is on iff (w3 >> 8) < this"""
    return 0 if opts['snr'] is None else int(math.floor(float(opts['noise_prob']) * (1 << 24)))


def sumsq_model(x):
    """(B, L) float32 -> (B,) float64: the sum of squares in the order of sdt_augment_sumsq_f64"""
    x = np.asarray(x, dtype=np.float32)
    B, L = x.shape
    n_chunks = -(-L // CHUNK)
    with np.errstate(all='ignore'):
        sq = np.zeros((B, n_chunks * CHUNK))
        sq[:, :L] = x.astype(np.float64) * x.astype(np.float64)
        sq = sq.reshape(B, n_chunks, 4, 256)  # [chunk, k, thread]: sample 1024 c + 256 k + t
        s = np.zeros((B, n_chunks, 256))
        for k in range(4):
            s = s + sq[:, :, k]
        waves = _butterfly_wave(s.reshape(B, n_chunks, 4, LANES))
        partials = ((waves[..., 0] + waves[..., 1]) + waves[..., 2]) + waves[..., 3]
        rounds = -(-n_chunks // LANES)
        p = np.zeros((B, rounds * LANES))
        p[:, :n_chunks] = partials
        p = p.reshape(B, rounds, LANES)
        s = np.zeros((B, LANES))
        for j in range(rounds):
            s = s + p[:, j]
        return _butterfly_wave(s)


def clip_params_model(opts, clip, step, ss=0.0, L=1, words=None):
    """one clip's parameters: {'ig', 'is', 's', 'polarity', 'noise', 'g' (float32, signed), 'a', 'sigma', 'ss', 'nonfinite'}.  ``words``: the
    four words of block 0 in place of the Philox draw (the tests' extremes)"""
    w = _words(0, 0, clip, step, opts['seed']) if words is None else [int(v) & 0xffffffff for v in words]
    S = int(opts['shift'])
    ig, i_s = w[0] >> 24, w[1] >> 24
    s = (w[2] % (2 * S + 1)) - S
    noise = int((w[3] >> 8) < noise_prob24(opts))
    flip = int(bool(opts['polarity']) and (w[3] & 1))
    g = gain_table(opts['gain_db'])[ig]
    a = snr_table(opts['snr'])[i_s]
    ss = np.float64(ss)
    with np.errstate(all='ignore'):
        sigma = np.sqrt(ss / np.float64(L)) * a if noise else np.float64(0.0)
    return {'ig': ig, 'is': i_s, 's': s, 'polarity': flip, 'noise': noise, 'g': np.float32(-g if flip else g), 'a': a, 'sigma': sigma,
            'ss': ss, 'nonfinite': int(not np.isfinite(ss))}


def noise_model(L, clip, step, seed):
    """z[0 .. L) float64 of one clip"""
    blocks = np.arange((L + 1) // 2, dtype=np.uint64)
    counter = np.stack([blocks, np.full_like(blocks, 1), np.full_like(blocks, int(clip) & 0xffffffff),
                        np.full_like(blocks, int(step) & 0xffffffff)], axis=-1)
    w = philox4x32(counter, _key(seed)).astype(np.int64).reshape(-1, 2, 2)  # [block, n & 1, word]
    h = (w & 0xffff).sum(-1) + (w >> 16).sum(-1) - 131070
    return (h.reshape(-1)[:L].astype(np.float64)) * NOISE_SCALE


def _record(p):
    r = np.zeros(REC_COLS, dtype=np.int64)
    r[IG], r[IS], r[SHIFT], r[POLARITY], r[NOISE_ON], r[NONFINITE] = p['ig'], p['is'], p['s'], p['polarity'], p['noise'], p['nonfinite']
    r[SIGMA], r[SS] = np.float64(p['sigma']).view(np.int64), np.float64(p['ss']).view(np.int64)
    return r


def audio_model(x, clip_index, step, opts):
    """(B, L) float32 -> ((B, L) float32, records (B, 32) int64): sdt_augment_sumsq_f64 + sdt_augment_audio_f32"""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    B, L = x.shape
    clip_index = np.asarray(clip_index, dtype=np.int64).reshape(B)
    ss = sumsq_model(x)
    y, rec = np.empty_like(x), np.zeros((B, REC_COLS), dtype=np.int64)
    with np.errstate(all='ignore'):
        for b in range(B):
            p = clip_params_model(opts, clip_index[b], step, ss[b], L)
            rec[b] = _record(p)
            s = p['s']
            xs = np.zeros(L, dtype=np.float32)
            lo, hi = max(0, s), min(L, L + s)  # n with 0 <= n - s < L
            if hi > lo:
                xs[lo:hi] = x[b, lo - s:hi - s]
            v = xs.astype(np.float64)
            if p['noise']:
                v = v + p['sigma'] * noise_model(L, clip_index[b], step, opts['seed'])
            y[b] = (np.float64(p['g']) * v).astype(np.float32)
    return y, rec


def mask_rects_model(opts, clip, step, M, F):
    """-> (frequency rectangles, time rectangles): lists of (start, width)"""
    out = []
    for (n, w), D, first in ((opts['freq_masks'], M, 1), (opts['time_masks'], F, 5)):
        rects = []
        for i in range(n):
            p = _words(first + i, 0, clip, step, opts['seed'])
            width = min(p[0] % (w + 1), D)
            rects.append((p[1] % (D - width + 1), width))
        out.append(rects)
    return out[0], out[1]


def mel_mask_model(mel, clip_index, step, opts, rec=None):
    """(B, M, F) float32 -> (the masked copy, records (B, 32) int64 with the rectangles in words 8 .. 25; ``rec``: the words to start from)"""
    mel = np.array(mel, dtype=np.float32, copy=True)
    B, M, F = mel.shape
    clip_index = np.asarray(clip_index, dtype=np.int64).reshape(B)
    rec = np.zeros((B, REC_COLS), dtype=np.int64) if rec is None else np.array(rec, dtype=np.int64, copy=True)
    for b in range(B):
        fr, tr = mask_rects_model(opts, clip_index[b], step, M, F)
        rec[b, FREQ0:NF] = 0
        for i, (start, width) in enumerate(fr):
            mel[b, start:start + width, :] = 0.0
            rec[b, FREQ0 + 2 * i], rec[b, FREQ0 + 2 * i + 1] = start, width
        for i, (start, width) in enumerate(tr):
            mel[b, :, start:start + width] = 0.0
            rec[b, TIME0 + 2 * i], rec[b, TIME0 + 2 * i + 1] = start, width
        rec[b, NF], rec[b, NT] = len(fr), len(tr)
    return mel, rec


def record_values(rec):
    """one clip's 32 words -> a dict with names"""
    rec = np.ascontiguousarray(np.asarray(rec, dtype=np.int64).reshape(REC_COLS))
    f = rec.view(np.float64)
    nf, nt = int(rec[NF]), int(rec[NT])
    return {'ig': int(rec[IG]), 'is': int(rec[IS]), 'shift': int(rec[SHIFT]), 'polarity': int(rec[POLARITY]), 'noise': int(rec[NOISE_ON]),
            'sigma': float(f[SIGMA]), 'ss': float(f[SS]), 'nonfinite': int(rec[NONFINITE]),
            'freq_masks': [(int(rec[FREQ0 + 2 * i]), int(rec[FREQ0 + 2 * i + 1])) for i in range(nf)],
            'time_masks': [(int(rec[TIME0 + 2 * i]), int(rec[TIME0 + 2 * i + 1])) for i in range(nt)]}


def describe(rec, opts):
    """one line for the log"""
    v = record_values(rec)
    G = float(opts['gain_db'])
    msg = 'gain %+.3f dB%s, shift %d samples' % (-G + 2.0 * G * (v['ig'] + 0.5) / 256.0, ' inverted' if v['polarity'] else '', v['shift'])
    if v['noise']:
        lo, hi = opts['snr']
        msg += ', noise at %.2f dB SNR (sigma %.6g)' % (lo + (hi - lo) * (v['is'] + 0.5) / 256.0, v['sigma'])
    else:
        msg += ', no noise'
    msg += ', rms %.6g' % math.sqrt(v['ss']) if v['ss'] >= 0 else ''
    for name in ('freq_masks', 'time_masks'):
        if v[name]:
            msg += ', %s %s' % (name, v[name])
    return msg + ('  NONFINITE' if v['nonfinite'] else '')


# ---- the device route (csrc/augment.hip) -------------------------------------------------------------------------------------------------------
def _dev_tensor(x, dtype, what):
    import torch
    if not torch.is_tensor(x) or x.device.type != 'cuda':
        raise RuntimeError('%s must be a CUDA tensor; %s' % (what, _NO_GPU))
    if x.dtype != dtype:
        raise TypeError('%s must be %s, got %s' % (what, dtype, x.dtype))
    return x.detach().contiguous()


def _call(fn, device, *args):
    import torch
    from . import _lib
    with torch.cuda.device(device):
        _lib.check(fn(*args, torch.cuda.current_stream(device).cuda_stream))


def _ptr(t):
    import ctypes as C
    return C.c_void_p(t.data_ptr())


def _index_tensors(clip_index, step, B, device):
    import torch
    clip_index = _dev_tensor(clip_index, torch.int64, 'clip_index').reshape(-1)
    step = _dev_tensor(step, torch.int64, 'the step').reshape(-1)
    if clip_index.numel() != B or step.numel() != 1 or clip_index.device != device or step.device != device:
        raise ValueError('clip_index must be (%d,) and the step (1,), int64 on %s; got %s and %s'
                         % (B, device, tuple(clip_index.shape), tuple(step.shape)))
    return clip_index, step


def _check_audio(x):
    import torch
    x = _dev_tensor(x, torch.float32, 'the audio')
    if x.ndim != 2 or not 1 <= x.shape[0] <= MAX_B or not 1 <= x.shape[1] <= MAX_L:
        raise ValueError('the audio must be (B, L) with B in [1, %d] and L in [1, 2^24], got %s' % (MAX_B, tuple(x.shape)))
    return x


def sumsq(x, work=None, out=None):
    """(B, L) float32 on the GPU -> (B,) float64, the clips' sums of squares (``work``, ``out``: buffers to use instead of new ones)"""
    import torch
    from . import _lib
    x = _check_audio(x)
    B, L = (int(v) for v in x.shape)
    lib = _lib.load()
    if work is None:
        work = torch.empty(int(lib.sdt_augment_workspace_bytes(B, L)) // 8, dtype=torch.float64, device=x.device)
    if out is None:
        out = torch.empty(B, dtype=torch.float64, device=x.device)
    _call(lib.sdt_augment_sumsq_f64, x.device, _ptr(x), B, L, _ptr(work), _ptr(out))
    return out


def device_tables(opts, device):
    """(gain table (256,) float32, SNR table (256,) float64) on ``device``: uploaded once by whoever holds them"""
    import torch
    return torch.from_numpy(gain_table(opts['gain_db'])).to(device), torch.from_numpy(snr_table(opts['snr'])).to(device)


def augment_audio(x, clip_index, step, opts, tables=None, ss=None, rec=None, out=None):
    """(B, L) float32 on the GPU, clip_index (B,) and step (1,) int64 on the GPU -> (a new (B, L) tensor, the records (B, 32) int64).
    ``tables``: ``device_tables`` kept by the caller; ``ss``: the clips' sums of squares if already computed; ``rec`` / ``out``: buffers to
    write into (``out`` a contiguous (B, L) float32 view that is not the input)"""
    import torch
    from . import _lib
    x = _check_audio(x)
    B, L = (int(v) for v in x.shape)
    clip_index, step = _index_tensors(clip_index, step, B, x.device)
    gain, snr = device_tables(opts, x.device) if tables is None else tables
    ss = sumsq(x) if ss is None else ss
    if rec is None:
        rec = torch.empty((B, REC_COLS), dtype=torch.int64, device=x.device)
    if out is None:
        out = torch.empty_like(x)
    if out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError('out must be a contiguous float32 tensor of shape %s on %s' % (tuple(x.shape), x.device))
    _call(_lib.load().sdt_augment_audio_f32, x.device, _ptr(x), B, L, _ptr(clip_index), _ptr(step), _ptr(ss), int(opts['seed']),
          int(opts['shift']), noise_prob24(opts), int(bool(opts['polarity'])), _ptr(gain), _ptr(snr), _ptr(rec), _ptr(out))
    return out, rec


def mel_mask(mel, clip_index, step, opts, rec=None):
    """(B, M, F) float32 on the GPU, masked IN PLACE -> the records (B, 32) int64 (``rec``, or zeros, with the rectangles in words 8 .. 25)"""
    import torch
    from . import _lib
    if not torch.is_tensor(mel) or mel.device.type != 'cuda':
        raise RuntimeError('the mel must be a CUDA tensor; %s' % _NO_GPU)
    if mel.dtype != torch.float32 or mel.ndim != 3 or not mel.is_contiguous():
        raise ValueError('the mel must be a contiguous float32 (B, M, F) tensor, got %s %s' % (mel.dtype, tuple(mel.shape)))
    B, M, F = (int(v) for v in mel.shape)
    clip_index, step = _index_tensors(clip_index, step, B, mel.device)
    if rec is None:
        rec = torch.zeros((B, REC_COLS), dtype=torch.int64, device=mel.device)
    (nf, wf), (nt, wt) = opts['freq_masks'], opts['time_masks']
    _call(_lib.load().sdt_augment_mel_mask_f32, mel.device, _ptr(mel.detach()), B, M, F, _ptr(clip_index), _ptr(step), int(opts['seed']), nf, wf,
          nt, wt, _ptr(rec))
    return rec


class Augmenter:
    """the tables (uploaded once) and the workspaces of one device: ``audio`` before the mel front end, ``mel_masks`` behind it.  Buffers are
    allocated at the first call of a shape -- in the eager steps that precede a graph capture -- and a replay allocates nothing.  ``record``
    is the (B, 32) int64 record of the last call, on the device."""

    def __init__(self, opts, device):
        import torch
        self.opts, self.device = opts, torch.device(device)
        self.tables = device_tables(opts, self.device)
        self.masks = any(n > 0 and w > 0 for n, w in (opts['freq_masks'], opts['time_masks']))
        self._bufs = {}
        self.record = None

    def _buffers(self, B, L):
        import torch
        from . import _lib
        if (B, L) not in self._bufs:
            work = torch.empty(int(_lib.load().sdt_augment_workspace_bytes(B, L)) // 8, dtype=torch.float64, device=self.device)
            self._bufs[(B, L)] = (work, torch.empty(B, dtype=torch.float64, device=self.device),
                                  torch.zeros((B, REC_COLS), dtype=torch.int64, device=self.device))
        return self._bufs[(B, L)]

    def audio(self, x, clip_index, step):
        """(B, L) float32 -> a new (B, L) tensor"""
        x = _check_audio(x)
        work, ss, rec = self._buffers(int(x.shape[0]), int(x.shape[1]))
        sumsq(x, work, ss)
        y, self.record = augment_audio(x, clip_index, step, self.opts, self.tables, ss, rec)
        return y

    def mel_masks(self, mel, clip_index, step):
        """(B, M, F) float32, in place; the rectangles join ``record`` (the record of the ``audio`` call of the same batch)"""
        if not self.masks:
            return mel
        rec = self.record if self.record is not None and self.record.shape[0] == mel.shape[0] else None
        self.record = mel_mask(mel, clip_index, step, self.opts, rec)
        return mel


# ---- command line ------------------------------------------------------------------------------------------------------------------------------
def read_wav(path):
    """-> (sample rate, (L,) float32 in [-1, 1), the file's dtype): 16-bit or float PCM, the first channel of several"""
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    if data.ndim == 2:
        data = data[:, 0]
    if data.dtype == np.int16:
        return int(sr), (data.astype(np.float32) / np.float32(32768.0)), np.int16
    if data.dtype in (np.float32, np.float64):
        return int(sr), data.astype(np.float32), np.float32
    raise ValueError('%s: 16-bit or float PCM expected, got %s' % (path, data.dtype))


def write_wav(path, sr, y, dtype):
    from scipy.io import wavfile
    y = np.asarray(y, dtype=np.float32)
    if dtype == np.int16:
        y = np.clip(np.rint(y.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    wavfile.write(path, int(sr), y)


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='write what the model would hear of a wav file as clip I at train step N, and print the record')
    ap.add_argument('inp', metavar='IN.wav')
    ap.add_argument('out', metavar='OUT.wav')
    ap.add_argument('--step', type=int, required=True, metavar='N', help='the global train step')
    ap.add_argument('--clip', type=int, required=True, metavar='I', help='the clip index')
    ap.add_argument('--seed', type=int, default=0, help='TRAIN.AUGMENT.SEED')
    ap.add_argument('--gain-db', type=float, default=0.0, metavar='G', help='TRAIN.AUGMENT.GAIN_DB, 0 .. 40')
    ap.add_argument('--snr', type=float, nargs=2, default=None, metavar=('lo', 'hi'), help='TRAIN.AUGMENT.NOISE_SNR_DB, -20 <= lo <= hi <= 80')
    ap.add_argument('--noise-prob', type=float, default=1.0, help='TRAIN.AUGMENT.NOISE_PROB')
    ap.add_argument('--shift-ms', type=float, default=0.0, help='TRAIN.AUGMENT.SHIFT_MS, 0 .. 500')
    ap.add_argument('--polarity', action='store_true', help='TRAIN.AUGMENT.POLARITY')
    a = ap.parse_args(argv)
    if a.step < 0 or a.clip < 0 or not 0 <= a.seed < 1 << 64:
        ap.error('--step and --clip must be >= 0 and --seed in [0, 2^64)')
    if not 0 <= a.gain_db <= 40 or not 0 <= a.shift_ms <= 500 or not 0 <= a.noise_prob <= 1:
        ap.error('--gain-db takes 0 .. 40, --shift-ms 0 .. 500, --noise-prob 0 .. 1')
    if a.snr is not None and not -20 <= a.snr[0] <= a.snr[1] <= 80:
        ap.error('--snr takes -20 <= lo <= hi <= 80')
    return a


def main(argv=None):
    a = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    sr, x, dtype = read_wav(a.inp)
    if not 1 <= x.size <= MAX_L:
        raise ValueError('%s: %d samples outside [1, 2^24]' % (a.inp, x.size))
    opts = options(seed=a.seed, gain_db=a.gain_db, snr=a.snr, noise_prob=a.noise_prob, shift_ms=a.shift_ms,
                   shift=int(math.floor(a.shift_ms * sr / 1000.0)), polarity=a.polarity)
    dev = torch.device('cuda', torch.cuda.current_device())
    y, rec = augment_audio(torch.from_numpy(x[None]).to(dev), torch.tensor([a.clip], dtype=torch.int64, device=dev),
                           torch.tensor([a.step], dtype=torch.int64, device=dev), opts)
    rec = rec.cpu().numpy()[0]
    print('clip %d at step %d: %s' % (a.clip, a.step, describe(rec, opts)))
    write_wav(a.out, sr, y.cpu().numpy()[0], dtype)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
