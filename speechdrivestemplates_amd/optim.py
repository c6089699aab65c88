"""Flat-buffer Adam: every parameter of an optimiser group is re-homed into ONE contiguous fp32 buffer (and its
gradient into a second one), so that a step is a single fused kernel launch and a data-parallel gradient
exchange is a single all-reduce.  Same update rule / defaults as ``torch.optim.Adam`` as the reference uses it
(core/pipelines/voice2pose.py:249-279): dense updates, so rows of the clip-code table with zero gradient still
have their moments decayed.  Learning rate and step counter live on the device (hipGraph-safe).

Optimiser-side safeguards (opt-in; DESIGN.md section 18, csrc/optim_guard.hip): a ``StepGuard`` measures the float64 L2 norm of a step
group's gradients on the device, derives the ``clip_grad_norm_`` scale and the "skip a non-finite step" flag from it, and the guarded
Adam kernel reads both from the device record -- no host read-back, so the step stays hipGraph-capturable.  ``FlatAdam.enable_ema``
keeps an exponential moving average of the flat parameter buffer, updated inside the same kernel pass.  ``sumsq_model`` is the numpy
contract model of the kernel's summation order (bit for bit)."""
import struct

import numpy as np
import torch

from . import ops

# launch shape of csrc/optim_guard.hip's sum of squares (checked against the library by the tests)
SUMSQ_THREADS, SUMSQ_MAX_BLOCKS = 256, 2048


def sumsq_blocks(n):
    return max(1, min(-(-(n // 4) // SUMSQ_THREADS), SUMSQ_MAX_BLOCKS))


def _tree256(acc):
    """(..., 256) per-thread float64 accumulators -> (...,): six butterfly steps inside each wave of 64, then (w0 + w1) + (w2 + w3)"""
    v = acc.reshape(acc.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    w = v[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def sumsq_model(g):
    """Contract model of ``sdt_grad_sumsq_f64``: the float64 sum of squares of the fp32 array ``g`` in the kernel's order -- thread
    t = block * 256 + lane adds the squares of the float4s t, t + T, t + 2T, ... (T = 256 * blocks; element 0 first) to an accumulator
    that starts at +0, thread t < n % 4 then the tail element's; a butterfly over each wave, (w0 + w1) + (w2 + w3) per block; one
    block over the block sums in index order (thread t: t, t + 256, ...), reduced the same way.  Adding the +0 of an idle slot is exact."""
    g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1)
    n = g.size
    nv, B = n // 4, sumsq_blocks(n)
    T = B * SUMSQ_THREADS
    trips = max(1, -(-nv // T))
    with np.errstate(over='ignore', invalid='ignore'):
        sq = np.zeros((trips * T, 4), dtype=np.float64)
        sq[:nv] = g[:4 * nv].astype(np.float64).reshape(nv, 4) ** 2
        acc = np.zeros(T, dtype=np.float64)
        for k in range(trips):
            for e in range(4):
                acc = acc + sq[k * T:(k + 1) * T, e]
        tail = g[4 * nv:].astype(np.float64) ** 2
        acc[:tail.size] = acc[:tail.size] + tail
        part = _tree256(acc.reshape(B, SUMSQ_THREADS))
        ftrips = -(-B // SUMSQ_THREADS)
        padded = np.zeros(ftrips * SUMSQ_THREADS, dtype=np.float64)
        padded[:B] = part
        facc = np.zeros(SUMSQ_THREADS, dtype=np.float64)
        for k in range(ftrips):
            facc = facc + padded[k * SUMSQ_THREADS:(k + 1) * SUMSQ_THREADS]
        return np.float64(_tree256(facc))


def sumsq_model_depth(n):
    """The largest number of float64 additions any one square passes through in ``sumsq_model``: the longest serial run of a thread
    (4 per float4 trip, + 1 tail element), the 6 + 2 tree levels of its block, the final block's serial run and its 6 + 2 levels.
    All terms are non-negative, so the sum's relative error is at most depth * 2^-53 / (1 - depth * 2^-53)."""
    B = sumsq_blocks(n)
    trips = max(1, -(-(n // 4) // (B * SUMSQ_THREADS)))
    return (4 * trips + (1 if n % 4 else 0)) + 8 + (-(-B // SUMSQ_THREADS)) + 8


class StepGuard:
    """The device-side guard of ONE step group (the optimisers that a pipeline steps together): owns the sum-of-squares partials of
    every member and the group's guard record, and issues the norm and record launches once, after the gradient exchange and before
    the members' ``step()``.  ``max_norm``: clip the group's global L2 norm (None: measure only); ``skip_nonfinite``: a step whose
    norm is not finite is not applied by any member.  The norm is that of the gradient Adam consumes: ``grad_scale * sqrt(sum g^2)``."""

    def __init__(self, optimizers, max_norm=None, skip_nonfinite=False):
        self.optimizers = list(optimizers)
        if not 1 <= len(self.optimizers) <= 4:
            raise ValueError('a step group has 1 to 4 optimisers, got %d' % len(self.optimizers))
        if max_norm is not None and not float(max_norm) > 0:
            raise ValueError('max_norm must be a positive number or None, got %r' % (max_norm,))
        self.max_norm = None if max_norm is None else float(max_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        dev = self.optimizers[0].flat_param.device
        self.partials = [torch.zeros(ops.grad_sumsq_partials(), device=dev, dtype=torch.float64) for _ in self.optimizers]
        self.record = torch.zeros(ops.GUARD_WORDS, device=dev, dtype=torch.int64)
        self._armed = set()
        for opt in self.optimizers:
            if opt.guard is not None:
                raise ValueError('optimiser already belongs to a step group')
            opt.guard = self

    def prepare(self):
        """norm -> record, on the current stream; every member's next ``step()`` consumes it"""
        scales = {float(opt.grad_scale) for opt in self.optimizers}
        if len(scales) != 1:
            raise RuntimeError('the optimisers of a step group must share one grad_scale, got %s' % sorted(scales))
        ops.join_side_stream()  # weight-gradient kernels may still be running on the side stream
        for opt, part in zip(self.optimizers, self.partials):
            ops.grad_sumsq(opt.flat_grad, part)
        ops.optim_guard_prep(self.partials, self.record, scales.pop(), self.max_norm or 0.0, self.skip_nonfinite)
        self._armed = {id(opt) for opt in self.optimizers}

    def consume(self, opt):
        if id(opt) not in self._armed:
            raise RuntimeError('StepGuard.prepare() must run before every step() of its optimisers (the record is stale)')
        self._armed.discard(id(opt))

    # device scalars (views of the record: read them on log steps only)
    def norm(self):
        """pre-clip gradient norm of the last prepared step, 0-d float64 device tensor"""
        return self.record.view(torch.float64)[0]

    def skipped(self):
        """number of steps skipped so far, 0-d int64 device tensor"""
        return self.record[2]


def _static_record(dev, grad_scale):
    """a guard record that never skips and scales by ``grad_scale`` (EMA without a StepGuard)"""
    words = struct.unpack('<4q', struct.pack('<dfiqq', 0.0, float(grad_scale), 0, 0, 0))
    return torch.tensor(words, dtype=torch.int64, device=dev)


def _physical_perm(t):
    return sorted(range(t.dim()), key=lambda d: (-t.stride(d), d))


class FlatAdam:
    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError('optimizer got an empty parameter list')
        dev = self.params[0].device
        if dev.type != 'cuda':
            raise RuntimeError('FlatAdam runs on the GPU only')
        self.offsets, total = [], 0
        for p in self.params:
            self.offsets.append(total)
            total += (p.numel() + 3) // 4 * 4  # keep every tensor 16-byte aligned inside the flat buffers
        self.flat_param = torch.zeros(total, device=dev, dtype=torch.float32)
        self.flat_grad = torch.zeros_like(self.flat_param)
        self.exp_avg = torch.zeros_like(self.flat_param)
        self.exp_avg_sq = torch.zeros_like(self.flat_param)
        self._perms = []
        for p, off in zip(self.params, self.offsets):
            perm = _physical_perm(p.data)
            phys = p.data.permute(perm)
            if not phys.is_contiguous():
                raise RuntimeError('parameter is not dense in memory')
            inv = [perm.index(d) for d in range(p.dim())]
            view = self.flat_param[off:off + p.numel()].view(phys.shape)
            view.copy_(phys)
            p.data = view.permute(inv)
            gview = self.flat_grad[off:off + p.numel()].view(phys.shape).permute(inv)
            if p.grad is not None:
                gview.copy_(p.grad)
            p.grad = gview
            self._perms.append((perm, inv, tuple(phys.shape)))
        self.param_groups = [dict(params=self.params, lr=float(lr), betas=tuple(betas), eps=float(eps),
                                  weight_decay=float(weight_decay))]
        self.lr_dev = torch.tensor([float(lr)], device=dev, dtype=torch.float32)
        self._lr_host = float(lr)
        self.state_dev = torch.zeros(2, device=dev, dtype=torch.int64)  # {int64 step; float bc1; float bc2_sqrt}
        self.grad_scale = 1.0
        self.guard = None  # StepGuard of this optimiser's step group (gradient clipping / non-finite step skip), set by StepGuard
        self.ema, self.ema_decay = None, None  # flat EMA copy of flat_param (enable_ema)
        self._static = None  # (record, grad_scale) for an EMA step without a guard
        self.mirrors = ops.WeightMirrors(self.params)  # transposed conv weights for the input-gradient kernels

    # -- torch.optim.Optimizer surface used by the reference -------------------------------------------
    def zero_grad(self, set_to_none=False):
        self.flat_grad.zero_()

    def sync_lr(self):
        lr = float(self.param_groups[0]['lr'])
        if lr != self._lr_host:  # MultiStepLR edits param_groups between epochs (trainer.py:396-398)
            self.lr_dev.fill_(lr)
            self._lr_host = lr

    def step(self):
        g = self.param_groups[0]
        ops.join_side_stream()  # weight-gradient kernels may still be running on the side stream (ops.OVERLAP_DW)
        self.sync_lr()
        if self.guard is None and self.ema is None:
            ops.adam_step(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.lr_dev, self.state_dev,
                          g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'], self.grad_scale)
        else:
            if self.guard is not None:
                self.guard.consume(self)
                record = self.guard.record
            else:
                if self._static is None or self._static[1] != float(self.grad_scale):
                    self._static = (_static_record(self.flat_param.device, self.grad_scale), float(self.grad_scale))
                record = self._static[0]
            ops.adam_step_guarded(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.lr_dev, self.state_dev, record,
                                  g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'], self.ema, self.ema_decay or 0.0)
        self.mirrors.mark_dirty()  # the next backward pass refreshes all mirrors in one launch

    # -- exponential moving average of the parameters ---------------------------------------------------
    def enable_ema(self, decay):
        """Keep ``ema = decay * ema + (1 - decay) * p`` after every applied step, starting from the current parameters."""
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError('EMA decay must lie in (0, 1), got %r' % (decay,))
        self.ema_decay = decay
        self.ema = self.flat_param.detach().clone()
        # (built here, not in step(): a host-to-device copy cannot be part of a hipGraph capture)
        self._static = (_static_record(self.flat_param.device, self.grad_scale), float(self.grad_scale))
        return self

    def ema_state(self):
        """the EMA of every parameter, in ``self.params`` order and in the parameters' logical shapes (copies)"""
        if self.ema is None:
            raise RuntimeError('this optimiser keeps no EMA (enable_ema)')
        return [self._per_param(self.ema, i).clone().contiguous() for i in range(len(self.params))]

    def load_ema_state(self, tensors):
        if self.ema is None:
            raise RuntimeError('this optimiser keeps no EMA (enable_ema)')
        tensors = list(tensors)
        if len(tensors) != len(self.params):
            raise ValueError('expected %d EMA tensors, got %d' % (len(self.params), len(tensors)))
        for i, t in enumerate(tensors):
            self._per_param(self.ema, i).copy_(t)

    def swap_ema(self):
        """Exchange the contents of the parameter buffer and the EMA buffer, bit for bit (a second call swaps back)."""
        if self.ema is None:
            raise RuntimeError('this optimiser keeps no EMA (enable_ema)')
        with torch.no_grad():
            tmp = self.flat_param.clone()
            self.flat_param.copy_(self.ema)
            self.ema.copy_(tmp)
        self.mirrors.mark_dirty()

    def _per_param(self, flat, i):
        p, off = self.params[i], self.offsets[i]
        perm, inv, shape = self._perms[i]
        return flat[off:off + p.numel()].view(shape).permute(inv)

    def state_dict(self):
        """torch.optim.Adam-compatible layout (the reference checkpoints '<name>_state_dict', trainer.py:318-319)."""
        step = int(self.state_dev[0].item())
        state = {}
        if step > 0:
            for i in range(len(self.params)):
                state[i] = {'step': torch.tensor(float(step)), 'exp_avg': self._per_param(self.exp_avg, i).clone(),
                            'exp_avg_sq': self._per_param(self.exp_avg_sq, i).clone()}
        g = dict(self.param_groups[0])
        g['params'] = list(range(len(self.params)))
        g.update(amsgrad=False, maximize=False)
        return {'state': state, 'param_groups': [g]}

    def load_state_dict(self, sd):
        g = sd['param_groups'][0]
        for k in ('lr', 'betas', 'eps', 'weight_decay', 'initial_lr'):  # 'initial_lr' is what an lr scheduler left there
            if k in g:
                self.param_groups[0][k] = g[k]
        step = 0
        for i, st in sd['state'].items():
            i = int(i)
            self._per_param(self.exp_avg, i).copy_(st['exp_avg'])
            self._per_param(self.exp_avg_sq, i).copy_(st['exp_avg_sq'])
            step = int(st['step']) if not torch.is_tensor(st['step']) else int(st['step'].item())
        self.state_dev.zero_()
        self.state_dev[0] = step
        self.sync_lr()
