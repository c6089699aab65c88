"""Fit a template code to a clip with the generator held fixed (TEST.FIT_CODE, DEMO.CODE_PATH; csrc/code_fit.hip).

The audio encoder does not depend on the code: it runs once per batch.  An iteration of the fit is the Conv1d stage forward and backward plus the
head (the kernels the train step runs), and around them four kernels of this module: the per-clip L1 loss and its gradient, the per-clip Adam step
on the (B, D) codes that also keeps the best iterate and writes the next code straight into the chain's input buffer, the write of given codes into
that buffer, and the per-clip choice among candidate codes.  Nothing is read back by the host inside the loop.

``loss_model`` / ``step_model`` / ``set_model`` / ``pick_model`` are the kernels' contracts in numpy, operation by operation; ``loop_model`` is the
whole loop in float64 torch over any generator tail given as a function (the tests hand it the oracle's).

Command line (one clip, on the GPU):
    python -m speechdrivestemplates_amd.code_fit --config CFG.yaml --checkpoint X.pth --clip CLIP.npz --out code.npz [--steps S] [--lr LR]
                                                 [--init zero|mean|table] [--candidates M] [--prior L]
"""
import math

import numpy as np

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8  # torch.optim.Adam's defaults, as everywhere in this package
MAX_D = 256  # csrc/code_fit.hip CODE_FIT_MAX_D
INITS = ('zero', 'mean', 'table')
_NO_GPU = 'speechdrivestemplates_amd.code_fit runs on the GPU only (no CPU fallback); the numpy models in this module are test infrastructure'


# ---- contract models (numpy) -------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """float32(a * b + c) with ONE rounding, elementwise on float32 arrays: the product of two floats is exact in float64, the float64 sum is
    rounded to odd (TwoSum gives its error), and a 53-bit round-to-odd value rounds to 24 bits as the exact one does"""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all='ignore'):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def _butterfly(v):
    """the xor butterfly of wave_sum_d over the last axis (64 lanes): every lane ends with the same bits"""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v


def loss_model(pred, gt):
    """sdt_code_fit_loss_f32: pred, gt (B, n) float32 -> (loss (B,) float64, dpred (B, n) float32), in the kernel's summation order"""
    pred, gt = np.asarray(pred, dtype=np.float32), np.asarray(gt, dtype=np.float32)
    B, n = pred.shape
    with np.errstate(all='ignore'):
        e = pred.astype(np.float64) - gt.astype(np.float64)
        inv = np.float32(1.0 / float(n))
        dpred = np.where(e > 0, inv, np.where(e < 0, -inv, np.where(e == 0, np.float32(0), np.float32(np.nan)))).astype(np.float32)
        rows = -(-n // 256)
        a = np.zeros((B, rows * 256), dtype=np.float64)  # (a padding +0.0 added to a sum that is >= +0 or NaN changes no bit)
        a[:, :n] = np.abs(e)
        a = a.reshape(B, rows, 256)
        acc = np.zeros((B, 256), dtype=np.float64)
        for r in range(rows):
            acc = acc + a[:, r]
        w = _butterfly(acc.reshape(B, 4, 64))[:, :, 0]
        s = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
        loss = np.where(np.isfinite(s), s / float(n), np.nan)
    return loss, dpred


def new_state(code, history_rows):
    """the device state of a fit as numpy arrays: code (B, D) float32 -> dict"""
    code = np.array(code, dtype=np.float32)
    B, D = code.shape
    return {'code': code, 'm': np.zeros((B, D), np.float32), 'v': np.zeros((B, D), np.float32), 'best_code': np.zeros((B, D), np.float32),
            'best_loss': np.full(B, np.inf), 'counter': 0, 'history': np.full((history_rows, B), np.nan), 'nonfinite': np.zeros(B, np.int32)}


def bias_corrections(step, beta1=BETA1, beta2=BETA2):
    """(bc1, bc2_sqrt) as adam_prep_kernel computes them: float64 pow of the float32 betas, rounded once to float32"""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    return np.float32(1.0 - math.pow(b1, float(step))), np.float32(math.sqrt(1.0 - math.pow(b2, float(step))))


def adam_model(p, g, m, v, lr, step, beta1=BETA1, beta2=BETA2, eps=EPS):
    """one Adam update of float32 arrays as the step kernel (and adam_kernel's vector path, weight_decay 0, grad_scale 1) evaluates it
    -> (p, m, v)"""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    bc1, bc2s = bias_corrections(step, beta1, beta2)
    with np.errstate(all='ignore'):
        step_size = f(lr) / bc1
        om1, om2 = f(1) - f(beta1), f(1) - f(beta2)
        mm = fma32(m, f(beta1), om1 * g)
        vv = fma32(v, f(beta2), (om2 * g) * g)
        denom = np.sqrt(vv) / bc2s + f(eps)
        return fma32(-step_size, mm / denom, p), mm, vv


def step_model(st, dh, loss, h, C, lr, lam=0.0, mu=None, ivar=None, mode=0):
    """sdt_code_fit_step_f32 on the state ``st`` (new_state), in place: dh, h (B, T, C + D) float32, loss (B,) float64"""
    f = np.float32
    B, D = st['code'].shape
    loss = np.asarray(loss, dtype=np.float64)
    with np.errstate(all='ignore'):
        better = loss < st['best_loss']
        st['best_code'][better] = st['code'][better]
        st['best_loss'][better] = loss[better]
        it = st['counter']
        if 0 <= it < st['history'].shape[0]:
            st['history'][it] = loss
        if mode != 0:
            return st
        T = dh.shape[1]
        s = np.zeros((B, D), dtype=np.float64)
        for t in range(T):
            s = s + np.asarray(dh[:, t, C:], dtype=f).astype(np.float64)
        g = s.astype(f)
        if lam > 0:
            g = (g.astype(np.float64) + ((lam * (st['code'].astype(np.float64) - mu)) * ivar) / float(D)).astype(f)
        ok = np.isfinite(loss) & np.isfinite(g).all(axis=1)
        p, mm, vv = adam_model(st['code'], g, st['m'], st['v'], lr, it + 1)
        st['code'][ok], st['m'][ok], st['v'][ok] = p[ok], mm[ok], vv[ok]
        st['nonfinite'][~ok] = 1
        h[:, :, C:] = st['code'][:, None, :]
        st['counter'] = it + 1
    return st


def set_model(codes, h, C):
    """sdt_code_fit_set_f32, in place on h (B, T, C + D)"""
    h[:, :, C:] = np.asarray(codes, dtype=np.float32)[:, None, :]
    return h


def pick_model(cand_loss, cands=None):
    """sdt_code_fit_pick_f32: cand_loss (M, B) float64 -> (index (B,) int32, best (B,) float64[, codes (B, D)])"""
    cand_loss = np.asarray(cand_loss, dtype=np.float64)
    M, B = cand_loss.shape
    index, best = np.full(B, -1, np.int32), np.full(B, np.nan)
    for b in range(B):
        for j in range(M):
            l = cand_loss[j, b]
            if np.isfinite(l) and (index[b] < 0 or l < best[b]):
                index[b], best[b] = j, l
    if cands is None:
        return index, best
    return index, best, np.asarray(cands, dtype=np.float32)[np.maximum(index, 0)]


def candidate_rows(num_rows, candidates):
    """the table rows INIT 'table' tries: floor(j * N / M), j = 0 .. M - 1"""
    if num_rows < 1 or candidates < 1:
        raise ValueError('candidate_rows needs at least one table row and one candidate, got N = %r, M = %r' % (num_rows, candidates))
    return [(j * num_rows) // candidates for j in range(candidates)]


def table_stats_model(table):
    """(mean float32 (D,), mu float64 (D,), ivar float64 (D,)) of table rows (N, D): the float64 mean, 1 / unbiased variance (0 where the
    variance is 0 or there is one row)"""
    t = np.asarray(table, dtype=np.float64)
    mu = t.mean(axis=0)
    var = t.var(axis=0, ddof=1) if t.shape[0] > 1 else np.zeros(t.shape[1])
    with np.errstate(all='ignore'):
        ivar = np.where(var > 0, 1.0 / var, 0.0)
    return mu.astype(np.float32), mu, ivar


def loop_model(tail, gt, code0, steps, lr, lam=0.0, mu=None, ivar=None):
    """The whole fit in float64 torch (CPU): ``tail(code (B, D)) -> pred (B, n)`` is the generator behind the audio encoder, differentiable and
    independent per clip; gt (B, n).  Plain Adam (0.9, 0.999, 1e-8) per clip on loss_b = mean |pred_b - gt_b| + lam * mean_d((c - mu)^2 ivar) / 2,
    the best iterate by the data loss kept, one more evaluation for the last code.
    -> {'code', 'loss_first', 'loss_best', 'history' (steps + 1, B), 'grads' [steps x (B, D)], 'codes' [steps + 1 x (B, D)], 'min_abs_diff'}"""
    import torch
    gt = gt.double()
    code = code0.double().clone()
    B, D = code.shape
    m, v = torch.zeros_like(code), torch.zeros_like(code)
    best_code, best_loss = code.clone(), torch.full((B,), float('inf'), dtype=torch.float64)
    history, grads, codes, min_abs = [], [], [code.clone()], float('inf')
    for it in range(steps + 1):
        c = code.clone().requires_grad_(it < steps)
        with torch.enable_grad():
            diff = tail(c) - gt
            loss = diff.abs().mean(dim=1)
            if it < steps:
                total = loss.sum()
                if lam > 0:
                    total = total + (lam * 0.5 / D) * (((c - mu) ** 2) * ivar).sum()
                (g,) = torch.autograd.grad(total, c)
        min_abs = min(min_abs, float(diff.detach().abs().min()))
        loss = loss.detach()
        better = loss < best_loss
        best_code[better], best_loss[better] = code[better], loss[better]
        history.append(loss.clone())
        if it == steps:
            break
        grads.append(g.clone())
        m = BETA1 * m + (1 - BETA1) * g
        v = BETA2 * v + (1 - BETA2) * g * g
        denom = v.sqrt() / math.sqrt(1 - BETA2 ** (it + 1)) + EPS
        code = code - (lr / (1 - BETA1 ** (it + 1))) * (m / denom)
        codes.append(code.clone())
    history = torch.stack(history)
    return {'code': best_code, 'loss_first': history[0], 'loss_best': best_loss, 'history': history, 'grads': grads, 'codes': codes,
            'min_abs_diff': min_abs}


# ---- kernel wrappers ---------------------------------------------------------------------------------------------------------------------------
def _ops():
    from . import _lib, ops
    return _lib.load(), ops, _lib.check


def clip_loss(pred, gt, loss=None, dpred=None):
    """pred, gt (B, ...) fp32 on the GPU -> (loss (B,) float64, dpred like pred): one launch, one workgroup per clip"""
    import torch
    lib, ops, check = _ops()
    ops._req_cuda(pred, gt)
    pred, gt = pred.contiguous(), gt.contiguous()
    if pred.dtype != torch.float32 or gt.dtype != torch.float32 or pred.shape != gt.shape or pred.dim() < 2:
        raise ValueError('clip_loss takes two fp32 tensors (B, ...) of one shape, got %s %s and %s %s'
                         % (tuple(pred.shape), pred.dtype, tuple(gt.shape), gt.dtype))
    B = pred.shape[0]
    loss = torch.empty(B, device=pred.device, dtype=torch.float64) if loss is None else loss
    dpred = torch.empty_like(pred) if dpred is None else dpred
    assert loss.dtype == torch.float64 and loss.numel() == B and loss.is_contiguous() and dpred.is_contiguous() and dpred.shape == pred.shape
    check(lib.sdt_code_fit_loss_f32(ops._p(pred), ops._p(gt), B, pred.numel() // B, ops._p(loss), ops._p(dpred), ops._stream()))
    return loss, dpred


def set_codes(codes, h, C):
    """h[b, t, C + d] = codes[b, d] on the GPU, in place"""
    import torch
    lib, ops, check = _ops()
    ops._req_cuda(codes, h)
    B, T, W = h.shape
    D = W - C
    if not (codes.dtype == h.dtype == torch.float32 and h.is_contiguous() and tuple(codes.shape) == (B, D) and D >= 1):
        raise ValueError('set_codes: codes %s do not fit the code channels of h %s behind %d feature channels' % (tuple(codes.shape), tuple(h.shape), C))
    check(lib.sdt_code_fit_set_f32(ops._p(codes.contiguous()), ops._p(h), B, T, C, D, ops._stream()))
    return h


def pick(cand_loss, cands=None):
    """cand_loss (M, B) float64 on the GPU -> (index (B,) int32, best (B,) float64, codes (B, D) or None)"""
    import torch
    lib, ops, check = _ops()
    ops._req_cuda(cand_loss, cands)
    cand_loss = cand_loss.contiguous()
    if cand_loss.dtype != torch.float64 or cand_loss.dim() != 2:
        raise ValueError('pick takes candidate losses (M, B) in float64, got %s %s' % (tuple(cand_loss.shape), cand_loss.dtype))
    M, B = cand_loss.shape
    index = torch.empty(B, device=cand_loss.device, dtype=torch.int32)
    best = torch.empty(B, device=cand_loss.device, dtype=torch.float64)
    out, D = None, 0
    if cands is not None:
        if cands.dtype != torch.float32 or cands.dim() != 2 or cands.shape[0] != M:
            raise ValueError('pick takes one fp32 candidate code per row of the losses, got %s for M = %d' % (tuple(cands.shape), M))
        cands, D = cands.contiguous(), cands.shape[1]
        out = torch.empty((B, D), device=cand_loss.device, dtype=torch.float32)
    check(lib.sdt_code_fit_pick_f32(ops._p(cand_loss), M, B, ops._p(cands), D, ops._p(index), ops._p(best), ops._p(out), ops._stream()))
    return index, best, out


class FitState:
    """the device state of one fit: codes, moments, best iterate, counter, learning rate, history and flags -- everything the step kernel
    reads and writes, so that no decision of the loop needs the host"""

    def __init__(self, code, history_rows, lr, lam=0.0, mu=None, ivar=None):
        import torch
        dev = code.device
        B, D = code.shape
        if D > MAX_D:
            raise ValueError('the code-fit step holds at most %d code dimensions, got %d' % (MAX_D, D))
        self.B, self.D, self.rows = B, D, int(history_rows)
        self.code = code.detach().clone().contiguous()
        self.m, self.v = torch.zeros_like(self.code), torch.zeros_like(self.code)
        self.best_code = torch.zeros_like(self.code)
        self.best_loss = torch.full((B,), float('inf'), device=dev, dtype=torch.float64)
        self.counter = torch.zeros(1, device=dev, dtype=torch.int64)
        self.lr = torch.full((1,), float(lr), device=dev, dtype=torch.float32)
        self.history = torch.full((self.rows, B), float('nan'), device=dev, dtype=torch.float64)
        self.nonfinite = torch.zeros(B, device=dev, dtype=torch.int32)
        self.lam = float(lam)
        self.mu = None if mu is None else mu.to(dev, torch.float64).contiguous()
        self.ivar = None if ivar is None else ivar.to(dev, torch.float64).contiguous()

    def step(self, dh, loss, h, C, mode=0):
        """one call of sdt_code_fit_step_f32: dh (B, T, C + D) the chain's input gradient (None with mode 1), loss (B,) float64, h the chain's
        input buffer, written in place"""
        lib, ops, check = _ops()
        if mode == 0:
            ops._req_cuda(dh, loss, h)
            dh = dh.contiguous()
            if tuple(dh.shape) != tuple(h.shape) or h.shape[0] != self.B or h.shape[2] != C + self.D or not h.is_contiguous():
                raise ValueError('the step needs dh and h of one shape (B, T, C + D), got %s and %s' % (tuple(dh.shape), tuple(h.shape)))
        T = h.shape[1] if h is not None else 1
        check(lib.sdt_code_fit_step_f32(ops._p(dh), ops._p(loss), ops._p(self.code), ops._p(self.m), ops._p(self.v), ops._p(self.best_code),
                                        ops._p(self.best_loss), ops._p(self.counter), ops._p(self.lr), ops._p(self.mu), ops._p(self.ivar),
                                        self.lam, BETA1, BETA2, EPS, ops._p(h), self.B, T, C, self.D, ops._p(self.history), self.rows,
                                        ops._p(self.nonfinite), mode, ops._stream()))


# ---- the fit -----------------------------------------------------------------------------------------------------------------------------------
def fit_opts(steps=100, lr=0.05, init='mean', candidates=0, prior=0.0):
    return {'steps': int(steps), 'lr': float(lr), 'init': init, 'candidates': int(candidates), 'prior': float(prior)}


class CodeFitter:
    """``fit`` finds, per clip of a batch, the code under which ``model`` (a Voice2PoseModel with a code table) explains the clip best.
    ``opts``: config.check_fit_code's dict (fit_opts).  The model's weights are constants of the fit: their requires_grad flags are lowered
    for its duration -- no weight gradient is launched, no ``.grad`` is touched -- and restored with the modules' training modes."""

    def __init__(self, model, opts):
        self.model, self.opts = model, dict(opts)
        if model.clips_code is None:
            raise ValueError('TEST.FIT_CODE needs VOICE2POSE.GENERATOR.CLIP_CODE.DIMENSION: this generator takes no code')
        if self.opts['init'] not in INITS:
            raise ValueError('TEST.FIT_CODE.INIT must be one of %s, got %r' % (', '.join(INITS), self.opts['init']))

    def table_rows(self, dev):
        """the rows the start code and the prior come from: the first num_clips rows of the table (the unmirrored clips' codes)"""
        table = self.model._code_table(dev).detach()
        n = table.size(0) if self.model.num_clips is None else min(int(self.model.num_clips), table.size(0))
        return table[:n]

    def table_stats(self, dev):
        """(mean (D,) fp32, mu (D,) float64, ivar (D,) float64) on the device; set-up work, outside the loop"""
        import torch
        rows = self.table_rows(dev).double()
        mu = rows.mean(dim=0)
        var = rows.var(dim=0, unbiased=True) if rows.shape[0] > 1 else torch.zeros_like(mu)
        ivar = torch.where(var > 0, 1.0 / var, torch.zeros_like(var))
        return mu.float(), mu, ivar

    def fit(self, audio, poses_gt, num_frames):
        """audio (B, L), poses_gt (B, T, 2, K) normalised, num_frames = T -> {'code' (B, D), 'loss_first', 'loss_best' (B,) float64,
        'history' (STEPS + 1, B) float64 (row STEPS: the last code), 'nonfinite' (B,) int32, 'poses_pred' (B, T, 2, K); with INIT 'table'
        also 'loss_table' (B,) float64 (the best of the tried table rows) and 'start_index' (B,) int32 (0: the mean, 1 + j: candidate j)};
        all on the device, nothing is read back"""
        import torch
        model = self.model
        params = list(model.parameters())
        flags = [p.requires_grad for p in params]
        modes = [(mod, mod.training) for mod in model.modules()]
        try:
            model.eval()
            for p in params:
                p.requires_grad_(False)
            with torch.enable_grad():
                return self._fit(audio, poses_gt, int(num_frames))
        finally:
            for p, f in zip(params, flags):
                p.requires_grad_(f)
            for mod, training in modes:
                mod.training = training

    def _fit(self, audio, poses_gt, T):
        import torch
        from . import ops
        model, o = self.model, self.opts
        netG, dev = model.netG, model._device()
        audio = audio.to(dev, non_blocking=True)
        gt = poses_gt.to(dev, non_blocking=True).float().contiguous()
        B, S = gt.shape[0], o['steps']
        if gt.shape[1] != T:
            raise ValueError('CodeFitter.fit: poses_gt has %d frames, num_frames is %d' % (gt.shape[1], T))
        mean, mu, ivar = self.table_stats(dev)
        D = mean.shape[0]
        with torch.no_grad():
            feat = netG.audio_encoder.encode_cl(model.mel_transfm(audio))
            start = torch.zeros((B, D), device=dev, dtype=torch.float32) if o['init'] == 'zero' else mean.expand(B, D).contiguous()
            h = ops.ResizeConcatFn.apply(feat, start, T)  # (B, T, C + D): the resize runs once, the loop rewrites the code channels only
            C = h.shape[2] - D
            gt2 = gt.reshape(B, T, -1)
            out = {}
            if o['init'] == 'table':
                rows = self.table_rows(dev)
                cands = torch.cat([mean[None], rows[candidate_rows(rows.shape[0], o['candidates'])]]).contiguous()
                cand_loss = torch.empty((cands.shape[0], B), device=dev, dtype=torch.float64)
                dpred = torch.empty_like(gt2)
                for j in range(cands.shape[0]):
                    set_codes(cands[j:j + 1].expand(B, D), h, C)
                    clip_loss(netG.forward_tail(h), gt2, cand_loss[j], dpred)
                out['start_index'], _, start = pick(cand_loss, cands)
                _, out['loss_table'], _ = pick(cand_loss[1:])
                set_codes(start, h, C)
        st = FitState(start, S + 1, o['lr'], o['prior'], mu, ivar)
        h.requires_grad_(True)
        loss = torch.empty(B, device=dev, dtype=torch.float64)
        for _ in range(S):
            y = netG.forward_tail(h)
            _, dpred = clip_loss(y.detach(), gt2, loss)
            (dh,) = torch.autograd.grad(y, h, dpred)
            st.step(dh, loss, h.detach(), C)
        with torch.no_grad():
            hd = h.detach()
            clip_loss(netG.forward_tail(hd), gt2, loss)
            st.step(None, loss, hd, C, mode=1)
            set_codes(st.best_code, hd, C)
            pred = netG.forward_tail(hd).reshape(B, T, 2, -1)
        out.update(code=st.best_code, loss_first=st.history[0].clone(), loss_best=st.best_loss, history=st.history, nonfinite=st.nonfinite,
                   poses_pred=pred)
        return out

    def code_z(self, code):
        """mean over the batch and the dimensions of |code - mu| * sqrt(ivar): how far fitted codes sit from the trained table"""
        _, mu, ivar = self.table_stats(code.device)
        return ((code.double() - mu).abs() * ivar.sqrt()).mean()


# ---- DEMO.CODE_PATH ----------------------------------------------------------------------------------------------------------------------------
def load_code_vector(path, dim):
    """the code of an npz written by this module's command line (or by hand): 'v' of shape (1, D) or (D,) -> float32 (1, D); ValueError
    names DEMO.CODE_PATH"""
    with np.load(path) as z:
        if 'v' not in z.files:
            raise ValueError("DEMO.CODE_PATH %r has no array 'v' (it holds %s)" % (path, ', '.join(z.files) or 'nothing'))
        v = np.asarray(z['v'])
    if v.ndim == 1:
        v = v[None]
    if v.ndim != 2 or v.shape[0] != 1:
        raise ValueError("DEMO.CODE_PATH %r: 'v' must have the shape (1, D) or (D,), got %s" % (path, tuple(np.asarray(v).shape)))
    if v.shape[1] != dim:
        raise ValueError("DEMO.CODE_PATH %r: 'v' has %d dimensions, VOICE2POSE.GENERATOR.CLIP_CODE.DIMENSION is %r" % (path, v.shape[1], dim))
    if not np.isfinite(v.astype(np.float64)).all():
        raise ValueError("DEMO.CODE_PATH %r: 'v' holds a non-finite number" % (path,))
    return np.ascontiguousarray(v, dtype=np.float32)


def demo_code(cfg):
    """None, or the (1, D) float32 vector a Voice2Pose demo is conditioned on (DEMO.CODE_PATH); ValueError names the key"""
    path = cfg.DEMO.CODE_PATH
    if path is None or cfg.PIPELINE_TYPE != 'Voice2Pose':
        return None
    dim = cfg.VOICE2POSE.GENERATOR.CLIP_CODE.DIMENSION
    if dim is None:  # a generator without codes never read the key: it still does not
        return None
    if cfg.DEMO.CODE_INDEX is not None:
        raise ValueError('DEMO.CODE_PATH and DEMO.CODE_INDEX both name the code of the demo: set one of them')
    return load_code_vector(path, dim)


# ---- command line ------------------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m speechdrivestemplates_amd.code_fit',
                                 description='fit a template code to one clip with the generator of a checkpoint held fixed (on the GPU)')
    ap.add_argument('--config', required=True, metavar='CFG.yaml')
    ap.add_argument('--checkpoint', required=True, metavar='X.pth')
    ap.add_argument('--clip', required=True, metavar='CLIP.npz', help="a clip of the data set's format: 'pose' (>= NUM_FRAMES, 3, 137) and 'audio'")
    ap.add_argument('--out', required=True, metavar='code.npz', help='v (1, D), history, loss_first, loss_best, loss_table')
    ap.add_argument('--steps', type=int, default=None, metavar='S')
    ap.add_argument('--lr', type=float, default=None, metavar='LR')
    ap.add_argument('--init', choices=INITS, default=None)
    ap.add_argument('--candidates', type=int, default=None, metavar='M')
    ap.add_argument('--prior', type=float, default=None, metavar='L')
    ap.add_argument('opts', nargs='*', metavar='KEY VAL', help='further configuration overrides, as for main.py')
    a = ap.parse_args(argv)
    if len(a.opts) % 2:
        ap.error('configuration overrides come as KEY VAL pairs')
    return a


def cfg_from_args(a):
    """the frozen configuration of a command-line fit: file <- KEY VAL pairs <- the fit's own flags, TEST.FIT_CODE.ENABLE on"""
    from .config import check_fit_code, get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(a.config)
    over = list(a.opts) + ['TEST.FIT_CODE.ENABLE', True]
    for key, val in (('STEPS', a.steps), ('LR', a.lr), ('INIT', a.init), ('CANDIDATES', a.candidates), ('PRIOR', a.prior)):
        if val is not None:
            over += ['TEST.FIT_CODE.' + key, val]
    cfg.merge_from_list(over)
    cfg.freeze()
    return cfg, check_fit_code(cfg)


def prepare_clip(cfg, path):
    """a clip npz -> (audio (1, L) float32, poses (1, T, 2, 121) normalised float32, T): what GestureDataset.__getitem__ makes of it"""
    import torch
    from .core.datasets.gesture_dataset import GestureDataset, crop_pad_audio, parse_audio_length, register_configured_speaker_stats
    register_configured_speaker_stats(cfg)
    ds = GestureDataset(root_dir=None, speaker=cfg.DATASET.SPEAKER, cfg=cfg)
    with np.load(path) as z:
        pose, audio = np.asarray(z['pose']), np.asarray(z['audio'])
    length, T = parse_audio_length(cfg.DATASET.AUDIO_LENGTH, cfg.DATASET.AUDIO_SR, cfg.DATASET.FPS)
    if pose.ndim != 3 or pose.shape[0] < cfg.DATASET.NUM_FRAMES or pose.shape[1:] != (3, 137):
        raise ValueError("--clip: 'pose' must be (>= %d, 3, 137), got %s" % (cfg.DATASET.NUM_FRAMES, pose.shape))
    p = ds.absolute_to_relative(ds.remove_unuesd_kp(torch.Tensor(pose[:cfg.DATASET.NUM_FRAMES])))
    if cfg.DATASET.HIERARCHICAL_POSE:
        p = ds.global_to_parted(p)
    stat = ds.get_speaker_stat(cfg.DATASET.SPEAKER, 121, parted=cfg.DATASET.HIERARCHICAL_POSE)
    poses = ds.normalize_poses(p[:, :2, :], stat)
    audio = crop_pad_audio(audio.astype(np.float32).reshape(-1), length)
    return torch.from_numpy(np.ascontiguousarray(audio))[None], torch.as_tensor(poses, dtype=torch.float32)[None], T


def main(argv=None):
    a = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    from .core.pipelines import get_pipeline
    cfg, opts = cfg_from_args(a)
    ckpt = torch.load(a.checkpoint, map_location='cpu')
    pipe = get_pipeline(cfg.PIPELINE_TYPE)(cfg)
    pipe.setup_model(cfg, state_dict=ckpt['model_state_dict'])
    pipe.model.eval()
    audio, poses, T = prepare_clip(cfg, a.clip)
    res = CodeFitter(pipe.model, opts).fit(audio, poses, T)
    first, best = float(res['loss_first'][0]), float(res['loss_best'][0])
    table = float(res['loss_table'][0]) if 'loss_table' in res else float('nan')
    print('code_fit: loss_first %.6f  loss_best %.6f  loss_table %.6f  steps %d  nonfinite %d'
          % (first, best, table, opts['steps'], int(res['nonfinite'][0])))
    np.savez(a.out, v=res['code'].cpu().numpy(), history=res['history'][:, 0].cpu().numpy(), loss_first=np.float64(first),
             loss_best=np.float64(best), loss_table=np.float64(table))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
