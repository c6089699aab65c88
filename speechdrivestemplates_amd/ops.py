"""Host-side wrappers of the libsdt_hip.so kernels: geometry builders (pure Python), thin launchers that
marshal raw device pointers + the current HIP stream, and the ``torch.autograd.Function`` glue that lets
the reference-shaped ``nn.Module``s in ``core.networks`` train through the hand-written kernels.

Conventions
  * activations are channels-last contiguous fp32: (B,H,W,C) / (B,T,C);
  * conv weights keep the reference's logical shape (Cout,Cin,kh,kw) / (Cout,Cin,k) as a strided view of
    (Cout,taps,Cin) storage (``weight_storage`` returns that storage, copying only if the layout is foreign);
  * parameter gradients are ACCUMULATED by the kernels straight into ``param.grad`` (created zero-filled when
    absent) -- the autograd functions return None for parameters.  This is what lets a pipeline place all
    parameters / gradients in two flat buffers (one fused Adam launch, one all-reduce).
There is no CPU or eager-PyTorch fallback: a non-CUDA tensor raises.
"""
import functools
import math
import os

import torch

from . import _lib
from ._lib import ConvGeom, check

LEAKY_SLOPE = 0.2  # building_blocks.py:46
BN_EPS, BN_MOMENTUM = 1e-5, 0.1  # nn.BatchNorm / nn.InstanceNorm defaults used at building_blocks.py:24-26,39-41


# --------------------------------------------------------------------------------------------
# geometry (host only; validated on CPU against F.conv2d by tests/test_geometry.py)
# --------------------------------------------------------------------------------------------
def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def _geom(**kw):
    g = ConvGeom()
    taps = kw.pop("taps")
    for k, v in kw.items():
        setattr(g, k, int(v))
    g.ntaps = len(taps)
    assert 0 < g.ntaps <= _lib.MAX_TAPS, "kernel has too many taps (%d)" % g.ntaps
    for i, (dy, dx, wt) in enumerate(taps):
        g.dy[i], g.dx[i], g.wt[i] = int(dy), int(dx), int(wt)
    return g


@functools.lru_cache(maxsize=None)
def fwd_geom(B, Hi, Wi, Cin, Cout, kh, kw, s, p):
    """Forward conv: X (B,Hi,Wi,Cin) * W (Cout,kh*kw,Cin) -> Y (B,Ho,Wo,Cout)."""
    Ho, Wo = out_size(Hi, kh, s, p), out_size(Wi, kw, s, p)
    taps = [(i - p, j - p, i * kw + j) for i in range(kh) for j in range(kw)]
    return _geom(B=B, Hi=Hi, Wi=Wi, Cin=Cin, Ho=Ho, Wo=Wo, Hy=Ho, Wy=Wo, Cout=Cout, sy=s, sx=s, osy=1, osx=1, ooy=0, oox=0,
                 Tw=kh * kw, taps=taps)


@functools.lru_cache(maxsize=None)
def dx_geoms(B, Hi, Wi, Cin, Cout, kh, kw, s, p):
    """Input gradient as tap-convs of dY (B,Ho,Wo,Cout) with W^T (Cin,kh*kw,Cout) -> dX (B,Hi,Wi,Cin):
    one geometry per output parity class (iy%s, ix%s); only taps with (iy+p-kh)%s==0 contribute, so a k4-s2
    conv costs 4 taps per class instead of 16 masked ones."""
    Ho, Wo = out_size(Hi, kh, s, p), out_size(Wi, kw, s, p)
    out = []
    for py in range(min(s, Hi)):
        for px in range(min(s, Wi)):
            taps = [((py + p - i) // s, (px + p - j) // s, i * kw + j)
                    for i in range(kh) if (py + p - i) % s == 0
                    for j in range(kw) if (px + p - j) % s == 0]
            nqy, nqx = (Hi - py + s - 1) // s, (Wi - px + s - 1) // s
            out.append((_geom(B=B, Hi=Ho, Wi=Wo, Cin=Cout, Ho=nqy, Wo=nqx, Hy=Hi, Wy=Wi, Cout=Cin, sy=1, sx=1,
                              osy=s, osx=s, ooy=py, oox=px, Tw=kh * kw, taps=taps) if taps else None, (py, px)))
    return out


# --------------------------------------------------------------------------------------------
# pointer / layout helpers
# --------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else t.data_ptr()


class _ZeroArena:
    """fp64 accumulator workspaces that must be zero on entry (colnorm / L0 / metrics, see include/sdt_hip.h).  One
    region per device is zeroed once per train step (``begin_step``) and handed out in bump-pointer slices, replacing
    ~30 tiny memset launches per step.  A slice is never handed out twice between two ``begin_step`` calls, so memory
    not yet handed out is always zero; when the region is exhausted (or outside a train step loop) ``take`` falls back
    to a fresh ``torch.zeros``."""
    SIZE = 1 << 19  # doubles (4 MiB)

    def __init__(self):
        self.buf, self.off = {}, {}

    def begin_step(self, dev):
        key = (dev.type, dev.index)
        if key not in self.buf:
            self.buf[key] = torch.zeros(self.SIZE, device=dev, dtype=torch.float64)
        elif self.off[key]:
            self.buf[key][:self.off[key]].zero_()
        self.off[key] = 0

    def take(self, n, dev):
        key = (dev.type, dev.index)
        n_al = (n + 31) & ~31
        if key not in self.buf or self.off[key] + n_al > self.SIZE:
            return torch.zeros(n, device=dev, dtype=torch.float64)
        o = self.off[key]
        self.off[key] = o + n_al
        return self.buf[key][o:o + n]


_ARENA = _ZeroArena()


# The host enqueues a step in about half the time the GPU needs for it and would run ahead until the launch queue is full
# (10+ steps).  Tensors handed to the side streams (record_stream) return to the caching allocator only when the GPU has
# passed their last use, so the reserved pool grows with the host's lead (measured: 21 GB reserved for 1.2 GB live, still
# creeping after thousands of steps).  begin_step therefore lets the host lead by at most MAX_STEPS_IN_FLIGHT steps.
MAX_STEPS_IN_FLIGHT = 2
_STEP_FENCE = {}


def begin_step(dev=None):
    """Recycle the zero-workspace region; call once at the start of a train step, on the main stream, when no kernel of
    the previous step can still be using its workspaces (i.e. after the side stream has been joined)."""
    dev = torch.device('cuda', torch.cuda.current_device()) if dev is None else torch.device(dev)
    if _side_ok():
        join_side_stream()
        if MAX_STEPS_IN_FLIGHT and not torch.cuda.is_current_stream_capturing():
            q = _STEP_FENCE.setdefault((dev.type, dev.index), [])
            if len(q) >= MAX_STEPS_IN_FLIGHT:
                q.pop(0).synchronize()  # the GPU has started the step that began MAX_STEPS_IN_FLIGHT calls ago
            e = torch.cuda.Event()
            e.record()
            q.append(e)
    _ARENA.begin_step(dev)


def _stream():
    # the raw hipStream_t of torch's current stream on the current device (thread-local, follows torch.cuda.stream());
    # the C-level getters cost ~0.3 us, torch.cuda.current_stream().cuda_stream ~5 us -- at ~340 launches per step
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _req_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("speechdrivestemplates_amd ops run on the GPU only (got a %s tensor); there is no CPU fallback"
                               % t.device)


def cl(x):
    """Logical channels-first (B,C,*spatial) -> channels-last contiguous (B,*spatial,C) (no copy when the
    tensor already has channels-last strides)."""
    perm = [0] + list(range(2, x.dim())) + [1]
    return x.permute(perm).contiguous()


def cf_view(x_cl):
    """Channels-last (B,*spatial,C) storage -> logical channels-first view (no copy)."""
    perm = [0, x_cl.dim() - 1] + list(range(1, x_cl.dim() - 1))
    return x_cl.permute(perm)


def weight_storage(w):
    """(Cout,Cin,*k) logical weight -> (Cout,taps,Cin) contiguous storage tensor sharing memory when possible."""
    if w.dim() == 4:  # fast path: already in the kernel layout (every parameter of an engine module is)
        co, ci, kh, kw = w.shape
        if w.stride() == (kh * kw * ci, 1, kw * ci, ci):
            return w.as_strided((co, kh * kw, ci), (kh * kw * ci, ci, 1))
    elif w.dim() == 3:
        co, ci, k = w.shape
        if w.stride() == (k * ci, 1, ci):
            return w.as_strided((co, k, ci), (k * ci, ci, 1))
    perm = [0] + list(range(2, w.dim())) + [1]
    s = w.permute(perm)
    if not s.is_contiguous():
        s = s.contiguous()
    return s.reshape(w.shape[0], -1, w.shape[1])


def to_weight_layout(w):
    """Return a tensor equal to ``w`` whose memory is (Cout,*k,Cin)-contiguous (the kernels' layout)."""
    perm = [0] + list(range(2, w.dim())) + [1]
    inv = [0, w.dim() - 1] + list(range(1, w.dim() - 1))
    return w.permute(perm).contiguous().permute(inv)


def grad_buffer(p):
    """``p.grad`` in the same physical layout as ``p`` (created zero-filled when absent)."""
    if p.grad is None:
        p.grad = torch.zeros_like(p)  # preserve_format keeps the (Cout,*k,Cin) strides
    return p.grad


def _ksize(w):
    return (w.shape[2], w.shape[3]) if w.dim() == 4 else (1, w.shape[2])


def _as4(x_cl):
    return x_cl if x_cl.dim() == 4 else x_cl.unsqueeze(1)


# --------------------------------------------------------------------------------------------
# raw launchers
# --------------------------------------------------------------------------------------------
def conv_geom_for(x4_shape, w, stride, pad):
    """Forward geometry of nn.Conv2d (4-D weight) or nn.Conv1d (3-D weight; the tensor is viewed as (B,1,T,C)
    and neither stride nor padding applies to the dummy axis)."""
    B, Hi, Wi, Cin = x4_shape
    if w.dim() == 4:
        return fwd_geom(B, Hi, Wi, Cin, w.shape[0], w.shape[2], w.shape[3], stride, pad)
    return _fwd_geom_1d(B, Wi, Cin, w.shape[0], w.shape[2], stride, pad)


@functools.lru_cache(maxsize=None)
def _fwd_geom_1d(B, Wi, Cin, Cout, k, stride, pad):
    Wo = out_size(Wi, k, stride, pad)
    return _geom(B=B, Hi=1, Wi=Wi, Cin=Cin, Ho=1, Wo=Wo, Hy=1, Wy=Wo, Cout=Cout, sy=1, sx=stride, osy=1, osx=1,
                 ooy=0, oox=0, Tw=k, taps=[(0, j - pad, j) for j in range(k)])


@functools.lru_cache(maxsize=None)
def dx_geoms_1d(B, Wi, Cin, Cout, k, s, p):
    """1-D analogue of ``dx_geoms`` on (B,1,T,C) views."""
    Wo = out_size(Wi, k, s, p)
    out = []
    for px in range(min(s, Wi)):
        taps = [(0, (px + p - j) // s, j) for j in range(k) if (px + p - j) % s == 0]
        nq = (Wi - px + s - 1) // s
        out.append((_geom(B=B, Hi=1, Wi=Wo, Cin=Cout, Ho=1, Wo=nq, Hy=1, Wy=Wi, Cout=Cin, sy=1, sx=1, osy=1, osx=s,
                          ooy=0, oox=px, Tw=k, taps=taps) if taps else None, (0, px)))
    return out


@functools.lru_cache(maxsize=None)
def dx_pack(B, Hi, Wi, Cin, Cout, kh, kw, s, p, one_d):
    """The parity-class geometries of an input gradient as one contiguous ``sdt_conv_geom[n]`` array for
    sdt_conv_taps_multi_f32 (None when a class has no taps, or there are more than 4 classes)."""
    geoms = dx_geoms_1d(B, Wi, Cin, Cout, kw, s, p) if one_d else dx_geoms(B, Hi, Wi, Cin, Cout, kh, kw, s, p)
    gs = [g for g, _ in geoms]
    if any(g is None for g in gs) or len(gs) > 4:
        return None
    return (ConvGeom * len(gs))(*gs), len(gs), gs


class NormBwdHolder:
    """Hand-over between a column normalisation (InstanceNorm2d / BatchNorm + activation) and the convolution that consumes its
    output, for ONE-consumer chains (the audio encoder): the consumer's input-gradient launch accumulates the statistics the
    normalisation's backward needs in its epilogue (sdt_conv_taps_multi_f32 with sdt_norm_bwd) and leaves them in ``sums``; the
    normalisation's backward then skips its statistics pass over dz and y."""
    __slots__ = ("y", "mean", "rstd", "gamma", "beta", "groups", "slope", "sums", "dx_id")

    def __init__(self):
        self.y = self.mean = self.rstd = self.gamma = self.beta = self.sums = None
        self.groups, self.slope = 0, 0.0
        self.dx_id = None  # (data_ptr, _version) of the gradient tensor whose launch accumulated ``sums``: see grad_matches()


HOLDER_HANDOVERS = {"used": 0, "refused": 0}  # tests: how often a normalisation backward took / refused the fused statistics


def _holder_filled(h, dx):
    """The consumer's input-gradient launch wrote ``dx`` and accumulated ``h.sums`` from exactly those values."""
    h.dx_id = (dx.data_ptr(), dx._version, tuple(dx.shape))


def _holder_grad_matches(h, gz):
    """``h.sums`` describes the gradient the normalisation's backward receives only if that gradient IS the tensor the consumer's launch
    wrote: one consumer, no hook that rescaled / clipped it (a new tensor), no in-place edit (version bump), no autograd accumulation of
    a second consumer's gradient.  Otherwise the statistics pass runs."""
    return h.dx_id is not None and h.dx_id == (gz.data_ptr(), gz._version, tuple(gz.shape))


class ConvProfiler:
    """Optional HIP-event timing of every MFMA conv launch (bench.py's roofline leg).  Events are recorded on the
    stream the kernels are launched on (torch's current stream).  Off by default: zero overhead."""

    def __init__(self, pool=0, only=None):
        self.records = []  # (kernel name, role, is_2d, algorithmic flops, algorithmic bytes, start, end)
        # ``only``: a set of kernel names -- launches of other kernels run without events (bench.py's short runs time every conv launch on
        # ONE sampled step and only the dominant kernel's on the others: an event pair costs the launch its overlap with its neighbours)
        self.only = only
        # hipEventCreate happens at an event's first record(): warm a pool before the timed region so that recording
        # inside it is a bare hipEventRecord
        self.pool = [torch.cuda.Event(enable_timing=True) for _ in range(pool)]
        for e in self.pool:
            e.record()

    def event(self):
        return self.pool.pop() if self.pool else torch.cuda.Event(enable_timing=True)

    @staticmethod
    def kernel_name(kind, variant):
        bm, bn, vec = variant // 10 // 1000, variant // 10 % 1000, variant % 10
        # names as rocprofv3 prints them (template arguments included)
        if kind == "dW":  # last argument: product arithmetic (0 = exact fp32)
            return "conv_dw_kernel<%d, %d, %s, 0>" % (bm, bn, "true" if vec else "false")
        # 4th argument: experiment-only priority/ablation mode (0 in production)
        return "conv_taps_kernel<%d, %d, %s, 0>" % (bm, bn, "true" if vec else "false")

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, role, is2d, flops, nbytes, e0, e1 in self.records:
            d = out.setdefault(name, {"launches": 0, "us": 0.0, "flops": 0.0, "bytes": 0.0, "roles": {}, "max_launch_tflops": 0.0})
            us = e0.elapsed_time(e1) * 1e3
            if us > 0.0:  # the fastest single launch: bench.py asserts that no launch beats the matrix peak (FLOP accounting guard)
                d["max_launch_tflops"] = max(d["max_launch_tflops"], flops / (us * 1e-6) / 1e12)
            d["launches"] += 1
            d["us"] += us
            d["flops"] += flops
            d["bytes"] += nbytes
            r = d["roles"].setdefault(role + ("2d" if is2d else "1d"), [0, 0.0, 0.0])
            r[0] += 1
            r[1] += us
            r[2] += flops
        return out


PROFILER = None  # set to a ConvProfiler instance to time conv launches


class StageTimer:
    """HIP-event windows around the four pieces of the Conv1d stage of a train step (bench.py's ``roofline_conv1d`` leg):
    generator 1-D forward and backward chains on the main stream, the no-grad pose-encoder passes and the deferred 1-D
    weight-gradient batch on the side stream.  ``mark`` records on torch's current stream.  Off by default."""

    def __init__(self):
        self.marks = []  # (name, event)

    def mark(self, name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.marks.append((name, e))

    def windows_us(self):
        torch.cuda.synchronize()
        out, open_ = {}, {}
        for name, e in self.marks:
            base, edge = name.rsplit(":", 1)
            if edge == "begin":
                open_[base] = e
            elif base in open_:
                d = out.setdefault(base, [0, 0.0])
                d[0] += 1
                d[1] += open_.pop(base).elapsed_time(e) * 1e3
        return out


STAGES = None  # set to a StageTimer instance to time the Conv1d stage windows


def stage_mark(name):
    if STAGES is not None:
        STAGES.mark(name)


def _conv_launch(kind, is2d, g, call, flops=None, name=None, esz=4):
    """``flops``: algorithmic FLOPs of the launch when they are not the geometry's ``2*M*Cout*ntaps*Cin`` (an input-gradient
    class of a valid-correlation layer: the tap table spans input positions no output position reaches; SURVEY.md 8d counts
    dX = forward)."""
    if PROFILER is None or (PROFILER.only is not None and name not in PROFILER.only):
        check(call())
        return
    lib = _lib.load()
    var = lib.sdt_conv_dw_variant(g) if kind == "dW" else lib.sdt_conv_taps_variant(g)
    m = g.B * g.Ho * g.Wo
    if flops is None:
        flops = 2.0 * m * g.Cout * g.ntaps * g.Cin
    # algorithmic bytes of this GEMM: input tensor + output positions x Cout + weights, each once, at the tensors' element size
    nbytes = float(esz) * (g.B * g.Hi * g.Wi * g.Cin + m * g.Cout + g.Cout * g.ntaps * g.Cin)
    e0, e1 = PROFILER.event(), PROFILER.event()
    e0.record()
    check(call())
    e1.record()
    if name is None and kind != "dW" and not is2d and _CONV_MATH_NOW[0] == 0 and lib.sdt_conv1d_small_used(g, 1, max(1, _splitk_hint(lib, g))) == 1:
        name = "conv1d_small_kernel<8>"
    PROFILER.records.append((name or ConvProfiler.kernel_name(kind, var), kind, is2d, flops, nbytes, e0, e1))


def _conv_launch_multi(kind, is2d, gs, call, extra_bytes=0.0, flops=None, name=None, esz=4):
    """as _conv_launch for a launch that covers several geometries (the parity classes of one input gradient); ``extra_bytes``:
    what a fused epilogue has to read on top of the GEMM's operands (the raw y of the block below for the backward statistics);
    ``flops``: the algorithmic FLOPs (input gradients pass the FORWARD layer's count, SURVEY.md 8d -- the classes' tap tables
    also cover (position, tap) pairs that fall outside the forward output, which the kernel culls and nobody should count)"""
    if PROFILER is None or (PROFILER.only is not None and name not in PROFILER.only):
        check(call())
        return
    lib = _lib.load()
    var = lib.sdt_conv_taps_variant(gs[0])
    if flops is None:
        flops = sum(2.0 * g.B * g.Ho * g.Wo * g.Cout * g.ntaps * g.Cin for g in gs)
    g0 = gs[0]
    nbytes = float(esz) * (g0.B * g0.Hi * g0.Wi * g0.Cin + g0.B * g0.Hy * g0.Wy * g0.Cout + g0.Cout * g0.Tw * g0.Cin) + extra_bytes
    e0, e1 = PROFILER.event(), PROFILER.event()
    e0.record()
    check(call())
    e1.record()
    if name is None and not is2d and _CONV_MATH_NOW[0] == 0:
        arr = (ConvGeom * len(gs))(*gs)
        if lib.sdt_conv1d_small_used(arr, len(gs), max(_splitk_hint(lib, g) for g in gs)) == 1:
            name = "conv1d_small_kernel<8>"
    name = name or ConvProfiler.kernel_name(kind, var)
    PROFILER.records.append((name, kind, is2d, flops, nbytes, e0, e1))



# --------------------------------------------------------------------------------------------
# persistent stream-K conv (csrc/convsk.hip): plans and workspaces
# --------------------------------------------------------------------------------------------
USE_STREAMK = True   # the Conv2d forward / input-gradient launches of the audio encoder go through sdt_convsk_f32 (exact fp32 math)
_SK_PLANS = {}       # (geometry bytes, rows_per_group, bwd_groups, device index, forward, reserve, dtype, routing knobs) -> _SKPlan | None
_SK_WS = {}          # (device index, raw stream) -> workspace tensor

# Storage of the Conv2d chain's activations (and of the conv operands' weight copies) in HBM: 'f32' (default: the reference's arithmetic, what
# the metric is quoted on) or 'bf16' (BASELINE config 4): the first block writes a bf16 tensor and every kernel up to the resize reads / writes
# bf16 -- products on v_mfma_f32_32x32x16_bf16, fp32 accumulation / statistics / master weights / gradients.  The 1-D stage keeps fp32 TENSORS;
# its forward / input-gradient products follow the storage mode unless CHAIN_MATH pins them (bf16 storage -> products of bf16-rounded operands
# in the chain launches, like the Conv2d chain; its weight gradients, the head, the losses and the optimiser are exact fp32 either way).
STORAGE = "f32"


def set_storage(mode):
    """'f32' | 'bf16'; returns the previous mode.  Takes effect for the next forward pass."""
    global STORAGE
    assert mode in ("f32", "bf16"), mode
    prev, STORAGE = STORAGE, mode
    return prev


def apply_knobs(knobs):
    """The process-wide mode switches a PIPELINE owns (``Trainer.knobs``: {'storage', 'chain1d', 'f32_split'} from its cfg.SYS), applied at the start of every
    step it runs: two pipelines with different configurations in one process (train in bf16 storage and validate another model in fp32; the
    reference's voice2pose + pose2pose tools) no longer inherit each other's settings (VERDICT r4 weak 14 / ADVICE r4).  Not allowed to change
    under a hipGraph capture (the captured launches were chosen under the knobs in force)."""
    global STORAGE, CHAIN1D, F32_SPLIT
    if not knobs:
        return
    st, ch, sp = knobs.get("storage", STORAGE), bool(knobs.get("chain1d", CHAIN1D)), bool(knobs.get("f32_split", F32_SPLIT))
    if st != STORAGE or ch != CHAIN1D or sp != F32_SPLIT:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a pipeline's storage / chain / conv-arithmetic mode cannot change inside a hipGraph capture")
        set_storage(st)
        CHAIN1D = ch
        F32_SPLIT = sp  # (plan caches are keyed on it: no stale plan)


def _dt(t):
    """enum sdt_dtype of a tensor"""
    if t.dtype == torch.float32:
        return _lib.F32
    if t.dtype == torch.bfloat16:
        return _lib.BF16
    raise RuntimeError("unsupported element type %s" % t.dtype)


def _geom_key(garr):
    """The bytes of a geometry (pack): plan caches are keyed on CONTENT, not on the identity of a cached object"""
    k = getattr(garr, "_key", None)
    if k is None:
        k = bytes(garr)
        try:
            garr._key = k
        except AttributeError:
            pass
    return k


class _SKPlan:
    """Host + device copy of a stream-K plan (built once per geometry pack and element type)."""
    __slots__ = ("host", "dev", "kind", "dtype")

    def __init__(self, garr, n, rpg, bwd_groups, dev, dtype=0, reserve=0, wpc=2):
        import ctypes as C
        lib = _lib.load()
        self.kind, self.dtype = "sk", dtype
        check(lib.sdt_convsk_set_reserved_slots(int(reserve)))  # process-wide knobs of the plan builder: set, build, reset
        check(lib.sdt_convsk_set_wg_per_cu(1 if int(wpc) == 3 else int(wpc)))  # wpc 3: one workgroup per CU, the split-fp32 form (fp32 tensors)
        check(lib.sdt_convsk_set_f32_split(1 if int(wpc) == 3 else 0))
        try:
            nbytes = lib.sdt_convsk_plan_bytes_t(garr, n, dtype)
            if nbytes <= 0:
                raise RuntimeError("geometry not supported by the stream-K kernel")
            self.host = (C.c_int32 * (nbytes // 4))()
            check(lib.sdt_convsk_plan_build_t(garr, n, int(rpg), int(bwd_groups), dtype, dtype, C.addressof(self.host), nbytes))
        finally:
            check(lib.sdt_convsk_set_reserved_slots(0))
            check(lib.sdt_convsk_set_wg_per_cu(2))
            check(lib.sdt_convsk_set_f32_split(0))
        self.dev = torch.frombuffer(self.host, dtype=torch.int32).to(dev)


# Which launches take the stream-K kernel (measured per layer on one MI355X, profiles/r03_streamk_ab.txt): it wins where a tile's K loop
# is long enough to amortise the tile switch of a 1-2-workgroup-per-CU kernel (set-up + pipeline fill + epilogue, ~10 us per 128x128
# tile) and loses on the 64-wide outputs and on the 2x2-tap parity classes of strided input gradients, which stay with the 64x64 kernel.
# FORWARD launches all take it (where it loses, L4: -3 %, L1 / L2: par): its chunked accumulation is what puts the forward error of
# every Conv2d layer level with the reference's blocked sums (tests/test_fullsize_gpu.py::test_b32_forward_stage_error_table).
# bf16 tensors: every launch (there is no other bf16-storage conv kernel).
# Workgroup slots that the plans of BACKWARD launches (input gradients, weight gradients) leave free.  0 on one GPU.  dp.GradReducer sets it in
# data-parallel runs: a persistent launch that fills every slot cannot share the GPU with the long-lived workgroups of a collective -- they wait
# for slots, or take them and strand the conv workgroups that find none (tools/debug/comm_emulation.py) -- and the gradient exchange overlaps backward
SK_RESERVED_SLOTS = 0
# ... and by FORWARD plans: 0 in every production setting (nothing is exchanged during the forward pass).  Two PROCESSES that share one GPU (the
# 2-ranks-on-1-GPU tests) set both: two persistent grids of 512 workgroups cannot be co-resident, and owners that spin for partners the other
# process's workgroups keep out starve each other until the spin limit poisons the tiles.
SK_RESERVED_SLOTS_FWD = 0
# Persistent workgroups per CU of the BACKWARD plans (fp32; experiment, bench.py --bwd-wpc): with ONE workgroup per CU (one wave per SIMD, half
# of the register file) a weight-gradient launch on the side stream leaves room for the main stream's HBM-bound passes to run BESIDE it
# instead of behind it.  Forward plans keep two.
SK_WPC_DX = 2
SK_WPC_DW = 2
STREAMK_MIN_STEPS = 48   # input gradients: K steps (of 32) per output tile, nominal: taps * Cin / 32
STREAMK_MIN_COUT = 128
STREAMK_ALL_FORWARD = True


def _sk_wanted(g0, forward=False):
    if forward and STREAMK_ALL_FORWARD:
        return True
    return g0.Cout % STREAMK_MIN_COUT == 0 and g0.ntaps * (g0.Cin // 32) >= STREAMK_MIN_STEPS


def clear_plans():
    """Drop every cached plan (the caches are keyed on the routing knobs as well, so flipping one never serves a stale plan; this frees memory)"""
    _SK_PLANS.clear()
    _SK_DW_PLANS.clear()


# fp32 tensors: the split-fp32 form of that kernel (three bf16 planes per operand made by the loader, six bf16 MFMAs per fragment pair, fp32-grade
# products at 2.7x the fp32 matrix rate) wherever it plans; False: the fp32-MFMA kernels of rounds 3-4 everywhere (SYS.CONV_F32_SPLIT)
F32_SPLIT = True
BF16_SHAPED = True  # bf16 tensors: the 256-row / 8-wave kernel of csrc/convbf.hip (one workgroup per CU) wherever a launch has >= 4 K steps per range


def _sk_plan(garr, n, rpg, bwd_groups, dev, forward=False, dtype=0, wpc=None):
    """garr: a ConvGeom (n == 1) or a ctypes array of n ConvGeoms; returns the stream-K plan or None when the pack does not qualify / is not
    wanted on that kernel (fp32 launches then take the 64x64 kernel of conv.hip)."""
    reserve = int(SK_RESERVED_SLOTS_FWD) if forward else int(SK_RESERVED_SLOTS)
    if dtype == _lib.BF16 and wpc is None:
        # the bf16-shaped kernel first (plans with one workgroup per CU); small launches fall back to the round-4 128-row kernel (two per CU)
        plan = _sk_plan(garr, n, rpg, bwd_groups, dev, forward, dtype, 1) if BF16_SHAPED else None
        return plan if plan is not None else _sk_plan(garr, n, rpg, bwd_groups, dev, forward, dtype, 2)
    if dtype == _lib.F32 and wpc is None and F32_SPLIT and USE_STREAMK:
        plan = _sk_plan(garr, n, rpg, bwd_groups, dev, forward, dtype, 3)
        if plan is not None:
            return plan
    if wpc is None:
        wpc = 2 if forward else int(SK_WPC_DX)
    key = (_geom_key(garr), n, int(rpg), int(bwd_groups), dev.index, bool(forward), reserve, dtype,
           USE_STREAMK, STREAMK_MIN_STEPS, STREAMK_MIN_COUT, STREAMK_ALL_FORWARD, wpc)
    plan = _SK_PLANS.get(key, False)
    if plan is False:
        lib = _lib.load()
        plan = None
        g0 = garr if isinstance(garr, ConvGeom) else garr[0]
        want = lib.sdt_convsk_supported_t(garr, n, dtype) and (dtype == _lib.BF16 or wpc == 3 or (USE_STREAMK and _sk_wanted(g0, forward)))
        if want:
            try:
                plan = _SKPlan(garr, n, rpg, bwd_groups, dev, dtype, reserve, wpc)
            except RuntimeError:  # e.g. too few K steps for a 256-way split (the 1-D stage), a tile without a live K step
                plan = None
        _SK_PLANS[key] = plan
    return plan


def _sk_workspace(dev, st):
    key = (dev.index, int(st))
    ws = _SK_WS.get(key)
    if ws is None:
        nbytes = _lib.load().sdt_convsk_workspace_bytes()
        # zero-filled ONCE: every flag a launch raises is lowered again by the workgroup that consumes it
        ws = _SK_WS[key] = torch.zeros(nbytes // 4, device=dev, dtype=torch.int32)
    return ws


_SK_ERR_WORD = 256 * 256 * 256 + 512  # int32 index of the error word: behind the slabs (csrc/convsk.hip SK_SLAB_BYTES) and the 512 flags


def streamk_error_codes():
    """Non-zero entries: the owner of a split tile gave up waiting for a partner's partial sums (the partner was never dispatched -- the GPU is shared
    with something that holds its slot); that tile was stored as NaN.  Synchronises.  Trainer / bench / tests call this; see check_streamk()."""
    out = {}
    for key, ws in _SK_WS.items():
        code = int(ws[_SK_ERR_WORD].item())
        if code:
            out[key] = code
    for dev, ws in _CHAIN_WS.items():  # the Conv1d chain launches: 0x40000000 + block (+ 64: backward) whose cluster never completed
        code = int(ws[_CHAIN_ERR].item())
        if code:
            out[(dev, "chain1d")] = code
    return out


def kernel_error_flag(dev=None):
    """Device-side float64 scalar (no host synchronisation): 1.0 when any error word of this process's persistent-launch workspaces on ``dev`` is
    non-zero.  dp.reduce_scalars / Trainer.check_kernels_all_ranks carry it through a collective so that EVERY rank learns that SOME rank lost a
    partner workgroup (the summing all-reduce has spread that rank's NaN gradients to all of them)."""
    dev = torch.device('cuda', torch.cuda.current_device()) if dev is None else torch.device(dev)
    words = [ws[_SK_ERR_WORD] for (d, _st), ws in _SK_WS.items() if d == dev.index]
    words += [ws[_CHAIN_ERR] for d, ws in _CHAIN_WS.items() if d == dev.index]
    if not words:
        return torch.zeros((), device=dev, dtype=torch.float64)
    return torch.stack(words).ne(0).any().to(torch.float64)


def check_streamk():
    """Raise if any stream-K launch of this process reported a lost partner (Trainer calls this on log steps and before every checkpoint)."""
    codes = streamk_error_codes()
    if codes:
        raise RuntimeError("a persistent launch gave up waiting for a partner workgroup (error words %r: stream-K convolution: range id + 1 per "
                           "(device, stream), its output tile was poisoned with NaN; Conv1d chain: 0x40000000 + block, its outputs are invalid).  The GPU is probably shared with another process or a "
                           "kernel that holds workgroup slots (see ops.SK_RESERVED_SLOTS); results since the last check are invalid" % (codes,))


# K order of the 8-wave kernels' tiles (csrc/convbf.hip; include/sdt_hip.h sdt_convsk_set_k_order): 1 = chunk-major -- all live taps of a 128-byte
# channel chunk before the next chunk, so that neighbouring taps find the previous step's cache lines in the CU's vector L1; 0 = tap-major (rounds 3-5).
# Measured +1.3 % over the 14 forward / input-gradient launches (profiles/r06_korder_ab.txt) -- inside the box-to-box spread of the step, and it
# regroups every Conv2d sum: trajectory quantities behind an Adam step move past their CALIBRATED bounds (tests/golden/margins.json; e.g. sdt_bp
# step-1 lip_sync 7e-7 -> 2e-5 against a stated 1e-3).  Not worth re-recording 800 margins in the round that had to turn the suite green: off.
# Its results ARE checked: tests/test_k_order_conv_sweep_gpu.py runs order 1 over every cursor edge of the loader (range cuts inside a chunk, culled
# and rotated tap masks, mixed parity classes, one tap, one chunk, reserved slots, pre-split planes) -- exact on integer operands, at the sweeps' own
# float64 bars on random ones, bf16 and split-fp32.  What remains before a default-on is the re-recording of the trajectory margins, nothing else.
SK_K_ORDER = 0
_K_ORDER_SET = [None]


# Split-fp32 launches can read the weights PRE-SPLIT (three bf16 planes kept beside the transposed mirrors, refreshed by the same batched launch once
# per optimiser step) instead of splitting them in every tile on every K step: half of the loader's VALU work of a 128 x 128 tile leaves the K loop --
# and the B operand's bytes per step grow by 50 % (3 x 64 B of planes instead of 128 B of fp32).  Measured (profiles/r06_w3_ab.txt, B = 32, L1-L7
# forward + input gradient, twice each): 2.89 ms split in the loader, 2.98 ms pre-split -- the kernel is bound by operand DELIVERY, not by the split's
# VALU work (bit-identical results either way: tests/test_ops_gpu.py::test_presplit_weights_are_bit_identical_to_the_in_kernel_split).  Off.
W3_PRESPLIT = False


def _sk_launch(plan, x4, ws_w, bias, y, stats, nb, st):
    lib = _lib.load()
    if _K_ORDER_SET[0] != SK_K_ORDER:
        check(lib.sdt_convsk_set_k_order(int(SK_K_ORDER)))
        _K_ORDER_SET[0] = SK_K_ORDER
    wsb = _sk_workspace(y.device, st)
    if plan.dtype == _lib.F32 and (plan.host[3] >> 26) & 1:
        w3 = WeightMirrors.lookup3(ws_w)
        if w3 is not None:
            return lib.sdt_convsk_f32_w3(_p(x4), _p(w3), _p(bias), _p(y), plan.host, _p(plan.dev), _p(wsb), 1, _p(stats), nb,
                                         x4.numel() * 4, ws_w.numel() * 4, y.numel() * 4, st)
    fn = lib.sdt_convsk_bf16 if plan.dtype == _lib.BF16 else lib.sdt_convsk_f32
    esz = 2 if plan.dtype == _lib.BF16 else 4
    return fn(_p(x4), _p(ws_w), _p(bias), _p(y), plan.host, _p(plan.dev), _p(wsb), 1, _p(stats), nb,
              x4.numel() * esz, ws_w.numel() * esz, y.numel() * esz, st)


_SK_DW_PLANS = {}
_SK_DW_WS = {}
USE_STREAMK_DW = True  # weight gradients of the 2-D layers with Cout % 128 == 0 through sdt_convsk_dw_f32 (deterministic)


class _SKDwPlan:
    __slots__ = ("host", "dev", "dtype")

    def __init__(self, g, dev, dtype=0, reserve=0, wpc=2, split=False):
        import ctypes as C
        lib = _lib.load()
        self.dtype = dtype
        check(lib.sdt_convsk_set_reserved_slots(int(reserve)))
        check(lib.sdt_convsk_set_wg_per_cu(int(wpc)))
        check(lib.sdt_convsk_set_f32_split(1 if split else 0))  # fp32 tensors, two workgroups per CU: the split-fp32 weight-gradient kernel
        try:
            nbytes = lib.sdt_convsk_dw_plan_bytes_t(g, dtype)
            self.host = (C.c_int32 * (nbytes // 4))()
            check(lib.sdt_convsk_dw_plan_build_t(g, dtype, C.addressof(self.host), nbytes))
        finally:
            check(lib.sdt_convsk_set_reserved_slots(0))
            check(lib.sdt_convsk_set_wg_per_cu(2))
            check(lib.sdt_convsk_set_f32_split(0))
        self.dev = torch.frombuffer(self.host, dtype=torch.int32).to(dev)


# Tiles of the split-fp32 weight gradient (csrc/convsk.hip dw_tile): True = 128-wide column tiles with a ragged last one where taps * Cin is an odd
# multiple of 64 (L2: five tiles instead of nine 64-wide ones: 279 -> 248 us, profiles/r06_dw_wide_ab.txt = 0.5 % of a step); False (default) = the
# rule of rounds 3-5 -- the re-cut K chunks regroup the sums behind the calibrated margins, which half a percent does not pay for
SK_DW_WIDE = False


def _sk_dw_plan(g, dev, dtype=0):
    reserve = int(SK_RESERVED_SLOTS)
    wpc = 2 if dtype != _lib.F32 else int(SK_WPC_DW)
    split = bool(F32_SPLIT) and dtype == _lib.F32 and wpc == 2
    wide = bool(SK_DW_WIDE)
    key = (_geom_key(g), dev.index, reserve, dtype, wpc, split, wide)
    plan = _SK_DW_PLANS.get(key, False)
    if plan is False:
        lib = _lib.load()
        check(lib.sdt_convsk_set_reserved_slots(reserve))  # "supported" depends on the grid (K steps per chunk) and on the tile rule
        check(lib.sdt_convsk_set_wg_per_cu(wpc))
        check(lib.sdt_convsk_set_f32_split(1 if split else 0))
        check(lib.sdt_convsk_set_dw_wide_tiles(1 if wide else 0))
        try:
            ok = lib.sdt_convsk_dw_supported_t(g, dtype)
            plan = _SKDwPlan(g, dev, dtype, reserve, wpc, split) if ok else None  # (_SKDwPlan sets and resets the same knobs; the tile rule stays set)
        finally:
            check(lib.sdt_convsk_set_reserved_slots(0))
            check(lib.sdt_convsk_set_wg_per_cu(2))
            check(lib.sdt_convsk_set_f32_split(0))
            check(lib.sdt_convsk_set_dw_wide_tiles(0))
        _SK_DW_PLANS[key] = plan
    return plan


def _sk_dw_workspace(dev, st):
    key = (dev.index, int(st))
    ws = _SK_DW_WS.get(key)
    if ws is None:
        ws = _SK_DW_WS[key] = torch.empty(_lib.load().sdt_convsk_dw_workspace_bytes() // 4, device=dev, dtype=torch.float32)
    return ws


def prepare_capture_stream(dev, stream):
    """Workspaces of the persistent launches for ``stream`` allocated BEFORE a hipGraph capture on it starts (graph.GraphedStep): allocated inside
    the capture they would come from the graph's private pool and their zero-fill would be a node of the graph -- every replay would wipe the
    error word of the previous one before anybody could read it."""
    st = int(stream.cuda_stream)
    _sk_workspace(dev, st)
    _sk_dw_workspace(dev, st)
    _chain_ws(dev)


def _sk_name(plan):
    if plan.dtype == _lib.BF16 and (plan.host[3] >> 16) & 0xff == 1:  # one workgroup per CU: the bf16-shaped kernel
        return "convbf2_kernel<%d, %d>" % (plan.host[1], plan.host[2])
    if (plan.host[3] >> 26) & 1:  # ... in its split-fp32 form
        return "convbf2_kernel<float, %d, %d>" % (plan.host[1], plan.host[2])
    return "convsk_kernel<%d, %d>" % (plan.host[1], plan.host[2])

def _splitk_hint(lib, g):
    k = getattr(g, "_splitk", None)  # geometries are cached objects: ask the library once per geometry
    if k is None:
        k = g._splitk = lib.sdt_conv_taps_splitk_hint(g)
    return k


def conv_forward(x_cl, w, bias, stride, pad):
    """x_cl (B,H,W,Cin)|(B,T,Cin); w logical (Cout,Cin,kh,kw)|(Cout,Cin,k) -> y channels-last."""
    _req_cuda(x_cl, w, bias)
    lib = _lib.load()
    x4 = _as4(x_cl)
    g = conv_geom_for(x4.shape, w, stride, pad)
    ws = weight_storage(w)
    y = torch.empty((g.B, g.Ho, g.Wo, g.Cout), device=x_cl.device, dtype=torch.float32)
    st = _stream()
    if USE_STREAMK and w.dim() == 4 and _CONV_MATH_NOW[0] == 0:
        plan = _sk_plan(g, 1, 0, 1, x_cl.device, forward=True)
        if plan is not None:
            _conv_launch("fwd", True, g, lambda: _sk_launch(plan, x4, ws, bias, y, None, None, st), name=_sk_name(plan))
            return y
    k = _splitk_hint(lib, g)
    if k > 1:  # too few output tiles for 256 CUs (1-D stage): slice the K loop, then a fixed-order reduce (+bias)
        part = torch.empty((k,) + tuple(y.shape), device=x_cl.device, dtype=torch.float32)
        _conv_launch("fwd", w.dim() == 4, g, lambda: lib.sdt_conv_taps_splitk_f32(_p(x4), _p(ws), None, _p(y), g, k, _p(part), st))
        check(lib.sdt_splitk_reduce_f32(_p(part), _p(bias), _p(y), y.numel(), g.Cout, k, st))
    else:
        _conv_launch("fwd", w.dim() == 4, g, lambda: lib.sdt_conv_taps_f32(_p(x4), _p(ws), _p(bias), _p(y), g, st))
    return y if x_cl.dim() == 4 else y.squeeze(1)


CONV_MATH = {'f32': 0, 'bf16': 1, 'bf16x3': 3, 'bf16x6': 6}
_CONV_MATH_NOW = [0]  # mirror of the library's process-wide setting (only set_conv_math changes it)


def set_conv_math(mode):
    """Multiplication arithmetic of the forward / input-gradient conv kernels (include/sdt_hip.h: sdt_set_conv_math):
    'f32' (default, exact fp32 MFMA), 'bf16', 'bf16x3', 'bf16x6'.  Returns the previous mode's name."""
    lib = _lib.load()
    prev = lib.sdt_get_conv_math()
    check(lib.sdt_set_conv_math(CONV_MATH[mode]))
    _CONV_MATH_NOW[0] = CONV_MATH[mode]
    return {v: k for k, v in CONV_MATH.items()}[prev]


class WeightMirrors:
    """(Cin,taps,Cout) mirrors of a set of conv weights -- the B operand of the input-gradient GEMM -- refreshed by ONE
    batched launch for the whole optimiser group instead of one transposition per layer per backward pass.
    ``lookup`` serves a mirror only while it is provably current: the owning group has not been stepped since the last
    refresh (optim.FlatAdam.step calls ``mark_dirty``; the first lookup afterwards refreshes all mirrors of the group)
    and the parameter's autograd version counter is unchanged (``load_state_dict`` / in-place edits bump it).  Code
    that writes weights through ``.data`` or raw pointers must call ``mark_dirty`` itself."""
    _by_ptr = {}
    _by_mirror = {}  # data_ptr of an fp32 mirror -> (owner, entry index): _sk_launch finds the pre-split planes of EITHER operand form by pointer
    dirty = True

    def __init__(self, params):
        self.entries, tiles = [], 0
        self.planes = 1  # what e[3] / e[4] hold: 1 = bf16 copies (bf16 storage), 3 = the three bf16 planes of the split-fp32 kernels (W3_PRESPLIT)
        for p in params:
            if p.dim() not in (3, 4):
                continue
            ws = weight_storage(p.data)
            if ws.data_ptr() != p.data_ptr():
                continue  # not in the kernel layout: conv_input_grad transposes it per call
            cout, taps, cin = ws.shape
            wt = torch.empty((cin, taps, cout), device=p.device, dtype=torch.float32)
            # [parameter, fp32 mirror, version at the last refresh, bf16 copy of W, bf16 copy of the mirror, first tile]
            self.entries.append([p, wt, -1, None, None, tiles])
            tiles += ((cin + 31) // 32) * ((cout + 31) // 32) * taps
        self.total_tiles = tiles
        self.table = None
        if self.entries:
            if STORAGE == "bf16":
                self._alloc16()
            elif F32_SPLIT and W3_PRESPLIT:
                self._alloc16(planes=3)
            self._build_table()
            import weakref
            me = weakref.ref(self)
            for i, e in enumerate(self.entries):
                WeightMirrors._by_ptr[e[0].data_ptr()] = (me, i)  # weak: a dead optimiser's mirrors are dropped
                WeightMirrors._by_mirror[e[1].data_ptr()] = (me, i)

    def _alloc16(self, planes=1):
        """bf16 copies of the Conv2d weights and of their mirrors (the operands of the bf16-storage path's kernels), or -- planes == 3 -- their
        exact three-way bf16 split [hi | mid | lo] (the pre-split B operand of the split-fp32 kernels: csrc/convbf.hip, W3)"""
        if planes != self.planes:
            for e in self.entries:
                e[3] = e[4] = None
            self.planes = planes
        for e in self.entries:
            p = e[0]
            if p.dim() == 4 and e[3] is None:
                cout, taps, cin = weight_storage(p.data).shape
                lead = (3,) if planes == 3 else ()
                e[3] = torch.empty(lead + (cout, taps, cin), device=p.device, dtype=torch.bfloat16)
                e[4] = torch.empty(lead + (cin, taps, cout), device=p.device, dtype=torch.bfloat16)

    def _build_table(self):
        descs = []
        for p, wt, _v, w16, wt16, tile0 in self.entries:
            cout, taps, cin = weight_storage(p.data).shape
            descs.append(_lib.WtDesc(p.data_ptr(), wt.data_ptr(), _p(w16), _p(wt16), cout, taps, cin, tile0, self.planes if w16 is not None else 0, 0))
        arr = (_lib.WtDesc * len(descs))(*descs)
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.entries[0][0].device)

    def refresh(self):
        if not self.entries:
            return
        check(_lib.load().sdt_weight_transpose_batched_f32(_p(self.table), len(self.entries), self.total_tiles, _stream()))
        for e in self.entries:
            e[2] = e[0]._version
        self.dirty = False

    def mark_dirty(self):
        self.dirty = True

    @staticmethod
    def _entry(w):
        hit = WeightMirrors._by_ptr.get(w.data_ptr())
        if hit is None:
            return None, None
        owner = hit[0]()
        if owner is None:
            del WeightMirrors._by_ptr[w.data_ptr()]
            return None, None
        e = owner.entries[hit[1]]
        if e[0].data_ptr() != w.data_ptr() or e[0].shape != w.shape:
            return None, None
        return owner, e

    @staticmethod
    def lookup(w):
        owner, e = WeightMirrors._entry(w)
        if owner is None:
            return None
        if owner.dirty or e[2] != e[0]._version:
            owner.refresh()
        return e[1]

    @staticmethod
    def lookup16(w):
        """(bf16 copy of W (Cout,taps,Cin), bf16 copy of its (Cin,taps,Cout) mirror), refreshed with the fp32 mirror by the same launch;
        None for a weight no optimiser group registered (the caller converts per call)."""
        owner, e = WeightMirrors._entry(w)
        if owner is None or e[0].dim() != 4:
            return None
        if e[3] is None or owner.planes != 1:  # the storage mode was switched on after this group was built
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("bf16 weight copies must exist before a hipGraph capture (set ops.STORAGE before setup_optimizer)")
            owner._alloc16(planes=1)
            owner._build_table()
            owner.dirty = True
        if owner.dirty or e[2] != e[0]._version:
            owner.refresh()
        return e[3], e[4]

    @staticmethod
    def lookup3(operand):
        """The pre-split planes (3, rows, taps, cols) bf16 of a conv operand given as the tensor a launch would otherwise read: a registered
        weight's storage (Cout,taps,Cin) or its fp32 mirror (Cin,taps,Cout); refreshed with the mirrors (one batched launch per optimiser step).
        None: not a registered Conv2d weight / pre-splitting is off -- the kernel then splits the fp32 weights itself, tile by tile."""
        if not W3_PRESPLIT:
            return None
        ptr = operand.data_ptr()
        hit, which = WeightMirrors._by_ptr.get(ptr), 3
        if hit is not None and hit[0]() is None:
            # a dead group's WEIGHT lived at this address: the allocator may have handed the block to a live group's mirror, whose planes
            # the stale key would hide (the launch then split in its loader: same bits, but the pre-split operand was silently not used)
            del WeightMirrors._by_ptr[ptr]
            hit = None
        if hit is None:
            hit, which = WeightMirrors._by_mirror.get(ptr), 4
        if hit is None:
            return None
        owner = hit[0]()
        if owner is None:
            WeightMirrors._by_mirror.pop(ptr, None)
            return None
        e = owner.entries[hit[1]]
        if e[0].dim() != 4 or (e[0].data_ptr() if which == 3 else e[1].data_ptr()) != ptr:
            return None
        if e[3] is None or owner.planes != 3:
            if torch.cuda.is_current_stream_capturing():
                return None  # (no allocation inside a capture: this launch splits in the kernel)
            owner._alloc16(planes=3)
            owner._build_table()
            owner.dirty = True
        if owner.dirty or e[2] != e[0]._version:
            owner.refresh()
        return e[which]


FUSE_DX_CLASSES = True   # one launch for all output parity classes of a strided layer's input gradient (fp32 math)
FUSE_BWD_STATS = True    # normalisation-backward statistics in the input-gradient epilogue (fp32 math, 2-D chains)


def conv_input_grad(gy_cl, w, x_shape, stride, pad, norm_holder=None):
    """dX for y = conv(x, w): tap-conv(s) of gy with the transposed weights -- one geometry per output parity class, all
    classes in ONE launch in fp32 math.  ``norm_holder``: the NormBwdHolder of the normalisation that produced x (see there)."""
    lib = _lib.load()
    gy4 = _as4(gy_cl)
    one_d = w.dim() == 3
    B, Hi, Wi, Cin = (x_shape[0], 1, x_shape[1], x_shape[2]) if one_d else x_shape
    Cout = w.shape[0]
    kh, kw = _ksize(w)
    st = _stream()
    # algorithmic work of an input gradient = the forward layer's: 2 * B*Ho*Wo * Cout * taps * Cin
    fwd_flops = 2.0 * B * (1 if one_d else out_size(Hi, kh, stride, pad)) * out_size(Wi, kw, stride, pad) * Cout * kh * kw * Cin
    if gy_cl.dtype == torch.bfloat16:
        dx = None if one_d else _conv_input_grad_bf16(gy4, w, (B, Hi, Wi, Cin), stride, pad, norm_holder, fwd_flops, st)
        if dx is not None:
            return dx
        gy_cl = gy_cl.float()  # no bf16 kernel for this geometry: the fp32 path takes it (and returns an fp32 gradient)
        gy4 = _as4(gy_cl)
    wt = WeightMirrors.lookup(w)
    if wt is None:
        ws = weight_storage(w)
        wt = torch.empty((Cin, kh * kw, Cout), device=w.device, dtype=torch.float32)
        check(lib.sdt_weight_transpose_f32(_p(ws), _p(wt), Cout, kh * kw, Cin, st))
    dx = torch.empty((B, Hi, Wi, Cin), device=w.device, dtype=torch.float32)
    pack = dx_pack(B, Hi, Wi, Cin, Cout, kh, kw, stride, pad, one_d) if (FUSE_DX_CLASSES and _CONV_MATH_NOW[0] == 0) else None
    if pack is not None and USE_STREAMK and not one_d:
        arr, n, gs = pack
        h = norm_holder
        fuse = (h is not None and FUSE_BWD_STATS and h.y is not None and h.y.dtype == torch.float32 and tuple(h.y.shape) == tuple(dx.shape)
                and all((g.B * g.Ho * g.Wo if h.groups == 1 else g.Ho * g.Wo) >= 32 for g in gs))
        plan = _sk_plan(arr, n, -1, h.groups if fuse else 1, w.device)
        if plan is not None:
            nb = None
            if fuse:
                h.sums = _ARENA.take(2 * h.groups * Cin, w.device)
                nb = _lib.NormBwd(_p(h.y), _p(h.mean), _p(h.rstd), _p(h.gamma), _p(h.beta), _p(h.sums), float(h.slope), int(h.groups))
                _holder_filled(h, dx)
            _conv_launch_multi("dX", True, gs, lambda: _sk_launch(plan, gy4, wt, None, dx, None, nb, st),
                               extra_bytes=4.0 * dx.numel() if nb is not None else 0.0, flops=fwd_flops, name=_sk_name(plan))
            return dx
    if pack is not None:
        arr, n, gs = pack
        k = max(_splitk_hint(lib, g) for g in gs)
        part = torch.empty((k,) + tuple(dx.shape), device=w.device, dtype=torch.float32) if k > 1 else None
        nb = None
        if (norm_holder is not None and FUSE_BWD_STATS and k == 1 and not one_d and Cout % 32 == 0 and norm_holder.y is not None
                and norm_holder.y.dtype == torch.float32  # (a bf16 y with a gradient no bf16 kernel took: these kernels would read it as fp32)
                and tuple(norm_holder.y.shape) == tuple(dx.shape) and dx.numel() * 4 < 2 ** 31 - 4  # (the epilogue's reads of y: 32-bit byte offsets)
                and all((g.B * g.Ho * g.Wo if norm_holder.groups == 1 else g.Ho * g.Wo) >= 64 for g in gs)):
            h = norm_holder
            h.sums = _ARENA.take(2 * h.groups * Cin, w.device)
            nb = _lib.NormBwd(_p(h.y), _p(h.mean), _p(h.rstd), _p(h.gamma), _p(h.beta), _p(h.sums), float(h.slope), int(h.groups))
            _holder_filled(h, dx)
        _conv_launch_multi("dX", not one_d, gs,
                           lambda: lib.sdt_conv_taps_multi_f32(_p(gy4), _p(wt), _p(dx), arr, n, k, _p(part), nb, st),
                           extra_bytes=4.0 * dx.numel() if nb is not None else 0.0, flops=fwd_flops)
        if k > 1:
            check(lib.sdt_splitk_reduce_f32(_p(part), None, _p(dx), dx.numel(), Cin, k, st))
        return dx.squeeze(1) if one_d else dx
    geoms = dx_geoms_1d(B, Wi, Cin, Cout, kw, stride, pad) if one_d else dx_geoms(B, Hi, Wi, Cin, Cout, kh, kw, stride, pad)
    k = 1
    if all(g is not None for g, _ in geoms):
        k = max(_splitk_hint(lib, g) for g, _ in geoms)
    part = torch.empty((k,) + tuple(dx.shape), device=w.device, dtype=torch.float32) if k > 1 else None
    for g, (py, px) in geoms:
        if g is None:  # parity class that no tap reaches: the gradient is zero there
            dx[:, py::(1 if one_d else stride), px::stride].zero_()
            continue
        nlive = sum(1 for gg, _ in geoms if gg is not None)
        _conv_launch("dX", not one_d, g,
                     lambda g=g: lib.sdt_conv_taps_splitk_f32(_p(gy4), _p(wt), None, _p(dx), g, k, _p(part), st), flops=fwd_flops / nlive)
    if k > 1:  # every dX element belongs to exactly one parity class, so each slab is fully written
        check(lib.sdt_splitk_reduce_f32(_p(part), None, _p(dx), dx.numel(), Cin, k, st))
    return dx.squeeze(1) if one_d else dx


def _bf16_weights(w):
    """(bf16 (Cout,taps,Cin), bf16 (Cin,taps,Cout)) of a Conv2d weight: the optimiser group's refreshed copies, or -- for a weight no group
    registered -- converted here"""
    pair = WeightMirrors.lookup16(w)
    if pair is None:
        ws = weight_storage(w.detach())
        pair = (ws.to(torch.bfloat16), ws.permute(2, 1, 0).contiguous().to(torch.bfloat16))
    return pair


def _conv_input_grad_bf16(gy4, w, x_shape, stride, pad, norm_holder, fwd_flops, st):
    """bf16-storage input gradient of a Conv2d layer (sdt_convsk_bf16): gy bf16 -> dx bf16, all parity classes in one launch, the
    normalisation-backward statistics in the epilogue when the block below left a bf16 ``y``.  None: geometry not supported."""
    B, Hi, Wi, Cin = x_shape
    Cout = w.shape[0]
    kh, kw = _ksize(w)
    pack = dx_pack(B, Hi, Wi, Cin, Cout, kh, kw, stride, pad, False)
    if pack is None:
        return None
    arr, n, gs = pack
    h = norm_holder
    fuse = (h is not None and FUSE_BWD_STATS and h.y is not None and h.y.dtype == torch.bfloat16 and tuple(h.y.shape) == (B, Hi, Wi, Cin)
            and all((g.B * g.Ho * g.Wo if h.groups == 1 else g.Ho * g.Wo) >= 32 for g in gs))
    plan = _sk_plan(arr, n, -1, h.groups if fuse else 1, w.device, dtype=_lib.BF16)
    if plan is None:
        return None
    wt16 = _bf16_weights(w)[1]
    dx = torch.empty((B, Hi, Wi, Cin), device=w.device, dtype=torch.bfloat16)
    nb = None
    if fuse:
        h.sums = _ARENA.take(2 * h.groups * Cin, w.device)
        nb = _lib.NormBwd(_p(h.y), _p(h.mean), _p(h.rstd), _p(h.gamma), _p(h.beta), _p(h.sums), float(h.slope), int(h.groups))
        _holder_filled(h, dx)
    _conv_launch_multi("dX", True, gs, lambda: _sk_launch(plan, gy4, wt16, None, dx, None, nb, st),
                       extra_bytes=2.0 * dx.numel() if nb is not None else 0.0, flops=fwd_flops, name=_sk_name(plan) + " bf16", esz=2)
    return dx


def conv_weight_grad(x_cl, gy_cl, w, stride, pad):
    """Accumulate dW into ``w.grad`` (kernel layout)."""
    lib = _lib.load()
    if x_cl.dtype == torch.bfloat16 or gy_cl.dtype == torch.bfloat16:
        if x_cl.dtype == gy_cl.dtype and w.dim() == 4:
            x4 = x_cl
            g = conv_geom_for(x4.shape, w, stride, pad)
            plan = _sk_dw_plan(g, x4.device, _lib.BF16)
            if plan is not None:
                gw = grad_buffer(w)
                gws = weight_storage(gw)
                if gws.data_ptr() != gw.data_ptr():
                    raise RuntimeError("weight gradient is not in the (Cout,taps,Cin) kernel layout")
                st = _stream()
                ws = _sk_dw_workspace(x4.device, st)
                _conv_launch("dW", True, g, lambda: lib.sdt_convsk_dw_bf16(_p(x4), _p(gy_cl), _p(gws), plan.host, _p(plan.dev), _p(ws),
                                                                           x4.numel() * 2, gy_cl.numel() * 2, st), name="convbf_dw_kernel", esz=2)
                return
        x_cl, gy_cl = x_cl.float(), gy_cl.float()  # no bf16 kernel for this layer: fp32 path
    x4, gy4 = _as4(x_cl), _as4(gy_cl)
    g = conv_geom_for(x4.shape, w, stride, pad)
    gw = grad_buffer(w)
    gws = weight_storage(gw)
    if gws.data_ptr() != gw.data_ptr():
        raise RuntimeError("weight gradient is not in the (Cout,taps,Cin) kernel layout")
    st = _stream()
    if USE_STREAMK_DW and w.dim() == 4 and _CONV_MATH_NOW[0] == 0:
        plan = _sk_dw_plan(g, x4.device)
        if plan is not None:
            ws = _sk_dw_workspace(x4.device, st)
            _conv_launch("dW", True, g, lambda: lib.sdt_convsk_dw_f32(_p(x4), _p(gy4), _p(gws), plan.host, _p(plan.dev), _p(ws),
                                                                      x4.numel() * 4, gy4.numel() * 4, st),
                         name="convx3_dw_kernel" if (plan.host[3] >> 26) & 1 else "convsk_dw_kernel")
            return
    if DETERMINISTIC_DW and _CONV_MATH_NOW[0] == 0 and g.ntaps == g.Tw:  # (the bf16 modes have no ordered variant: atomics)
        nbytes = lib.sdt_conv_dw_workspace_bytes(g)
        ws = torch.empty(nbytes // 4, device=x4.device, dtype=torch.float32)  # on the launching stream: freed blocks are reused in order
        _conv_launch("dW", w.dim() == 4, g, lambda: lib.sdt_conv_dw_det_f32(_p(x4), _p(gy4), _p(gws), g, _p(ws), nbytes, st))
        return
    _conv_launch("dW", w.dim() == 4, g, lambda: lib.sdt_conv_dw_f32(_p(x4), _p(gy4), _p(gws), g, st))


# Weight gradients are off the backward critical path (only the optimiser consumes them): with OVERLAP_DW they are
# launched on a side HIP stream, concurrently with the input-gradient / normalisation chain on the main stream, so the
# two fill each other's launch tails (the 1060-workgroup layers leave 17 % of the CUs idle at the end of a launch) and
# the latency-bound 1-D launches: +4 % on the train step.  join_side_stream() is called before the gradient exchange /
# optimiser step.
OVERLAP_DW = True
OVERLAP_DW_MIN_FLOPS = 4e9
# Bit-reproducible weight gradients (the reference sets cudnn.deterministic = True, main.py:37-38): the 2-D layers with Cout % 128 == 0
# go through the stream-K weight gradient (sdt_convsk_dw_f32, ordered slab reduce, as fast as the atomics kernel), every other layer
# through row-range slabs + an ordered reduce (sdt_conv_dw_det_f32, -0.9 % on the step when it carried all layers,
# profiles/r02_deterministic_dw.txt).  False: fp32 atomics (the round-1/2 default).
DETERMINISTIC_DW = True
_SIDE = {}


CAPTURE_SIDE_STREAMS = False  # experiment: fork / join the side streams inside a hipGraph capture as well


def _side_ok():
    return CAPTURE_SIDE_STREAMS or not torch.cuda.is_current_stream_capturing()


def _side_stream(which=0):
    key = (torch.cuda.current_device(), which)
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=key[0])
    return _SIDE[key]


PAIR_AUX = True     # the two no-grad pose-encoder passes of a train step as one pass over the concatenated batch (PoseSeqEncoder.forward_pair)
OVERLAP_AUX = True  # the no-grad pose-encoder passes of a train step run on the side stream (voice2pose.py); a stream of their own: no change (r04)


class side_stream_scope:
    """``with side_stream_scope(enabled):`` runs the body on the side stream (after everything queued on the main
    stream so far) when OVERLAP_AUX is on and ``enabled``; otherwise it is a no-op."""

    def __init__(self, enabled=True):
        self.on = bool(enabled and OVERLAP_AUX and torch.cuda.is_available() and _side_ok())
        self.ctx = None

    def __enter__(self):
        if self.on:
            self.side = _side_stream()
            self.side.wait_stream(torch.cuda.current_stream())
            self.ctx = torch.cuda.stream(self.side)
            self.ctx.__enter__()
        return self

    def uses(self, *tensors):
        if self.on:
            for t in tensors:
                if t is not None and t.is_cuda:
                    t.record_stream(self.side)  # produced on the main stream, consumed here

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


# The 1-D stage's weight-gradient launches (15 of 10-20 us, latency-bound) are too short to be worth a pair of cross-stream
# events each, but nothing on the backward chain needs them either: while deferral is on (a train step that promises to
# flush) they are only recorded, and ``flush_deferred_dw`` enqueues all of them behind ONE event on the side stream --
# from the hook that fires when backward reaches the audio encoder, so they run under the long Conv2d backward instead
# of between the 1-D stage's input-gradient launches.
DEFER_SMALL_DW = True
_DEFERRED = []  # (x_cl, gy, w, stride, pad)
_DEFER_ON = [False]


def defer_small_dw(on):
    # (also without a side stream -- inside a hipGraph capture: the batch then runs on the capturing stream, still as ONE grouped launch)
    _DEFER_ON[0] = bool(on) and DEFER_SMALL_DW and torch.cuda.is_available()


GROUP_DW = True   # the deferred small weight gradients of a step in one grouped launch + one ordered reduce (sdt_conv_dw_group_f32)
_DW_GROUPS = {}   # (geometry bytes ..., device) -> (host plan, device plan, workspace, n)


def _dw_group_launch(items):
    """``items``: [(x4, gy4, gradient storage, geometry)], 2..24 of them, fp32, every geometry one the deterministic weight gradient takes."""
    import ctypes as C
    lib = _lib.load()
    dev = items[0][0].device
    key = tuple(_geom_key(it[3]) for it in items) + (dev.index,)
    grp = _DW_GROUPS.get(key)
    n = len(items)
    if grp is None:
        nbytes = lib.sdt_conv_dw_group_plan_bytes(n)
        host = (C.c_int32 * (nbytes // 4))()
        garr = (C.POINTER(_lib.ConvGeom) * n)(*[C.pointer(it[3]) for it in items])
        wsb = C.c_int64(0)
        check(lib.sdt_conv_dw_group_plan(garr, n, C.addressof(host), C.byref(wsb)))
        grp = _DW_GROUPS[key] = (host, torch.frombuffer(host, dtype=torch.int32).to(dev), torch.empty(wsb.value // 4, device=dev, dtype=torch.float32))
    host, plan_dev, ws = grp
    xs = (C.c_void_p * n)(*[it[0].data_ptr() for it in items])
    dys = (C.c_void_p * n)(*[it[1].data_ptr() for it in items])
    dws = (C.c_void_p * n)(*[it[2].data_ptr() for it in items])
    st = _stream()
    call = lambda: lib.sdt_conv_dw_group_f32(xs, dys, dws, n, C.addressof(host), _p(plan_dev), _p(ws), st)  # noqa: E731
    if PROFILER is None or (PROFILER.only is not None and "conv_dw_group_kernel" not in PROFILER.only):
        check(call())
        return
    flops = sum(2.0 * g.B * g.Ho * g.Wo * g.Cout * g.ntaps * g.Cin for _x, _y, _w, g in items)
    nbytes = sum(4.0 * (g.B * g.Hi * g.Wi * g.Cin + g.B * g.Ho * g.Wo * g.Cout + g.Cout * g.ntaps * g.Cin) for _x, _y, _w, g in items)
    e0, e1 = PROFILER.event(), PROFILER.event()
    e0.record()
    check(call())
    e1.record()
    PROFILER.records.append(("conv_dw_group_kernel", "dW", False, flops, nbytes, e0, e1))


def _launch_weight_grads(jobs):
    """[(x_cl, gy, w, stride, pad)]: the small fp32 layers the ordered slab kernel would take go into grouped launches, the rest one by one."""
    group, gjobs, rest = [], [], []
    for job in jobs:
        x_cl, gy, w, stride, pad = job
        ok = (GROUP_DW and DETERMINISTIC_DW and _CONV_MATH_NOW[0] == 0 and x_cl.dtype == torch.float32 and gy.dtype == torch.float32
              and not (USE_STREAMK_DW and w.dim() == 4))
        if ok:
            x4, gy4 = _as4(x_cl.contiguous()), _as4(gy.contiguous())
            g = conv_geom_for(x4.shape, w, stride, pad)
            gw = grad_buffer(w)
            gws = weight_storage(gw)
            ok = (g.ntaps == g.Tw and g.Cin % 4 == 0 and g.Cout % 4 == 0 and gws.data_ptr() == gw.data_ptr()
                  and (x4.data_ptr() | gy4.data_ptr() | gws.data_ptr()) % 16 == 0)
            if ok:
                group.append((x4, gy4, gws, g))
                gjobs.append(job)
                continue
        rest.append(job)
    for i in range(0, len(group), 24):
        if len(group[i:i + 24]) >= 2:
            _dw_group_launch(group[i:i + 24])
        else:  # nothing to share a grid with
            rest.append(gjobs[i])
    for x_cl, gy, w, stride, pad in rest:
        conv_weight_grad(x_cl, gy, w, stride, pad)


def flush_deferred_dw():
    if not _DEFERRED:
        return
    if not (OVERLAP_DW and _side_ok()):  # no side stream (hipGraph capture, --no-overlap-dw): the batch runs here
        stage_mark("dw1d:begin")
        _launch_weight_grads(list(_DEFERRED))
        stage_mark("dw1d:end")
        _DEFERRED.clear()
        return
    side = _side_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        stage_mark("dw1d:begin")
        _launch_weight_grads(list(_DEFERRED))
        stage_mark("dw1d:end")
    for x_cl, gy, _w, _s, _p2 in _DEFERRED:
        gy.record_stream(side)
        x_cl.record_stream(side)
    _DEFERRED.clear()


def side_stream_if_any():
    return _SIDE.get((torch._C._cuda_getDevice(), 0))


# autograd's contract: when backward() returns, every .grad is ready on the stream backward ran on.  Weight gradients launched on the side stream
# (or deferred) break it unless that stream is joined when the backward pass ends: _conv_backward queues ONE engine callback per pass for that.
# (The train step joined before its optimiser anyway; a stand-alone `loss.backward(); torch_optimizer.step()` on these modules did not.)
_JOIN_QUEUED = [-1]  # id of the backward pass (autograd graph task) whose end-of-pass join has been queued


def _end_of_backward():
    join_side_stream()


def _queue_backward_join():
    """One engine callback per backward PASS.  Keyed on the pass's id, not on a flag the callback clears: the engine runs no final callbacks for a
    pass that raised, and a latched flag would then silently drop the join of every later pass."""
    tid = torch._C._current_graph_task_id()
    if tid < 0 or tid == _JOIN_QUEUED[0]:
        return  # not inside a backward pass (a direct call of the op: the caller joins), or already queued for this pass
    try:
        torch.autograd.Variable._execution_engine.queue_callback(_end_of_backward)
        _JOIN_QUEUED[0] = tid
    except RuntimeError:
        pass


def join_side_stream():
    if _DEFERRED:
        flush_deferred_dw()
    if not _SIDE:
        return
    dev = torch._C._cuda_getDevice()
    for (d, _which), st in _SIDE.items():
        if d == dev:
            torch.cuda.current_stream().wait_stream(st)


class ConvFn(torch.autograd.Function):
    """nn.Conv1d/nn.Conv2d (building_blocks.py:15-22,31-38; generator.py:103) on channels-last tensors."""

    @staticmethod
    def forward(ctx, x_cl, w, bias, stride, pad, in_holder=None):
        x_cl = x_cl.contiguous()
        ctx.save_for_backward(x_cl, w, bias)
        ctx.stride, ctx.pad, ctx.in_holder = stride, pad, in_holder
        return conv_forward(x_cl, w, bias, stride, pad)

    @staticmethod
    def backward(ctx, gy):
        x_cl, w, bias = ctx.saved_tensors
        return (_conv_backward(x_cl, w, bias, gy.contiguous(), ctx.stride, ctx.pad, ctx.needs_input_grad[0], ctx.in_holder),
                None, None, None, None, None)


def _conv_backward(x_cl, w, bias, gy, stride, pad, need_dx, in_holder=None):
    """Weight / bias gradients accumulated into ``.grad``; returns dX (or None)."""
    if w.requires_grad:
        # only launches long enough to pay for the cross-stream events: on the 1-D stage's 10-20 us kernels the
        # side stream costs more than it hides (pose2pose: -11 %)
        big = 2.0 * gy.numel() * x_cl.shape[-1] * (w.numel() // (w.shape[0] * w.shape[1])) >= OVERLAP_DW_MIN_FLOPS
        if OVERLAP_DW and big and _side_ok():
            side = _side_stream()
            side.wait_stream(torch.cuda.current_stream())  # gy (and x) are produced on the main stream
            with torch.cuda.stream(side):
                conv_weight_grad(x_cl, gy, w, stride, pad)
            gy.record_stream(side)  # keep the caching allocator from recycling gy under the side stream
            x_cl.record_stream(side)
            _queue_backward_join()
        elif _DEFER_ON[0] and not big:
            _DEFERRED.append((x_cl, gy, w, stride, pad))
            _queue_backward_join()
        else:
            conv_weight_grad(x_cl, gy, w, stride, pad)
    if bias is not None and bias.requires_grad:
        gb = grad_buffer(bias)
        check(_lib.load().sdt_col_sum_f32(_p(gy), _p(gb), gy.numel() // gy.shape[-1], gy.shape[-1], _stream()))
    return conv_input_grad(gy, w, x_cl.shape, stride, pad, in_holder) if need_dx else None


class ConvStatsFn(torch.autograd.Function):
    """Bias-free forward conv whose epilogue also accumulates the per-(group, channel) sum / sum of squares of its output
    (sdt_conv_taps_stats_f32 / the stream-K kernel's EPI 1) -- the statistics pass of the InstanceNorm2d /
    BatchNorm that follows.  Returns (y, sums); ``sums`` goes to ColNormActFn(..., sums).  Use only when ``conv_stats_fusable``
    says so."""

    @staticmethod
    def forward(ctx, x_cl, w, stride, pad, groups, in_holder=None):
        _req_cuda(x_cl, w)
        lib = _lib.load()
        x_cl = x_cl.contiguous()
        ctx.in_holder = in_holder
        g = conv_geom_for(x_cl.shape, w, stride, pad)
        sums = _ARENA.take(2 * groups * g.Cout, x_cl.device)
        rpg = g.B * g.Ho * g.Wo // groups
        st = _stream()
        if x_cl.dtype == torch.bfloat16:  # bf16-storage path (conv_stats_fusable has checked that the plan exists)
            y = torch.empty((g.B, g.Ho, g.Wo, g.Cout), device=x_cl.device, dtype=torch.bfloat16)
            w16 = _bf16_weights(w)[0]
            plan = _sk_plan(g, 1, rpg, 1, x_cl.device, forward=True, dtype=_lib.BF16)
            _conv_launch("fwd", True, g, lambda: _sk_launch(plan, x_cl, w16, None, y, sums, None, st), name=_sk_name(plan) + " bf16", esz=2)
        else:
            y = torch.empty((g.B, g.Ho, g.Wo, g.Cout), device=x_cl.device, dtype=torch.float32)
            ws = weight_storage(w)
            plan = _sk_plan(g, 1, rpg, 1, x_cl.device, forward=True) if (USE_STREAMK and _CONV_MATH_NOW[0] == 0 and rpg >= 32) else None
            if plan is not None:
                _conv_launch("fwd", True, g, lambda: _sk_launch(plan, x_cl, ws, None, y, sums, None, st), name=_sk_name(plan))
            else:
                _conv_launch("fwd", True, g, lambda: lib.sdt_conv_taps_stats_f32(_p(x_cl), _p(ws), None, _p(y), g, _p(sums), rpg, st))
        ctx.save_for_backward(x_cl, w)
        ctx.stride, ctx.pad = stride, pad
        ctx.mark_non_differentiable(sums)
        ctx.set_materialize_grads(False)  # no zero-filled float64 "gradient" of sums in backward (one fill launch per layer)
        return y, sums

    @staticmethod
    def backward(ctx, gy, _gsums):
        x_cl, w = ctx.saved_tensors
        return (_conv_backward(x_cl, w, None, gy.contiguous(), ctx.stride, ctx.pad, ctx.needs_input_grad[0], ctx.in_holder),
                None, None, None, None, None)


def conv_stats_fusable(x_cl, w, stride, pad, groups):
    """True when the conv + column-norm pair can use the fused-statistics epilogue (2-D, dense geometry, Cin % 32 == 0, exact
    fp32 math, no split-K, groups dividing the batch)."""
    if x_cl.dim() != 4 or w.dim() != 4 or PROFILER_NO_FUSION:
        return False
    g = conv_geom_for(x_cl.shape, w, stride, pad)
    if x_cl.dtype == torch.bfloat16:  # bf16-storage path: the stream-K kernel is the only one, its plan must exist for this geometry
        m = g.B * g.Ho * g.Wo
        return m % groups == 0 and m // groups >= 32 and _sk_plan(g, 1, m // groups, 1, x_cl.device, forward=True, dtype=_lib.BF16) is not None
    key = (groups, _CONV_MATH_NOW[0])  # the library's answer depends on the product arithmetic in force
    ok = getattr(g, "_stats_ok", None)
    if ok is None or ok[0] != key:
        m = g.B * g.Ho * g.Wo
        ok = g._stats_ok = (key, bool(m % groups == 0 and _lib.load().sdt_conv_taps_stats_supported(g, m // groups)))
    return ok[1]


PROFILER_NO_FUSION = False  # experiments: force the unfused conv -> colstats -> apply sequence


class ConvRowNormFn(torch.autograd.Function):
    """ConvNormRelu('1d', norm='IN') in one autograd node (building_blocks.py:31-51): Conv1d (no bias) -> per-(b,t) norm
    over channels -> LeakyReLU.  When the conv is K-split (the 1-D stage: too few output tiles for 256 CUs) the slab
    reduction is done by the normalisation kernel (sdt_rownorm_slabs_fwd_f32): two launches instead of three, same
    summation order as conv -> splitk_reduce -> rownorm."""

    @staticmethod
    def forward(ctx, x_cl, w, stride, pad, slope):
        _req_cuda(x_cl, w)
        lib = _lib.load()
        x_cl = x_cl.contiguous()
        x4 = _as4(x_cl)
        g = conv_geom_for(x4.shape, w, stride, pad)
        k = _splitk_hint(lib, g)
        ws = weight_storage(w)
        st = _stream()
        dev = x_cl.device
        y = torch.empty((g.B, g.Ho, g.Wo, g.Cout), device=dev, dtype=torch.float32)
        z = torch.empty_like(y)
        rows, C = g.B * g.Ho * g.Wo, g.Cout
        mean = torch.empty(rows, device=dev, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        if k > 1:
            part = torch.empty((k,) + tuple(y.shape), device=dev, dtype=torch.float32)
            _conv_launch("fwd", w.dim() == 4, g, lambda: lib.sdt_conv_taps_splitk_f32(_p(x4), _p(ws), None, _p(y), g, k, _p(part), st))
            check(lib.sdt_rownorm_slabs_fwd_f32(_p(part), k, _p(y), _p(z), _p(mean), _p(rstd), rows, C, BN_EPS, slope, st))
        else:
            _conv_launch("fwd", w.dim() == 4, g, lambda: lib.sdt_conv_taps_f32(_p(x4), _p(ws), None, _p(y), g, st))
            check(lib.sdt_rownorm_fwd_f32(_p(y), _p(z), _p(mean), _p(rstd), rows, C, BN_EPS, slope, st))
        if x_cl.dim() == 3:
            y, z = y.squeeze(1), z.squeeze(1)
        ctx.save_for_backward(x_cl, w, y, mean, rstd)
        ctx.stride, ctx.pad, ctx.slope = stride, pad, slope
        return z

    @staticmethod
    def backward(ctx, gz):
        x_cl, w, y, mean, rstd = ctx.saved_tensors
        gz = gz.contiguous()
        C = y.shape[-1]
        gy = torch.empty_like(y)
        check(_lib.load().sdt_rownorm_bwd_f32(_p(gz), _p(y), _p(mean), _p(rstd), _p(gy), y.numel() // C, C, ctx.slope, _stream()))
        return _conv_backward(x_cl, w, None, gy, ctx.stride, ctx.pad, ctx.needs_input_grad[0]), None, None, None, None


class ColNormActFn(torch.autograd.Function):
    """InstanceNorm2d (groups = batch) or training-mode BatchNorm (groups = 1) + LeakyReLU/ReLU."""

    @staticmethod
    def forward(ctx, y, gamma, beta, rmean, rvar, nbt, groups, slope, sums=None, holder=None, out_f32=False):
        """``y`` fp32 or bf16 (bf16-storage path); ``z`` has y's element type unless ``out_f32`` (the block that feeds the fp32 1-D stage)."""
        _req_cuda(y)
        lib = _lib.load()
        y = y.contiguous()
        C = y.shape[-1]
        R = y.numel() // C // groups
        z = torch.empty_like(y, dtype=torch.float32) if out_f32 else torch.empty_like(y)
        ready = sums is not None  # accumulated by the producing conv's epilogue (ConvStatsFn)
        if not ready:
            sums = _ARENA.take(2 * groups * C, y.device)
        mean = torch.empty(groups * C, device=y.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        check(lib.sdt_colnorm_fwd_t(_p(y), _dt(y), _p(z), _dt(z), _p(sums), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(rmean), _p(rvar),
                                    _p(nbt), groups, R, C, BN_EPS, BN_MOMENTUM, slope, int(ready), _stream()))
        ctx.save_for_backward(y, mean, rstd, gamma, beta)
        ctx.groups, ctx.slope, ctx.holder = groups, slope, holder
        if holder is not None:  # what the consuming conv's input-gradient epilogue needs (NormBwdHolder)
            holder.y, holder.mean, holder.rstd, holder.gamma, holder.beta = y, mean, rstd, gamma, beta
            holder.groups, holder.slope, holder.sums = groups, slope, None
        return z

    @staticmethod
    def backward(ctx, gz):
        y, mean, rstd, gamma, beta = ctx.saved_tensors
        lib = _lib.load()
        gz = gz.contiguous()
        C = y.shape[-1]
        R = y.numel() // C // ctx.groups
        if y.dtype == torch.float32 and gz.dtype != torch.float32:
            gz = gz.float()  # (an fp32 block after a bf16 one: not a combination the kernels are built for)
        dy = torch.empty_like(y)  # the element type of y: the conv below reads it with the same type as its saved input
        h = ctx.holder
        # accumulated by the epilogue of the conv that produced gz -- trusted only if gz IS that launch's output tensor
        ready = h is not None and h.sums is not None and _holder_grad_matches(h, gz)
        if h is not None and h.sums is not None:
            HOLDER_HANDOVERS["used" if ready else "refused"] += 1
        sums = h.sums if ready else _ARENA.take(2 * ctx.groups * C, y.device)
        if h is not None:
            h.sums = h.dx_id = None
        dg = grad_buffer(gamma) if gamma is not None and gamma.requires_grad else None
        db = grad_buffer(beta) if beta is not None and beta.requires_grad else None
        check(lib.sdt_colnorm_bwd_t(_p(gz), _dt(gz), _p(y), _dt(y), _p(dy), _dt(dy), _p(sums), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dg), _p(db),
                                    ctx.groups, R, C, ctx.slope, int(ready), _stream()))
        return dy, None, None, None, None, None, None, None, None, None, None


class L0BlockFn(torch.autograd.Function):
    """Conv2d(1,64,k3,s1,p1) + InstanceNorm2d | BatchNorm2d(train) + LeakyReLU in one pass over the 64-channel output
    (first block of the audio encoder, generator.py:16).  mel (B,H,W) -> z (B,H,W,64) channels-last."""

    @staticmethod
    def forward(ctx, mel, w, gamma, beta, rmean, rvar, nbt, groups, slope, holder=None):
        _req_cuda(mel, w)
        lib = _lib.load()
        mel = mel.contiguous()
        B, H, W = mel.shape
        ws = weight_storage(w)
        # the first tensor of the bf16-storage path: written as bf16 when ops.STORAGE says so
        z = torch.empty((B, H, W, 64), device=mel.device, dtype=torch.bfloat16 if STORAGE == "bf16" else torch.float32)
        # zero on entry; read again by this step's backward (an arena slice is not handed out twice within a step, and
        # the arena is only recycled by the next step's begin_step)
        mom = _ARENA.take(54 * B, mel.device)
        mean = torch.empty(groups * 64, device=mel.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        check(lib.sdt_l0_block_fwd_t(_p(mel), _p(ws), _p(z), _dt(z), _p(mom), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(rmean),
                                     _p(rvar), _p(nbt), B, H, W, groups, BN_EPS, BN_MOMENTUM, slope, _stream()))
        ctx.save_for_backward(mel, w, mean, rstd, gamma, beta, mom)
        ctx.groups, ctx.slope = groups, slope
        return z

    @staticmethod
    def backward(ctx, gz):
        mel, w, mean, rstd, gamma, beta, mom = ctx.saved_tensors
        lib = _lib.load()
        gz = gz.contiguous()
        B, H, W = mel.shape
        sums = _ARENA.take(11 * ctx.groups * 64, mel.device)
        gw = grad_buffer(w)
        if weight_storage(gw).data_ptr() != gw.data_ptr():
            raise RuntimeError("weight gradient is not in the (Cout,taps,Cin) kernel layout")
        dg = grad_buffer(gamma) if gamma is not None and gamma.requires_grad else None
        db = grad_buffer(beta) if beta is not None and beta.requires_grad else None
        check(lib.sdt_l0_block_bwd_t(_p(gz), _dt(gz), _p(mel), _p(weight_storage(w)), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(mom), _p(sums),
                                     _p(gw), _p(dg), _p(db), B, H, W, ctx.groups, ctx.slope, _stream()))
        return None, None, None, None, None, None, None, None, None, None


def colnorm_eval(y, gamma, beta, rmean, rvar, slope):
    lib = _lib.load()
    y = y.contiguous()
    z = torch.empty_like(y)
    C = y.shape[-1]
    check(lib.sdt_colnorm_eval_f32(_p(y), _p(z), _p(gamma), _p(beta), _p(rmean), _p(rvar), y.numel() // C, C, BN_EPS, slope,
                                   _stream()))
    return z


class RowNormActFn(torch.autograd.Function):
    """InstanceNorm1d over the permuted tensor == LayerNorm over C per (b,t), no affine (building_blocks.py:50-51)."""

    @staticmethod
    def forward(ctx, y, slope):
        _req_cuda(y)
        lib = _lib.load()
        y = y.contiguous()
        C = y.shape[-1]
        rows = y.numel() // C
        z = torch.empty_like(y)
        mean = torch.empty(rows, device=y.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        check(lib.sdt_rownorm_fwd_f32(_p(y), _p(z), _p(mean), _p(rstd), rows, C, BN_EPS, slope, _stream()))
        ctx.save_for_backward(y, mean, rstd)
        ctx.slope = slope
        return z

    @staticmethod
    def backward(ctx, gz):
        y, mean, rstd = ctx.saved_tensors
        gz = gz.contiguous()
        C = y.shape[-1]
        dy = torch.empty_like(y)
        check(_lib.load().sdt_rownorm_bwd_f32(_p(gz), _p(y), _p(mean), _p(rstd), _p(dy), y.numel() // C, C, ctx.slope, _stream()))
        return dy, None


_ROW_INDEX = {}


def _row_index(n, dev):
    """arange(n) on ``dev`` (int64), created once per (n, device): read-only."""
    key = (n, dev.type, dev.index)
    if key not in _ROW_INDEX:
        _ROW_INDEX[key] = torch.arange(n, device=dev, dtype=torch.int64)
    return _ROW_INDEX[key]


class ResizeConcatFn(torch.autograd.Function):
    """F.interpolate(x,(1,T),'bilinear').squeeze(2) ++ code (generator.py:41-42,110-111), channels-last."""

    @staticmethod
    def forward(ctx, x_cl, code, T):
        _req_cuda(x_cl, code)
        lib = _lib.load()
        x_cl = x_cl.contiguous()
        B, H, W, C = x_cl.shape
        # resize_concat_fwd_kernel reads row b of ``code`` for clip b without a bound check: the shape is checked here
        if code is not None and (code.dim() != 2 or code.shape[0] != B):
            raise ValueError("ResizeConcatFn needs one code row per clip: code %s for %d clips" % (tuple(code.shape), B))
        D = 0 if code is None else code.shape[1]
        idx = None
        if code is not None:
            code = code.contiguous()
            idx = _row_index(B, x_cl.device)
        out = torch.empty((B, T, C + D), device=x_cl.device, dtype=torch.float32)
        check(lib.sdt_resize_concat_fwd_f32(_p(x_cl), _p(code), _p(idx), _p(out), B, H, W, C, T, D, _stream()))
        ctx.dims = (B, H, W, C, T, D)
        ctx.save_for_backward(idx)
        return out

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        B, H, W, C, T, D = ctx.dims
        g = g.contiguous()
        dx = torch.empty((B, H, W, C), device=g.device, dtype=torch.float32)
        dcode = torch.zeros((B, D), device=g.device, dtype=torch.float32) if D and ctx.needs_input_grad[1] else None
        check(_lib.load().sdt_resize_concat_bwd_f32(_p(g), _p(idx) if dcode is not None else None, _p(dx), _p(dcode),
                                                     B, H, W, C, T, D, _stream()))
        return dx, dcode, None


class UpsampleAddFn(torch.autograd.Function):
    """F.interpolate(prev, To, 'linear') (+ skip) (generator.py:79-83, autoencoder.py:62-66), channels-last."""

    @staticmethod
    def forward(ctx, prev, skip, To):
        _req_cuda(prev, skip)
        prev = prev.contiguous()
        B, Ti, C = prev.shape
        if skip is not None:
            skip = skip.contiguous()
        out = torch.empty((B, To, C), device=prev.device, dtype=torch.float32)
        check(_lib.load().sdt_upsample_add_fwd_f32(_p(prev), _p(skip), _p(out), B, Ti, To, C, _stream()))
        ctx.dims = (B, Ti, To, C)
        return out

    @staticmethod
    def backward(ctx, g):
        B, Ti, To, C = ctx.dims
        g = g.contiguous()
        dprev = torch.empty((B, Ti, C), device=g.device, dtype=torch.float32)
        check(_lib.load().sdt_upsample_add_bwd_f32(_p(g), _p(dprev), B, Ti, To, C, _stream()))
        return dprev, (g if ctx.needs_input_grad[1] else None), None


# ---------------------------------------------------------------------------------------------
# The generator's Conv1d stage as ONE persistent launch per direction (csrc/chain1d.hip): 8 workgroups per clip, raw conv outputs handed from
# block to block inside the launch, normalisation + activation (+ upsampling + skip) applied by the consumer on load.
CHAIN1D = True
# product arithmetic of the chain launches: None = follow the storage mode (exact fp32 with fp32 storage; products of bf16-rounded operands on the
# bf16 MFMA in a bf16-storage run, like its Conv2d chain: BASELINE config 4), or 'f32' / 'bf16' to pin it
CHAIN_MATH = None


def chain_math():
    mode = CHAIN_MATH if CHAIN_MATH is not None else STORAGE
    return CONV_MATH['bf16'] if mode == 'bf16' else CONV_MATH['f32']

_CHAIN_WS = {}  # device index -> int32 [64 cluster counters | error word]
_CHAIN_ERR = 64


def _chain_ws(dev):
    ws = _CHAIN_WS.get(dev.index)
    if ws is None:
        ws = _CHAIN_WS[dev.index] = torch.zeros(_CHAIN_ERR + 64, device=dev, dtype=torch.int32)  # zero-filled once: a launch leaves its counters at zero
    return ws


def chain_blocks(spec, T0, Cin0):
    """[(Ti, To, Cin, k, stride, pad, in_mode, src_a, src_b)] of a chain whose blocks are ``spec`` = ((k, stride, pad, in_mode, src_a, src_b), ...)
    fed with (B, T0, Cin0); raises ValueError when the wiring is inconsistent."""
    out = []
    for l, (k, stride, pad, mode, sa, sb) in enumerate(spec):
        if mode == _lib.CHAIN_PLAIN:
            Ti, Cin = T0, Cin0
        elif mode == _lib.CHAIN_NORM:
            Ti, Cin = out[sa][1], 256
        else:
            Ti, Cin = out[sb][1], 256
        To = out_size(Ti, k, stride, pad)
        if To < 1:
            raise ValueError("block %d of the chain has no output frames" % l)
        out.append((Ti, To, Cin, k, stride, pad, mode, sa, sb))
    return out


def chain1d_usable(h, spec, weights):
    """The launch exists for this chain on this device: fp32 (B, T <= 64, Cin % 32 == 0) input, every block 256 wide with its weight in the kernel
    layout (a launch holds 32 clips on MI355X; larger batches run as consecutive launches inside the entry point)."""
    if not (CHAIN1D and h.is_cuda and h.dtype == torch.float32 and h.dim() == 3 and _CONV_MATH_NOW[0] == 0):
        return False
    B, T0, Cin0 = h.shape
    if T0 > 64 or Cin0 % 32 or Cin0 > 320 or len(spec) > 20 or len(spec) != len(weights):
        return False
    try:
        blocks = chain_blocks(spec, T0, Cin0)
    except (ValueError, IndexError):
        return False
    for (Ti, To, Cin, k, stride, pad, mode, sa, sb), w in zip(blocks, weights):
        if w.dim() != 3 or tuple(w.shape) != (256, Cin, k) or weight_storage(w).data_ptr() != w.data_ptr() or w.dtype != torch.float32:
            return False
    tab = (_lib.ChainLayer * len(blocks))(*[_lib.ChainLayer(Ti, To, Cin, k, stride, pad, mode, sa, sb, 0, 1, 0, 1, 0, 0, 0)
                                            for (Ti, To, Cin, k, stride, pad, mode, sa, sb) in blocks])
    return bool(_lib.load().sdt_chain1d_supported(tab, len(blocks), B))


def _chain_launch(name, kind, flops, nbytes, call):
    if PROFILER is None or (PROFILER.only is not None and name not in PROFILER.only):
        check(call())
        return
    e0, e1 = PROFILER.event(), PROFILER.event()
    e0.record()
    check(call())
    e1.record()
    PROFILER.records.append((name, kind, False, flops, nbytes, e0, e1))


class Chain1dFn(torch.autograd.Function):
    """A chain of ConvNormRelu('1d', norm='IN') blocks -- UNet_1D + the decoder stack, generator.py:53-85,96-103 -- in one launch per direction.
    ``spec``: ((k, stride, pad, in_mode, src_a, src_b), ...) per block (include/sdt_hip.h sdt_chain1d_layer); ``h`` (B, T, Cin) feeds block 0;
    returns the activated output of the last block (B, T_last, 256).  Weight gradients are accumulated into ``.grad`` by the usual launches
    (deferred to the side stream inside a train step), from the conv inputs / raw-output gradients the two launches leave in HBM."""

    @staticmethod
    def _slices(buf, sizes, shapes):
        out, o = [], 0
        for n, shp in zip(sizes, shapes):
            out.append(buf[o:o + n].view(shp))
            o += n
        return out

    @staticmethod
    def forward(ctx, h, spec, slope, *weights):
        _req_cuda(h, *weights)
        lib = _lib.load()
        h = h.contiguous()
        B, T0, Cin0 = h.shape
        math = ctx.math = chain_math()
        blocks = chain_blocks(spec, T0, Cin0)
        n = len(blocks)
        dev = h.device
        want_grad = any(ctx.needs_input_grad)  # (grad mode is off inside forward(): needs_input_grad is what says a backward may follow)
        need_dx0 = bool(ctx.needs_input_grad[0])
        ysz = [B * b[1] * 256 for b in blocks]
        ys = Chain1dFn._slices(torch.empty(sum(ysz), device=dev, dtype=torch.float32), ysz, [(B, b[1], 256) for b in blocks])
        xs = [None] * n
        if want_grad:
            xsz = [B * b[0] * 256 for b in blocks[1:]]
            xs = [None] + Chain1dFn._slices(torch.empty(sum(xsz), device=dev, dtype=torch.float32), xsz, [(B, b[0], 256) for b in blocks[1:]])
        zout = torch.empty((B, blocks[-1][1], 256), device=dev, dtype=torch.float32)
        wst = [weight_storage(w) for w in weights]
        tab = (_lib.ChainLayer * n)(*[_lib.ChainLayer(Ti, To, Cin, k, stride, pad, mode, sa, sb, 0, _p(wst[l]), None, _p(ys[l]), _p(xs[l]), None, None)
                                      for l, (Ti, To, Cin, k, stride, pad, mode, sa, sb) in enumerate(blocks)])
        ws = _chain_ws(dev)
        flops = sum(2.0 * B * To * 256 * k * Cin for (Ti, To, Cin, k, *_r) in blocks)
        nbytes = 4.0 * (h.numel() + zout.numel() + sum(w.numel() for w in weights))
        st = _stream()
        _chain_launch("chain1d_fwd_kernel" + (" bf16" if math else ""), "fwd", flops, nbytes,
                      lambda: lib.sdt_chain1d_fwd_f32(tab, n, _p(h), _p(zout), B, float(slope), BN_EPS, math, ws.data_ptr(), ws.data_ptr() + 4 * _CHAIN_ERR, st))
        ctx.blocks, ctx.slope, ctx.xs = blocks, float(slope), xs
        if want_grad:
            # everything backward() needs besides the gradient itself is prepared HERE: in a train step the host is about a millisecond ahead of
            # the GPU during the forward pass and level with it when the backward pass reaches this stage (its table-building showed as a gap of
            # the main stream in front of the launch).  The (Cin,taps,Cout) weight mirrors have stable addresses; backward() only asks for a refresh.
            dys = Chain1dFn._slices(torch.empty(sum(ysz), device=dev, dtype=torch.float32), ysz, [(B, b[1], 256) for b in blocks])
            dsz = [B * b[0] * b[2] for b in blocks]
            dxs = Chain1dFn._slices(torch.empty(sum(dsz), device=dev, dtype=torch.float32), dsz, [(B, b[0], b[2]) for b in blocks])
            wts = []
            for l, w in enumerate(weights):
                wt = None
                if l or need_dx0:
                    _owner, e = WeightMirrors._entry(w)
                    # no optimiser group mirrors this weight: transposed per call in backward()
                    wt = e[1] if e is not None else torch.empty((blocks[l][2], blocks[l][3], 256), device=dev, dtype=torch.float32)
                wts.append(wt)
            ctx.dys, ctx.dxs, ctx.wts = dys, dxs, wts
            ctx.btab = (_lib.ChainLayer * n)(*[_lib.ChainLayer(Ti, To, Cin, k, stride, pad, mode, sa, sb, 0, _p(wst[l]), _p(wts[l]), _p(ys[l]), _p(xs[l]),
                                                               _p(dys[l]), _p(dxs[l]))
                                               for l, (Ti, To, Cin, k, stride, pad, mode, sa, sb) in enumerate(blocks)])
            ctx.bflops = sum(2.0 * B * To * 256 * k * Cin for l, (Ti, To, Cin, k, *_r) in enumerate(blocks) if l or need_dx0)
            ctx.bbytes = 4.0 * (zout.numel() + 2 * sum(ysz) + sum(w.numel() for w in weights))
        ctx.save_for_backward(h, ys[0]._base, *weights)
        return zout

    @staticmethod
    def backward(ctx, gz):
        h = ctx.saved_tensors[0]
        weights = ctx.saved_tensors[2:]
        lib = _lib.load()
        blocks, xs, dys, dxs = ctx.blocks, ctx.xs, ctx.dys, ctx.dxs
        n = len(blocks)
        B = h.shape[0]
        gz = gz.contiguous()
        st = _stream()
        need_dx0 = bool(ctx.needs_input_grad[0])
        for l, w in enumerate(weights):
            if ctx.wts[l] is None:
                continue
            wt = WeightMirrors.lookup(w)  # refreshes the optimiser group's mirrors when they are stale (one batched launch for all of them)
            if wt is None:
                check(lib.sdt_weight_transpose_f32(_p(weight_storage(w)), _p(ctx.wts[l]), 256, blocks[l][3], blocks[l][2], st))
            elif wt.data_ptr() != ctx.wts[l].data_ptr():
                raise RuntimeError("the weight mirrors were rebuilt between forward and backward")
        ws = _chain_ws(h.device)
        tab = ctx.btab
        _chain_launch("chain1d_bwd_kernel" + (" bf16" if ctx.math else ""), "dX", ctx.bflops, ctx.bbytes,
                      lambda: lib.sdt_chain1d_bwd_f32(tab, n, _p(gz), B, ctx.slope, BN_EPS, int(need_dx0), ctx.math, ws.data_ptr(), ws.data_ptr() + 4 * _CHAIN_ERR, st))
        for l, (b, w) in enumerate(zip(blocks, weights)):  # weight gradients: the per-block launches, deferred to the side stream inside a train step
            if w.requires_grad:
                _conv_backward(h if l == 0 else xs[l], w, None, dys[l], b[4], b[5], False)
        return (dxs[0] if need_dx0 else None, None, None) + (None,) * n


class L1LossFn(torch.autograd.Function):
    """(nn.L1Loss(reduction='none')(pred, gt) * lambda).mean()  (voice2pose.py:141-142)."""

    @staticmethod
    def forward(ctx, pred, gt, lam):
        _req_cuda(pred, gt)
        pred, gt = pred.contiguous(), gt.contiguous()
        partial = torch.empty(256, device=pred.device, dtype=torch.float64)
        loss = torch.empty((), device=pred.device, dtype=torch.float32)
        check(_lib.load().sdt_l1_loss_fwd_f32(_p(pred), _p(gt), pred.numel(), lam, _p(partial), _p(loss), _stream()))
        ctx.save_for_backward(pred, gt)
        ctx.lam = lam
        return loss

    @staticmethod
    def backward(ctx, gout):
        pred, gt = ctx.saved_tensors
        dp = torch.empty_like(pred)
        gout = gout.contiguous()
        check(_lib.load().sdt_l1_loss_bwd_f32(_p(pred), _p(gt), _p(gout), pred.numel(), ctx.lam, _p(dp), _stream()))
        return dp, None, None


class RegLossFn(torch.autograd.Function):
    """L1LossFn with a confidence mask, per-channel weights and a velocity term (csrc/reg_loss.hip):
    (reg, vel) = (lam_reg * sum(m w |e|) / max(sum m, 1), lam_vel * sum(m2 w |d|) / max(sum m2, 1)) with e = pred - gt on (B, T, ...),
    d its first difference over T, m = score > min_conf (score None: 1), m2 the product of a pair's two m, w = chan_w per trailing
    element (None: 1).  Two launches forward, one backward; the divisors stay on the device."""

    @staticmethod
    def forward(ctx, pred, gt, score, chan_w, lam_reg, lam_vel, min_conf):
        _req_cuda(pred, gt)
        assert pred.dim() >= 3 and pred.shape == gt.shape and pred.dtype == gt.dtype == torch.float32
        pred, gt = pred.contiguous(), gt.contiguous()
        B, T = pred.shape[0], pred.shape[1]
        C = pred.numel() // (B * T)
        if score is not None:
            _req_cuda(score)
            assert score.shape == pred.shape and score.dtype == torch.float32 and min_conf is not None
            score = score.contiguous()
        if chan_w is not None:
            _req_cuda(chan_w)
            assert chan_w.shape == (C,) and chan_w.dtype == torch.float32 and chan_w.is_contiguous()
        dev = pred.device
        partial = torch.empty(512, device=dev, dtype=torch.float64)
        counts = torch.empty(512, device=dev, dtype=torch.int64)
        losses = torch.empty(2, device=dev, dtype=torch.float32)
        denom = torch.empty(2, device=dev, dtype=torch.float64)
        ctx.args = (B, T, C, float(lam_reg), float(lam_vel), 0.0 if score is None else float(min_conf))
        check(_lib.load().sdt_reg_loss_fwd_f32(_p(pred), _p(gt), _p(score), _p(chan_w), *ctx.args, _p(partial), _p(counts), _p(losses),
                                               _p(denom), _stream()))
        ctx.save_for_backward(pred, gt, score, chan_w, denom)
        ctx.set_materialize_grads(False)  # backward takes None for a loss that nothing consumed
        reg, vel = losses.unbind(0)
        return reg, vel

    @staticmethod
    def backward(ctx, g_reg, g_vel):
        pred, gt, score, chan_w, denom = ctx.saved_tensors
        if g_reg is None and g_vel is None:
            return (None,) * 7
        dp = torch.empty_like(pred)
        g_reg = None if g_reg is None else g_reg.contiguous()
        g_vel = None if g_vel is None else g_vel.contiguous()
        check(_lib.load().sdt_reg_loss_bwd_f32(_p(pred), _p(gt), _p(score), _p(chan_w), _p(g_reg), _p(g_vel), _p(denom), *ctx.args,
                                               _p(dp), _stream()))
        return (dp,) + (None,) * 6


def bone_incidence(edges, K):
    """CSR list of the edges incident to each of ``K`` keypoints: (inc_ptr[K + 1], inc_edge[2 E]), entry = 2 * e + (1 if the keypoint is
    edge e's first end, where the edge's gradient enters with a minus sign), edges ascending within a keypoint"""
    rows = [[] for _ in range(K)]
    for e, (a, b) in enumerate(edges):
        rows[a].append(2 * e + 1)
        rows[b].append(2 * e)
    ptr = [0]
    for r in rows:
        ptr.append(ptr[-1] + len(r))
    return ptr, [x for r in rows for x in r]


class BoneTable:
    """The skeleton a BoneLossFn call runs on: edges (E, 2), the part root of each of K keypoints (-1: none) and one weight per edge (None:
    1), validated ON THE HOST once -- K <= 256, E <= 512, indices inside [0, K), no edge from a keypoint to itself, a root that is itself in
    no part, finite weights >= 0 -- with the incidence and children lists backward gathers through.  ``on(device)`` uploads the tables once
    per device: no host-to-device copy inside a step, which a hipGraph capture would refuse."""
    MAX_K, MAX_E = 256, 512

    def __init__(self, edges, root, edge_w=None):
        edges = [(int(a), int(b)) for a, b in edges]
        root = [int(r) for r in root]
        K, E = len(root), len(edges)
        if not 0 < K <= self.MAX_K or E > self.MAX_E:
            raise ValueError("BoneTable: 0 < K <= %d keypoints and E <= %d edges are supported, got K = %d, E = %d"
                             % (self.MAX_K, self.MAX_E, K, E))
        for e, (a, b) in enumerate(edges):
            if not (0 <= a < K and 0 <= b < K) or a == b:
                raise ValueError("BoneTable: edge %d = (%d, %d) must join two different keypoints of [0, %d)" % (e, a, b, K))
        for k, r in enumerate(root):
            if r < -1 or r >= K or r == k:
                raise ValueError("BoneTable: root[%d] = %d must be -1 or another keypoint of [0, %d)" % (k, r, K))
            if r >= 0 and root[r] >= 0:
                raise ValueError("BoneTable: root[%d] = %d is itself in a part (root[%d] = %d): a root must be in no part" % (k, r, r, root[r]))
        if edge_w is not None:
            edge_w = [float(w) for w in edge_w]
            if len(edge_w) != E or not all(w >= 0 and w != float('inf') for w in edge_w):
                raise ValueError("BoneTable: edge_w must hold one finite weight >= 0 per edge, got %r" % (edge_w,))
        self.K, self.E, self.edges, self.root, self.edge_w = K, E, edges, root, edge_w
        self.inc_ptr, self.inc_edge = bone_incidence(edges, K)
        kids = [[j for j in range(K) if root[j] == k] for k in range(K)]
        self.child_ptr = [0]
        for c in kids:
            self.child_ptr.append(self.child_ptr[-1] + len(c))
        self.child_idx = [j for c in kids for j in c]
        self._dev = {}

    def on(self, dev):
        key = str(dev)
        if key not in self._dev:
            i32 = lambda v, shape=None: torch.tensor(v, dtype=torch.int32).reshape(shape or (len(v),)).to(dev)  # noqa: E731
            self._dev[key] = (i32(self.edges, (self.E, 2)), None if self.edge_w is None else torch.tensor(self.edge_w, dtype=torch.float64).to(dev),
                              i32(self.root), i32(self.inc_ptr), i32(self.inc_edge), i32(self.child_ptr), i32(self.child_idx))
        return self._dev[key]


class BoneLossFn(torch.autograd.Function):
    """Relative limb-length error and 1 - cos of the limb direction between prediction and ground truth, on the de-normalised global
    keypoints (csrc/bone_loss.hip): (bone, bone_dir) =
    (lam_len * sum(m w |lp - lg| / max(lg, min_len)) / max(sum m, 1), lam_dir * sum(md w (1 - vp.vg / (lp lg))) / max(sum md, 1)) over the
    edges of ``table`` (a BoneTable) in every frame of pred, gt (B, T, 2, K) fp32; mean, std: float64 (B, 2 K); score: (B, T, 2, K) or None.
    Two launches forward, one backward; the divisors stay on the device."""

    @staticmethod
    def forward(ctx, pred, gt, mean, std, score, table, lam_len, lam_dir, min_conf, min_len):
        _req_cuda(pred, gt, mean, std)
        K, E = table.K, table.E
        assert pred.dim() == 4 and pred.shape[2:] == (2, K) and pred.shape == gt.shape and pred.dtype == gt.dtype == torch.float32
        pred, gt = pred.contiguous(), gt.contiguous()
        B, T = pred.shape[0], pred.shape[1]
        assert mean.shape == std.shape == (B, 2 * K) and mean.dtype == std.dtype == torch.float64
        mean, std = mean.contiguous(), std.contiguous()
        if score is not None:
            _req_cuda(score)
            assert score.shape == pred.shape and score.dtype == torch.float32 and min_conf is not None
            score = score.contiguous()
        dev = pred.device
        tabs = table.on(dev)
        psum = torch.empty(2 * B * T, device=dev, dtype=torch.float64)
        pcnt = torch.empty(2 * B * T, device=dev, dtype=torch.int64)
        losses = torch.empty(2, device=dev, dtype=torch.float32)
        denom = torch.empty(2, device=dev, dtype=torch.float64)
        ctx.args = (B, T, K, E, float(lam_len), float(lam_dir), 0.0 if score is None else float(min_conf), float(min_len))
        edges, edge_w, root = tabs[:3]
        check(_lib.load().sdt_bone_loss_fwd_f32(_p(pred), _p(gt), _p(score), _p(mean), _p(std), _p(edges), _p(edge_w), _p(root), *ctx.args,
                                                _p(psum), _p(pcnt), _p(losses), _p(denom), _stream()))
        ctx.save_for_backward(pred, gt, mean, std, score, denom)
        ctx.tabs = tabs
        ctx.set_materialize_grads(False)  # backward takes None for a loss that nothing consumed
        bone, bone_dir = losses.unbind(0)
        return bone, bone_dir

    @staticmethod
    def backward(ctx, g_len, g_dir):
        pred, gt, mean, std, score, denom = ctx.saved_tensors
        if g_len is None and g_dir is None:
            return (None,) * 10
        dp = torch.empty_like(pred)
        g_len = None if g_len is None else g_len.contiguous()
        g_dir = None if g_dir is None else g_dir.contiguous()
        check(_lib.load().sdt_bone_loss_bwd_f32(_p(pred), _p(gt), _p(score), _p(mean), _p(std), *(_p(t) for t in ctx.tabs), _p(g_len),
                                                _p(g_dir), _p(denom), *ctx.args, _p(dp), _stream()))
        return (dp,) + (None,) * 9


class MseConstFn(torch.autograd.Function):
    """lambda * mean((scores - target)^2): the LSGAN generator / discriminator terms (voice2pose.py:171-189)."""

    @staticmethod
    def forward(ctx, scores, target, lam):
        _req_cuda(scores)
        scores = scores.contiguous()
        loss = torch.empty((), device=scores.device, dtype=torch.float32)
        check(_lib.load().sdt_mse_const_fwd_f32(_p(scores), scores.numel(), float(target), float(lam), _p(loss), _stream()))
        ctx.save_for_backward(scores)
        ctx.target, ctx.lam = float(target), float(lam)
        return loss

    @staticmethod
    def backward(ctx, gout):
        (scores,) = ctx.saved_tensors
        ds = torch.empty_like(scores)
        gout = gout.contiguous()
        check(_lib.load().sdt_mse_const_bwd_f32(_p(scores), _p(gout), scores.numel(), ctx.target, ctx.lam, _p(ds), _stream()))
        return ds, None, None


class CodeGatherKLFn(torch.autograd.Function):
    """code = table[idx] and the batch-KL regulariser on it (voice2pose.py:94,147-157) in one launch.
    Returns (code, kl, valid); kl == 0 and valid == 0 when any batch variance is exactly zero (the
    reference skips the term on the host, voice2pose.py:154 -- here the predicate stays on the device).
    The gradient of both outputs is scatter-ACCUMULATED into the dense ``table.grad``."""

    @staticmethod
    def forward(ctx, table, idx, lam, allow_single=False):
        _req_cuda(table, idx)
        B, D = idx.shape[0], table.shape[1]
        table = table.contiguous()
        idx = idx.contiguous()
        if B > 1:
            code = torch.empty((B, D), device=table.device, dtype=torch.float32)
            loss = torch.empty((), device=table.device, dtype=torch.float32)
            valid = torch.empty((), device=table.device, dtype=torch.int32)
            check(_lib.load().sdt_code_kl_fwd_f32(_p(table), _p(idx), table.shape[0], B, D, lam, _p(code), _p(loss), _p(valid),
                                                  _stream()))
        elif allow_single and not table.requires_grad:
            # validation / test with a last batch of one clip: torch.var of a single sample is nan, nan != 0, and the
            # reference adds that nan KL term to the batch's losses (voice2pose.py:152-157) -- mirrored, no crash mid-run
            code = table[idx].clone()
            loss = torch.full((), float('nan'), device=table.device, dtype=torch.float32)
            valid = torch.ones((), device=table.device, dtype=torch.int32)
        else:  # training batches come from a drop_last loader (trainer.py:75-77): B == 1 there is a configuration error
            raise RuntimeError("clip-code KL needs a batch of at least 2 clips")
        ctx.save_for_backward(code, valid, idx, table)
        ctx.lam = lam
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)  # backward takes None for an unused output's gradient
        return code, loss, valid

    @staticmethod
    def backward(ctx, gcode, gloss, _gvalid):
        code, valid, idx, table = ctx.saved_tensors
        if not table.requires_grad:
            return None, None, None, None
        lib = _lib.load()
        B, D = code.shape
        N = table.shape[0]
        gt = grad_buffer(table)
        st = _stream()
        if gcode is not None:
            gcode = gcode.contiguous()
            check(lib.sdt_rows_scatter_add_f32(_p(gcode), _p(idx), _p(gt), N, B, D, st))
        if gloss is not None:
            gloss = gloss.contiguous()
            check(lib.sdt_code_kl_bwd_f32(_p(code), _p(valid), _p(gloss), _p(idx), N, B, D, ctx.lam, _p(gt), st))
        return None, None, None, None


class TimeDiffFn(torch.autograd.Function):
    """x[:,1:]-x[:,:-1] on (B,T,C) (voice2pose.py:187-188)."""

    @staticmethod
    def forward(ctx, x):
        _req_cuda(x)
        x = x.contiguous()
        B, T, C = x.shape
        y = torch.empty((B, T - 1, C), device=x.device, dtype=torch.float32)
        check(_lib.load().sdt_time_diff_fwd_f32(_p(x), _p(y), B, T, C, _stream()))
        ctx.dims = (B, T, C)
        return y

    @staticmethod
    def backward(ctx, g):
        B, T, C = ctx.dims
        g = g.contiguous()
        dx = torch.empty((B, T, C), device=g.device, dtype=torch.float32)
        check(_lib.load().sdt_time_diff_bwd_f32(_p(g), _p(dx), B, T, C, _stream()))
        return dx


# --------------------------------------------------------------------------------------------
# no-grad ops
# --------------------------------------------------------------------------------------------
def clip_poses_prepare(raw_store, idx, mean, std, num_frames, hierarchical):
    """Device-side GestureDataset.__getitem__ + collate for a batch of stored clips (gesture_dataset.py:85-119):
    raw_store (N,Tstore,3,137) fp32, idx (B,) int64, mean/std (242,) fp32 -> poses, score (B,num_frames,2,121)."""
    _req_cuda(raw_store, idx, mean, std)
    assert raw_store.dim() == 4 and raw_store.shape[2:] == (3, 137) and raw_store.is_contiguous() and raw_store.dtype == torch.float32
    assert idx.dtype == torch.int64 and mean.numel() == 242 and std.numel() == 242
    N, Tstore = raw_store.shape[:2]
    B = idx.numel()
    poses = torch.empty((B, num_frames, 2, 121), device=raw_store.device, dtype=torch.float32)
    score = torch.empty_like(poses)
    idx, mean, std = idx.contiguous(), mean.contiguous(), std.contiguous()  # named: a temporary's block is free (and reusable) once _p() returns
    check(_lib.load().sdt_clip_poses_prepare_f32(_p(raw_store), _p(idx), _p(mean), _p(std),
                                                 _p(poses), _p(score), N, Tstore, B, num_frames, int(bool(hierarchical)), _stream()))
    return poses, score


def rows_gather(src, idx):
    """dst[b] = src[idx[b]] for a (N, n_cols) fp32 store (the batch's audio rows)."""
    _req_cuda(src, idx)
    assert src.dim() == 2 and src.is_contiguous() and src.dtype == torch.float32 and idx.dtype == torch.int64
    dst = torch.empty((idx.numel(), src.shape[1]), device=src.device, dtype=torch.float32)
    idx = idx.contiguous()
    check(_lib.load().sdt_rows_gather_f32(_p(src), _p(idx), _p(dst), src.shape[0], idx.numel(), src.shape[1], _stream()))
    return dst


def final_metrics(pred, gt, mean, std, scale, hierarchical, want_final=True):
    """get_final_results x2 + evaluate_step in float64 (gesture_dataset.py:193-220, voice2pose.py:412-430).
    pred/gt (B,T,2,K) fp32; mean/std (B,2K) f64; scale (B,) f64 -> (final_pred, final_gt, metrics[2])."""
    _req_cuda(pred, gt, mean, std, scale)
    B, T, _, K = pred.shape
    pred, gt = pred.contiguous(), gt.contiguous()
    dev = pred.device
    fp = torch.empty((B, T, 2, K), device=dev, dtype=torch.float64) if want_final else None
    fg = torch.empty((B, T, 2, K), device=dev, dtype=torch.float64) if want_final else None
    work = _ARENA.take(3 * B * T + 4, dev)
    metrics = torch.empty(2, device=dev, dtype=torch.float64)
    # the contiguous copies of broadcast statistics (DeviceClipStore hands out expand()ed views) must outlive the launch call: as unnamed
    # temporaries the three copies were freed one by one and re-used each other's block -- the kernel then read `std` through `mean`'s pointer
    mean, std, scale = mean.contiguous(), std.contiguous(), scale.contiguous()
    check(_lib.load().sdt_final_metrics_f64(_p(pred), _p(gt), _p(mean), _p(std), _p(scale),
                                            1 if hierarchical else 0, B, T, K, _p(fp), _p(fg), _p(work), _p(metrics), _stream()))
    return fp, fg, metrics


N_FFT, WIN, HOP, N_FREQ = 512, 400, 160, 257


def dft_basis(window):
    """(514, 3, 160) fp32 windowed real-DFT basis: row 2f = w*cos, row 2f+1 = -w*sin (bin f) over the 400
    window samples that sit at offset 56 in the 512-sample frame; zero beyond sample 400."""
    w = window.detach().double().cpu()
    k = torch.arange(WIN, dtype=torch.float64)
    f = torch.arange(N_FREQ, dtype=torch.float64)
    ang = 2.0 * math.pi * torch.outer(f, k + (N_FFT - WIN) // 2) / N_FFT
    basis = torch.zeros(2 * N_FREQ, 3 * HOP, dtype=torch.float64)
    basis[0::2, :WIN] = torch.cos(ang) * w
    basis[1::2, :WIN] = -torch.sin(ang) * w
    return basis.float().reshape(2 * N_FREQ, 3, HOP).contiguous()


def fb_bin_ranges(fb):
    """[lo,hi) of the non-zero rows of every filterbank column (int32 tensors on fb's device)."""
    nz = (fb.detach().cpu() != 0)
    n_freq = nz.shape[0]
    idx = torch.arange(n_freq).unsqueeze(1)
    lo = torch.where(nz, idx, torch.full_like(idx, n_freq)).min(0).values
    hi = torch.where(nz, idx + 1, torch.zeros_like(idx)).max(0).values
    lo = torch.minimum(lo, hi)
    return lo.to(torch.int32).to(fb.device), hi.to(torch.int32).to(fb.device)


def mel_spectrogram(audio, basis, fb, bins=None):
    """audio (B,L) -> power mel (B, n_mels, 1+L//160)  (torchaudio 0.7 MelSpectrogram as set up at voice2pose.py:27-30)."""
    _req_cuda(audio, basis, fb)
    lo, hi = bins if bins is not None else fb_bin_ranges(fb)
    lib = _lib.load()
    audio = audio.contiguous()
    B, L = audio.shape
    F = 1 + L // HOP
    nh = F + 2
    st = _stream()
    hops = torch.empty((B, nh, HOP), device=audio.device, dtype=torch.float32)
    check(lib.sdt_stft_frames_f32(_p(audio), _p(hops), B, L, nh, st))
    g = _geom(B=B, Hi=1, Wi=nh, Cin=HOP, Ho=1, Wo=F, Hy=1, Wy=F, Cout=2 * N_FREQ, sy=1, sx=1, osy=1, osx=1, ooy=0, oox=0,
              Tw=3, taps=[(0, 0, 0), (0, 1, 1), (0, 2, 2)])
    spec = torch.empty((B, F, 2 * N_FREQ), device=audio.device, dtype=torch.float32)
    math = _CONV_MATH_NOW[0]
    if math != 0:  # the STFT keeps exact fp32 products whatever arithmetic the convolutions run in: the power mel spans 5 decades
        check(lib.sdt_set_conv_math(0))
    try:
        check(lib.sdt_conv_taps_f32(_p(hops), _p(basis), None, _p(spec), g, st))
    finally:
        if math != 0:
            check(lib.sdt_set_conv_math(math))
    nmel = fb.shape[1]
    mel = torch.empty((B, nmel, F), device=audio.device, dtype=torch.float32)
    fb = fb.contiguous()
    check(lib.sdt_mel_fb_f32(_p(spec), _p(fb), _p(lo), _p(hi), _p(mel), B, F, N_FREQ, nmel, st))
    return mel


def adam_step(p, g, m, v, lr_dev, state_dev, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0):
    """One torch.optim.Adam step over flat fp32 buffers (voice2pose.py:249-279,302-304)."""
    _req_cuda(p, g, m, v, lr_dev, state_dev)
    check(_lib.load().sdt_adam_step_f32(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(lr_dev), beta1, beta2, eps, weight_decay,
                                        grad_scale, _p(state_dev), _stream()))


# --------------------------------------------------------------------------------------------
# Optimiser-side safeguards (csrc/optim_guard.hip)
GUARD_WORDS = 4  # the guard record as int64 words: {f64 norm | f32 scale, i32 skip | i64 skipped | reserved}


def grad_sumsq_partials():
    """float64 elements the ``partial`` buffer of ``grad_sumsq`` needs"""
    return int(_lib.load().sdt_grad_sumsq_partials())


def optim_guard_pass_elems(which):
    """elements ONE grid pass of the launch as built covers: 'sumsq' or 'adam' (the guarded step)"""
    return int(_lib.load().sdt_optim_guard_pass_elems({'sumsq': 0, 'adam': 1}[which]))


def grad_sumsq(g, partial):
    """partial[0] = ordered float64 sum of squares of the fp32 buffer ``g`` (bit-identical to optim.sumsq_model)"""
    _req_cuda(g, partial)
    if g.dtype != torch.float32 or partial.dtype != torch.float64 or partial.numel() < grad_sumsq_partials():
        raise ValueError('grad_sumsq: g must be fp32 and partial %d float64 elements' % grad_sumsq_partials())
    check(_lib.load().sdt_grad_sumsq_f64(_p(g), g.numel(), _p(partial), _stream()))
    return partial


def optim_guard_prep(partials, guard, grad_scale=1.0, max_norm=0.0, skip_nonfinite=False):
    """Combine up to four buffers' sums of squares (argument order) into the device guard record: pre-clip norm, effective gradient
    scale, skip flag, skip counter.  ``max_norm`` <= 0: no clipping."""
    _req_cuda(guard, *partials)
    if not 1 <= len(partials) <= 4:
        raise ValueError('a step group has 1 to 4 buffers, got %d' % len(partials))
    if guard.dtype != torch.int64 or guard.numel() < GUARD_WORDS:
        raise ValueError('the guard record is %d int64 words' % GUARD_WORDS)
    import ctypes as C
    arr = (C.c_void_p * len(partials))(*[_p(t) for t in partials])
    check(_lib.load().sdt_optim_guard_prep(arr, len(partials), grad_scale, float(max_norm), int(bool(skip_nonfinite)), _p(guard), _stream()))


def adam_step_guarded(p, g, m, v, lr_dev, state_dev, guard, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, ema=None, ema_decay=0.0):
    """``adam_step`` with the gradient scale and the skip decision read from the guard record; ``ema``: the EMA of the new parameters in
    the same pass."""
    _req_cuda(p, g, m, v, lr_dev, state_dev, guard)
    if ema is not None:
        _req_cuda(ema)
        if ema.numel() != p.numel() or ema.dtype != torch.float32:
            raise ValueError('the EMA buffer must match the parameter buffer')
    check(_lib.load().sdt_adam_step_guarded_f32(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(lr_dev), beta1, beta2, eps, weight_decay,
                                                _p(guard), _p(ema), ema_decay, _p(state_dev), _stream()))


# --------------------------------------------------------------------------------------------
# Per-tensor histograms and moments of a flat buffer (csrc/tensor_hist.hip; tensor_hist.py is the interface)
def _check_sizes(status):
    """as ``check``; the library's "unsupported size" status becomes a ValueError"""
    if status == -3:  # SDT_ERR_UNSUPPORTED
        raise ValueError('libsdt_hip: %s' % _lib.load().sdt_last_error().decode())
    check(status)


def tensor_hist_constants():
    """launch constants of the library as built: {'threads', 'chunk', 'buckets', 'max_segments'}"""
    lib = _lib.load()
    return {k: int(getattr(lib, 'sdt_tensor_hist_' + k)()) for k in ('threads', 'chunk', 'buckets', 'max_segments')}


def tensor_hist_plan(offsets, sizes, n):
    """Host side (no GPU): the segment table (S, 3) {offset, numel, first chunk} and the chunk table (C, 2) {segment, chunk number} of a
    flat buffer of ``n`` elements, int64 CPU tensors.  ValueError for sizes the kernel does not take."""
    import ctypes as C
    lib = _lib.load()
    S = len(offsets)
    if len(sizes) != S:
        raise ValueError('tensor_hist_plan: %d offsets but %d sizes' % (S, len(sizes)))
    segs = torch.tensor([[int(o), int(s)] for o, s in zip(offsets, sizes)], dtype=torch.int64).reshape(S, 2)
    n_chunks = C.c_int64(0)
    _check_sizes(lib.sdt_tensor_hist_plan(_p(segs) if S else None, S, int(n), None, None, 0, C.addressof(n_chunks)))
    seg_plan = torch.zeros((S, 3), dtype=torch.int64)
    chunk_plan = torch.zeros((max(1, n_chunks.value), 2), dtype=torch.int64)
    _check_sizes(lib.sdt_tensor_hist_plan(_p(segs), S, int(n), _p(seg_plan), _p(chunk_plan), n_chunks.value, C.addressof(n_chunks)))
    return seg_plan, chunk_plan[:n_chunks.value]


def tensor_hist(flat, seg_plan, chunk_plan, edges, scale, counts, tallies, stats, partials):
    """one segmented pass over the fp32 buffer ``flat`` on the current stream (tables, edges and outputs are device tensors)"""
    _req_cuda(flat, seg_plan, chunk_plan, edges, counts, tallies, stats, partials)
    S, nc = seg_plan.shape[0], chunk_plan.shape[0]
    if flat.dtype != torch.float32 or not flat.is_contiguous():
        raise ValueError('tensor_hist: flat must be a contiguous fp32 buffer')
    if counts.dtype != torch.int64 or tallies.dtype != torch.int64 or stats.dtype != torch.float64 or edges.dtype != torch.float64 \
            or counts.numel() < S * (edges.numel() - 1) or tallies.numel() < 3 * S or stats.numel() < 4 * S or partials.numel() < 4 * nc \
            or partials.dtype != torch.float64:
        raise ValueError('tensor_hist: output buffers of the wrong type or size')
    _check_sizes(_lib.load().sdt_tensor_hist_f32(_p(flat), flat.numel(), _p(seg_plan), S, _p(chunk_plan), nc, _p(edges), edges.numel(),
                                                 float(scale), _p(counts), _p(tallies), _p(stats), _p(partials), _stream()))
