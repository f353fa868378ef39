"""Functional NFP: `nfp(x, cfg)` — the autograd op behind NFPPooling.forward.

CUDA tensors go through libnfp_hip.so (include/nfp.h) — one fused forward kernel,
one fused backward kernel, saved state = the output map plus one float per input
pixel.  Nothing else can serve a CUDA tensor: if the library is missing or refuses
the configuration the call raises.  CPU tensors use `_host.nfp_host` (see there).
"""
import ctypes
import dataclasses
import os
from collections import OrderedDict
from dataclasses import dataclass

import torch

from . import _abi
from ._host import attention_pool_host, compress_conv, compress_finish, compress_map_host, compress_pool_host, nfp_host


@dataclass(frozen=True)
class NfpConfig:
    """Constructor arguments of NFPPooling that define the op (nfp.py:16-39)."""
    R: int = 1
    measure: str = "norm"          # lower-cased name (nfp.py:21)
    p: float = 1
    stride: int = 1
    padding: int = 0
    dilation: int = 1
    padding_mode: str = "reflect"
    similarity: bool = True
    eps: float = 1e-6
    q_scs: float = 1e-6
    diff_weights: bool = True      # raw measure string in ['norm','rmse','mahalanobis'] (nfp.py:74)
    inner_R: int = 0               # 1 with R = 2: also the maps of radius 1 (padding 1), first in the channel axis —
                                   # the concatenation models/nfp_heads.py:80-118 builds from two layers
    map_f32: int = 0               # 1 with a bf16 x: float32 maps, a bf16 gradient (nfp_desc.map_f32) — set by `nfp` itself
                                   # for a bf16 map under torch.autocast, never by a module's constructor

    @property
    def kernel_size(self):
        return 2 * self.R + 1

    @property
    def out_channels(self):
        return self.kernel_size ** 2 - 1 + ((2 * self.inner_R + 1) ** 2 - 1 if self.inner_R else 0)


_DTYPES = {torch.float32: _abi.F32, torch.bfloat16: _abi.BF16}

_CPP = None     # the C++ autograd nodes (csrc/nfp_torch.cpp), None until looked for, False when absent


def _cpp_nodes():
    """neighbour_feature_pooling_amd/_nfp_torch.so — the same autograd nodes as the Python classes below, in C++
    (no interpreter on the launch path).  Optional: NFP_PY_NODES=1 or a missing module selects the Python nodes."""
    global _CPP
    if _CPP is None:
        import importlib.util
        import os
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_nfp_torch.so")
        _CPP = False
        if os.environ.get("NFP_PY_NODES") != "1" and os.path.exists(path):
            _abi.load()     # libnfp_hip.so first: the module links against it
            spec = importlib.util.spec_from_file_location(__package__ + "._nfp_torch", path)
            mod = importlib.util.module_from_spec(spec)
            try:
                spec.loader.exec_module(mod)
                if mod.desc_bytes == ctypes.sizeof(_abi.NfpDesc):
                    _CPP = mod
            except (ImportError, OSError):   # built against another torch: the Python nodes serve
                _CPP = False
    return _CPP


def _cpp_call(fn, *args):
    """Run a C++ node; its TORCH_CHECK messages carry the library's error class as a prefix."""
    try:
        return fn(*args)
    except RuntimeError as e:
        msg = str(e).split("\n")[0]
        if "libnfp_hip unsupported: " in msg:
            raise _abi.NfpUnsupported("libnfp_hip: " + msg.split("libnfp_hip unsupported: ", 1)[1]) from None
        if "libnfp_hip error: " in msg:
            raise _abi.NfpError("libnfp_hip: " + msg.split("libnfp_hip error: ", 1)[1]) from None
        raise


def _layout_of(shape, strides):
    """'nchw' / 'nhwc' when every image of a [B,C,H,W] tensor with these element strides is dense in that order —
    whatever the batch stride — else None.  (Size-1 dimensions carry arbitrary strides in torch: they match anything.)"""
    _, C, H, W = shape

    def matches(canon):
        return all(n == 1 or s == c for n, s, c in zip((C, H, W), strides[1:], canon))

    if matches((H * W, W, 1)):
        return "nchw"
    if matches((1, W * C, C)):
        return "nhwc"
    return None


def _inner_layout(x):
    """`_layout_of` a tensor: the kernels take the batch stride from the descriptor, so e.g. ViT patch tokens behind a
    class token (a [B,1+HW,C] buffer viewed as [B,C,H,W], texture_pooling.py:181-188) are read in place."""
    return _layout_of(x.shape, x.stride())


def _in_place_layout(shape, strides, itemsize=0, ptr=0):
    """The layout in which the kernels read such a tensor where it lies — images dense in NCHW or channels-last order that
    do not overlap (batch stride >= C*H*W) — else None.  With `itemsize` (and the data pointer) also what the fused
    channels-last kernels ask: they load 16 bytes per lane, so images start on 16-byte boundaries."""
    layout = _layout_of(shape, strides)
    if layout is None or (shape[0] > 1 and strides[0] < shape[1] * shape[2] * shape[3]):
        return None
    if layout == "nhwc" and (ptr % 16 or (strides[0] * itemsize) % 16):
        return None
    return layout


def _canon(shape, layout, sB=None):
    """Element strides handed to the library for a dense-image layout (batch stride sB; None or B = 1: dense)."""
    B, C, H, W = shape
    if sB is None or B == 1:
        sB = C * H * W
    return (sB, H * W, W, 1) if layout == "nchw" else (sB, 1, W * C, C)


def _canonical_strides(x, layout):
    """`_canon` of a tensor (size-1 dimensions carry arbitrary strides in torch)."""
    return _canon(x.shape, layout, x.stride(0))


def _dense(x):
    """(x, layout): x itself when its images are dense NCHW or channels-last (read in place by strides), otherwise an
    NCHW copy."""
    layout = _in_place_layout(x.shape, x.stride())
    return (x, layout) if layout is not None else (x.contiguous(), "nchw")


def build_desc(shape, strides, dtype, cfg):
    """The NfpDesc of a call from plain values — the one place a descriptor is filled; `ws` is left unset."""
    if dtype not in _DTYPES:
        raise _abi.NfpUnsupported(f"NFP HIP kernels take float32 or bfloat16 feature maps, got {dtype}")
    d = _abi.NfpDesc()
    d.B, d.C, d.H, d.W = shape
    d.R, d.pad, d.stride, d.dilation = cfg.R, cfg.padding, cfg.stride, cfg.dilation
    d.pad_mode = _abi.PAD_MODES.index(cfg.padding_mode)
    d.measure = _abi.measure_id(cfg.measure)
    d.similarity = int(bool(cfg.similarity))
    d.diff_weights = int(bool(cfg.diff_weights))
    d.dtype = _DTYPES[dtype]
    d.p, d.eps, d.q_scs = float(cfg.p), float(cfg.eps), float(cfg.q_scs)
    d.sxB, d.sxC, d.sxH, d.sxW = strides
    d.sgB = d.C * d.H * d.W          # grad_x is always allocated dense, in x's inner layout
    d.inner_R = int(cfg.inner_R)
    d.map_f32 = int(cfg.map_f32)
    return d


def make_desc(x, cfg, layout=None):
    """`build_desc` of a tensor (one that is not dense inside its images: of its NCHW copy)."""
    if layout is None:
        x, layout = _dense(x)
    return build_desc(x.shape, _canonical_strides(x, layout), x.dtype, cfg)


def output_shape(d):
    L = _abi.load()
    n, ho, wo = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _abi.check(L.nfp_output_shape(ctypes.byref(d), ctypes.byref(n), ctypes.byref(ho), ctypes.byref(wo)))
    return d.B, n.value, ho.value, wo.value


_WORKSPACES = {}            # (device, geometry) -> [uint8 tensor, fill event or None, fill stream, device index] or False
_PENDING_FILLS = []         # the records of _WORKSPACES whose fill event has not been seen complete yet


def _order_after_fills(device):
    """Every launch path calls this while a table fill may still be running (the ordering used to live in
    _workspace(), which a plan-cache hit never reaches — a same-shape call on ANOTHER stream right after the first one
    launched on tables that were not written yet).  A fill is ordered before later work of its own stream; any other
    stream waits for its event on the device (no host synchronisation); a completed event is dropped, so in steady state
    this is one truthiness test of an empty list.  Under a graph capture neither an event query nor a wait on an event
    recorded outside the capture is legal: nothing is done — a capture is preceded by a device synchronisation
    (torch.cuda.graph does one itself), which also completes every fill enqueued before it."""
    if torch.cuda.is_current_stream_capturing():
        return
    cur = None
    for rec in list(_PENDING_FILLS):
        if rec[1] is None or rec[1].query():
            rec[1] = None
            _PENDING_FILLS.remove(rec)
        elif rec[3] == device.index:
            if cur is None:
                cur = _raw_stream(device)
            if cur != rec[2]:
                torch.cuda.current_stream(device).wait_event(rec[1])


def _workspace(d, device):
    """Device pointer of the workspace of `d` (include/nfp.h: nfp_workspace_bytes / nfp_workspace_init: the pooled
    kernels' arrival counters and the geometry's constant tables), or None.  It depends on the geometry only, so every call
    with the same map size and kernel on the same stream shares one buffer.  The fill kernel is enqueued once, on the stream that first needs the tables, followed by an event
    (_order_after_fills).  Under a graph capture no table is built (the fill would only be recorded, not run, and a
    later eager call would read an unfilled buffer): that one call is planned without tables and nothing is cached —
    warm a geometry up before capturing it, as every graph user does anyway."""
    # (one workspace per STREAM: besides the constant tables it holds the arrival counters of the pooled kernels' row bands
    # — include/nfp.h: one pooled launch at a time per workspace; launches on one stream are ordered)
    key = (device.index, d.H, d.W, d.R, d.pad, d.stride, d.dilation, d.pad_mode, d.inner_R, _raw_stream(device))
    rec = _WORKSPACES.get(key)
    if rec is None:
        L = _abi.load()
        nbytes = int(L.nfp_workspace_bytes(ctypes.byref(d)))
        if nbytes < 0:
            return None     # the descriptor itself is refused (bad p / eps ...): say nothing about the GEOMETRY
        if nbytes == 0:
            _WORKSPACES[key] = rec = False
        else:
            if torch.cuda.is_current_stream_capturing():
                import warnings
                warnings.warn("NFP: a geometry first seen inside a graph capture runs without its workspace tables "
                              "(general kernels); call the op once before capturing", RuntimeWarning, stacklevel=4)
                return None
            with _on_device(device):
                ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
                _abi.check(L.nfp_workspace_init(ctypes.byref(d), ws.data_ptr(), _raw_stream(device)))
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(device))
            _WORKSPACES[key] = rec = [ws, ev, _raw_stream(device), device.index]
            _PENDING_FILLS.append(rec)
    if rec is False:
        return None
    return rec[0].data_ptr()


_PLANS = OrderedDict()      # plan key -> _Plan, least recently used first
_PLANS_MAX = 256


def _plans_get(key):
    plan = _PLANS.get(key)
    if plan is not None:
        _PLANS.move_to_end(key)
    return plan


def _plans_put(key, plan):
    _PLANS[key] = plan
    if len(_PLANS) > _PLANS_MAX:
        _PLANS.popitem(last=False)


class _Plan:
    """What the host side of a call needs, asked of the library once per input signature: the descriptor, a uint8 tensor
    over the descriptor's own bytes (what the C++ nodes take and save for their backward: the tensor keeps the descriptor
    alive, in the cache or not), the output shape, the floats of saved state and `no_bwd` — None when nfp_backward serves
    the descriptor too, else the library's message: forward and backward envelopes differ for a few large maps, and a call
    that will need a gradient must fail in forward(), not inside loss.backward(); `no_fwd` likewise for nfp_forward (asked
    of map_f32 plans alone: the native autocast call needs both directions).  `cacheable` is False for the table-less
    plan of a geometry first seen under a graph capture: it says nothing about later calls.  Whatever else the library
    says about the descriptor (`ask`) is kept here too, so that nothing about a plan outlives it."""
    __slots__ = ("desc", "desc_tensor", "nhwc", "oshape", "saved_floats", "no_bwd", "no_fwd", "cacheable", "_asked")

    def __init__(self, desc, layout, cacheable=True):
        self.desc = desc
        self.desc_tensor = torch.frombuffer(desc, dtype=torch.uint8)
        self.nhwc = layout == "nhwc"
        self.oshape = output_shape(desc)
        self.saved_floats = 0
        self.no_bwd = None
        self.no_fwd = None
        self.cacheable = cacheable
        self._asked = {}

    def ask(self, fn):
        """int(<fn>(descriptor)) of the library's descriptor-only queries (nfp_pool_saved_floats, nfp_gap_saved_floats,
        nfp_pool_supported, nfp_gap_supported, nfp_bias_saved_floats, nfp_bias_scratch_floats), each asked once."""
        v = self._asked.get(fn)
        if v is None:
            v = self._asked[fn] = int(getattr(_abi.load(), fn)(ctypes.byref(self.desc)))
        return v


def _plan(x, layout, cfg):
    """The _Plan of this input signature — cached (LRU): in eager mode the host side of a call (a few ctypes round trips)
    otherwise costs more than the two kernels."""
    key = (tuple(x.shape), x.stride(0), layout, x.dtype, cfg, x.device.index)
    plan = _plans_get(key)
    if _PENDING_FILLS:
        _order_after_fills(x.device)
    if plan is None:
        L = _abi.load()
        d = make_desc(x, cfg, layout)
        d.ws = _workspace(d, x.device)
        plan = _Plan(d, layout, cacheable=d.ws is not None or not torch.cuda.is_current_stream_capturing())
        buf = ctypes.create_string_buffer(1024)
        if L.nfp_plan(ctypes.byref(d), 1, buf, len(buf)) != 0:
            plan.no_bwd = L.nfp_last_error().decode()
        if d.map_f32 and L.nfp_plan(ctypes.byref(d), 0, buf, len(buf)) != 0:
            plan.no_fwd = L.nfp_last_error().decode()
        plan.saved_floats = int(L.nfp_saved_floats(ctypes.byref(d)))
        if plan.cacheable:
            _plans_put(key, plan)
    return plan


def _planned(x, cfg):
    """(x as the kernels read it, its plan)."""
    x, layout = _dense(x)
    return x, _plan(x, layout, cfg)


def _raw_stream(dev):
    """hipStream_t of torch's current stream on `dev` as an int.  torch.cuda.current_stream() builds a Stream
    object through several Python layers (~20 us, more than both kernels' launch cost); the raw accessor that
    Inductor-generated code uses is a single C call."""
    try:
        return torch._C._cuda_getCurrentRawStream(dev.index)
    except AttributeError:  # pragma: no cover - older / newer torch without the private accessor
        return torch.cuda.current_stream(dev).cuda_stream


class _on_device:
    """`with torch.cuda.device(dev)` only when dev is not already current (the common case costs nothing)."""

    def __init__(self, dev):
        self.ctx = None if dev.index == torch.cuda.current_device() else torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def _keeps_state(cfg, dtype, need_grad):
    """No saved state without a gradient to follow — except bf16 Attention, which keeps its raw dots there regardless."""
    return need_grad or (cfg.measure == "attention" and dtype != torch.float32)


def _saved_len(plan, cfg, dtype, need_grad):
    """Floats of saved state nfp_forward gets for this call; refuses a call whose gradient could not be served."""
    if need_grad and plan.no_bwd is not None:
        raise _abi.NfpUnsupported(f"libnfp_hip: the forward of this call is served but its backward is not "
                                  f"({plan.no_bwd}); run it under torch.no_grad() or on a detached input")
    return max(plan.saved_floats, 0) if _keeps_state(cfg, dtype, need_grad) else 0


def _scratch_len(need, ns):
    """The scratch length of a launch: what the library asks for, or the caller's (the compiled graph's shape-only bound)."""
    if ns is None:
        return need
    assert need <= ns, f"the library needs {need} floats of saved state, the caller allots {ns}"
    return ns


def _empty_grad_x(x, nhwc):
    """grad_x: dense, in x's inner layout (desc.sgB) — a batch-strided view of x does not get a gradient with gaps."""
    return torch.empty(x.shape, dtype=x.dtype, device=x.device,
                       memory_format=torch.channels_last if nhwc else torch.contiguous_format)


def _grad_out_as(grad_out, dtype):
    go = grad_out.contiguous()
    return go if go.dtype == dtype else go.to(dtype)


def nfp_forward_call(x, cfg, need_grad, ns=None):
    """(out, saved, x as launched, plan) from nfp_forward.  need_grad: x.requires_grad and grad mode on, sampled by the
    caller (grad mode is always off inside an autograd.Function, and ctx.needs_input_grad ignores torch.no_grad())."""
    L = _abi.load()
    x, plan = _planned(x, cfg)
    ns = _scratch_len(_saved_len(plan, cfg, x.dtype, need_grad), ns)
    with _on_device(x.device):
        out = torch.empty(plan.oshape, dtype=torch.float32 if plan.desc.map_f32 else x.dtype, device=x.device)
        saved = torch.empty(ns, dtype=torch.float32, device=x.device)
        _abi.check(L.nfp_forward(ctypes.byref(plan.desc), x.data_ptr(), out.data_ptr(),
                                 saved.data_ptr() if ns > 0 else None, _raw_stream(x.device)))
    return out, saved, x, plan


def nfp_backward_call(x, plan, out, saved, grad_out):
    """grad_x from nfp_backward; (x, plan) as `_planned` or the forward call gave them."""
    L = _abi.load()
    go = _grad_out_as(grad_out, out.dtype)      # (the maps' type: x's, or float32 for a map_f32 plan)
    with _on_device(x.device):
        gx = _empty_grad_x(x, plan.nhwc)
        _abi.check(L.nfp_backward(ctypes.byref(plan.desc), x.data_ptr(), go.data_ptr(), out.data_ptr(),
                                  saved.data_ptr() if saved.numel() else None, gx.data_ptr(), _raw_stream(x.device)))
    return gx


class _NfpHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cfg, need_grad):
        out, saved, x, ctx.plan = nfp_forward_call(x, cfg, need_grad)
        ctx.save_for_backward(x, out, saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, out, saved = ctx.saved_tensors
        return nfp_backward_call(x, ctx.plan, out, saved, grad_out), None, None


def pool_forward_call(x, cfg, want_gap, need_grad, ns=None):
    """(gap [B,C], nfpm [B,N], maps, saved, x as launched, plan) from nfp_pool_forward on a call `nfp_pool_fused_ok`
    accepted.  want_gap = False: gap comes back empty and its sums are never taken; need_grad = False: the maps themselves
    are not stored either (include/nfp.h, ABI 6)."""
    L = _abi.load()
    x, plan = _planned(x, cfg)
    B, N, Ho, Wo = plan.oshape
    ns = _scratch_len(max(plan.ask("nfp_pool_saved_floats"), 0), ns)
    with _on_device(x.device):
        gap = torch.empty(B if want_gap else 0, x.shape[1], dtype=torch.float32, device=x.device)
        nfpm = torch.empty(B, N, dtype=torch.float32, device=x.device)
        out_map = torch.empty((B, N, Ho, Wo) if need_grad else (0,), dtype=x.dtype, device=x.device)
        saved = torch.empty(ns, dtype=torch.float32, device=x.device)
        _abi.check(L.nfp_pool_forward(ctypes.byref(plan.desc), x.data_ptr(), gap.data_ptr() if want_gap else None,
                                      nfpm.data_ptr(), out_map.data_ptr() if need_grad else None,
                                      saved.data_ptr() if ns > 0 else None, _raw_stream(x.device)))
    return gap, nfpm, out_map, saved, x, plan


def pool_backward_call(x, plan, out_map, saved, grad_gap, grad_nfpm):
    """grad_x from nfp_pool_backward; grad_gap None: GAP(x) took no part (ggap = NULL in the library)."""
    L = _abi.load()
    gg = grad_gap.contiguous().float() if grad_gap is not None else None
    gn = grad_nfpm.contiguous().float()
    with _on_device(x.device):
        gx = _empty_grad_x(x, plan.nhwc)
        _abi.check(L.nfp_pool_backward(ctypes.byref(plan.desc), x.data_ptr(), gg.data_ptr() if gg is not None else None,
                                       gn.data_ptr(), out_map.data_ptr(), saved.data_ptr() if saved.numel() else None,
                                       gx.data_ptr(), _raw_stream(x.device)))
    return gx


class _NfpPoolHip(torch.autograd.Function):
    """(gap [B,C], nfpm [B,N]) = fused tail of models/NFP_Pooling.py:27-31 in one pass over x.  want_gap = False: the
    pooled NFP maps alone (texture_pooling.py:251-252, 320-321)."""

    @staticmethod
    def forward(ctx, x, cfg, want_gap, need_grad):
        gap, nfpm, out_map, saved, x, ctx.plan = pool_forward_call(x, cfg, want_gap, need_grad)
        ctx.want_gap = want_gap
        ctx.save_for_backward(x, out_map, saved)
        return gap, nfpm

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_gap, g_nfpm):
        x, out_map, saved = ctx.saved_tensors
        return pool_backward_call(x, ctx.plan, out_map, saved, g_gap if ctx.want_gap else None, g_nfpm), None, None, None


def _fused_ok(x, cfg, supported):
    """True when the library's `supported` predicate (a dry run of both launchers) accepts this call as it lies in memory:
    float32 or bfloat16, readable in place, channels-last images on 16-byte boundaries."""
    if not (x.is_cuda and x.dim() == 4 and x.dtype in _DTYPES):
        return False
    layout = _in_place_layout(x.shape, x.stride(), x.element_size(), x.data_ptr())
    return layout is not None and bool(_plan(x, layout, cfg).ask(supported))


def nfp_pool_fused_ok(x, cfg):
    """True when the fused GAP + pooled-NFP kernels can serve this call: "same" maps (stride 1, pad = R; above 512 pixels:
    rows of W <= 254 / 142 pixels for k = 3 / 5, any height), cosine / dot / gfc / L2 / rmse, float32 or bfloat16, images dense in NCHW
    or channels-last order."""
    return _fused_ok(x, cfg, "nfp_pool_supported")


_WARNED_F64 = False


def _amp_input(x):
    """What the reference's op sequence does with low precision on the GPU (measured on an MI355X,
    profiles/r03_c_autocast_probe_reference_ops.jsonl; scripts/probe_autocast.py):
      * under torch.autocast("cuda", ...) F.cosine_similarity and linalg.norm are on autocast's float32 list: the maps
        come back float32 whatever the input type, gradients in the input's type;
      * a float16 tensor outside autocast runs in float16 end to end: float16 maps.
    The kernels store float32 / bfloat16 and always sum in float32, so: under autocast the input is taken as float32
    and the op runs outside autocast (float32 maps, as the reference; no bf16 rounding of the inputs in between, so
    it is the closer of the two to the float32 result); float16 is computed in float32 and the maps rounded to float16
    once.  Returns (tensor to run on, dtype to cast the result to or None)."""
    if x.is_cuda and torch.is_autocast_enabled("cuda"):
        return x.float(), None
    if x.is_cuda and x.dtype == torch.float16:
        return x.float(), torch.float16
    if x.is_cuda and x.dtype == torch.float64:
        # The reference follows the input type (nfp.py:141-159): float64 in, float64 maps.  The kernels compute in
        # float32: the maps agree with the float64 reference to float32 rounding (<= 1e-6 of the tensor's magnitude, inside
        # the 1e-5 parity bar), in the reference's type.  Said once per process, not silently.
        global _WARNED_F64
        if not _WARNED_F64:
            import warnings
            warnings.warn("NFP: float64 feature maps are computed in float32 by the HIP kernels and returned as float64",
                          RuntimeWarning, stacklevel=4)
            _WARNED_F64 = True
        return x.float(), torch.float64
    return x, None


_MIXED_CFGS = {}      # cfg -> the same with map_f32 = 1


def _autocast_native(x, cfg):
    """(x as launched, plan, the map_f32 configuration) of the native torch.autocast call — bf16 x in, float32 maps out, a bf16 grad_x back
    (nfp_desc.map_f32): no float32 copy of x, no cast of the gradient — or None where `_amp_input`'s upcast serves:
    anything but a bf16 CUDA map under autocast, torch.compile, SharpenedCosine / Attention, two radii at once, a
    descriptor the library does not plan in both directions, or NFP_AMP_UPCAST=1 (read at call time: a safety valve).
    OPT-IN: taken only with NFP_AMP_NATIVE=1 in the environment (read at call time).  The timing that was to decide, per
    shape class, whether this call replaces the upcast has not been made; until it is, the upcast stays the
    default for every class."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and torch.is_autocast_enabled("cuda")):
        return None
    if (torch.compiler.is_compiling() or cfg.measure in ("scs", "attention") or cfg.inner_R
            or os.environ.get("NFP_AMP_NATIVE") != "1" or os.environ.get("NFP_AMP_UPCAST") == "1"):
        return None
    mcfg = _MIXED_CFGS.get(cfg)
    if mcfg is None:
        mcfg = _MIXED_CFGS[cfg] = dataclasses.replace(cfg, map_f32=1)
    try:
        xd, plan = _planned(x, mcfg)
    except _abi.NfpError:
        return None
    return (xd, plan, mcfg) if plan.no_fwd is None and plan.no_bwd is None else None


def nfp_pool(x, cfg, want_gap=True):
    """(GAP(x) [B,C], GAP(NFP(x)) [B,N]) — NFP_Pooling.py:27-31.  Fused on the GPU where supported,
    otherwise the same two reductions composed from `nfp` and torch ops.  want_gap = False: (None, GAP(NFP(x))) — the
    channel sums of x are not taken (nfp_pooled)."""
    xin, cast = _amp_input(x)
    if xin is not x:
        with torch.autocast("cuda", enabled=False):
            gap, nfpm = nfp_pool(xin, cfg, want_gap)
        return (gap, nfpm) if cast is None else (None if gap is None else gap.to(cast), nfpm.to(cast))
    if x.is_cuda and torch.compiler.is_compiling() and x.dim() == 4:
        # under torch.compile: the registered custom op (one node in the compiled graph, no graph break) — _ops.py
        from . import _ops
        need_grad = x.requires_grad and torch.is_grad_enabled()
        gap, nfpm, _, _ = torch.ops.nfp_amd.nfp_pool(x, *_ops.cfg_args(cfg), bool(want_gap), bool(need_grad))
        return (gap if want_gap else None), nfpm
    if x.dim() == 4 and nfp_pool_fused_ok(x, cfg):
        need_grad = x.requires_grad and torch.is_grad_enabled()
        try:
            cpp = _cpp_nodes()
            if cpp:
                xd, plan = _planned(x, cfg)
                gap, nfpm = _cpp_call(cpp.nfp_pool_apply, xd, plan.desc_tensor, list(plan.oshape),
                                      max(plan.ask("nfp_pool_saved_floats"), 0), plan.nhwc, bool(want_gap), bool(need_grad))
            else:
                gap, nfpm = _NfpPoolHip.apply(x, cfg, bool(want_gap), bool(need_grad))
            return (gap if want_gap else None), nfpm
        except _abi.NfpUnsupported:
            pass    # (nfp_pool_supported is a dry run of both launchers; should it ever disagree, the composition serves)
    return (x.mean((2, 3)) if want_gap else None), nfp(x, cfg).mean((2, 3))


def nfp_pooled(x, cfg):
    """adaptive_avg_pool2d(NFPPooling(x), 1).flatten(1) — [B, N] float32 — as MobileNetV3_MultiStageNFP and MidNFP consume
    their NFP layers (models/texture_pooling.py:251-252, 320-321): no GAP(x) beside it.  On the GPU one pass over x that
    neither sums the channels of x nor, without a gradient to follow, stores the maps."""
    return nfp_pool(x, cfg, want_gap=False)[1]


def multi_radius_config(cfg1, cfg2):
    """The one configuration (R = 2, inner_R = 1) that stands for two which differ only in R / padding (radii 1 and 2,
    padding = R) and whose measure the two-radius kernels serve — else None."""
    import dataclasses
    if (cfg1.R == 1 and cfg2.R == 2 and cfg1.padding == 1 and cfg2.padding == 2
            and dataclasses.replace(cfg1, R=2, padding=2) == cfg2 and cfg2.inner_R == 0
            and cfg2.measure in ("cosine", "norm", "dot", "gfc", "rmse", "emd")):   # (norm: p = 1 or 2; else refused by the library)
        return dataclasses.replace(cfg2, inner_R=1)
    return None


def nfp_multi_radius(x, cfg1, cfg2):
    """torch.cat([NFP_R1(x), NFP_R2(x)], dim=1) for two configurations that differ only in R / padding (radii 1 and 2,
    padding = R): what MultiRadiusNFPHead.forward computes with two layers (models/nfp_heads.py:109-110).  On the GPU
    both radii come from ONE pass over x (and one backward pass) where the hot-path kernels serve the map; otherwise
    the two maps are computed one after the other."""
    xin, cast = _amp_input(x)       # (autocast / float16: the float32 upcast, also where the two layers run one by one)
    if xin is not x:
        with torch.autocast("cuda", enabled=False):
            out = nfp_multi_radius(xin, cfg1, cfg2)
        return out if cast is None else out.to(cast)
    cfg = multi_radius_config(cfg1, cfg2) if x.is_cuda and x.dim() == 4 else None
    if cfg is not None:
        try:
            return nfp(x, cfg)
        except _abi.NfpUnsupported:
            pass
    return torch.cat([nfp(x, cfg1), nfp(x, cfg2)], dim=1)


def _warn_scs():
    import warnings
    warnings.warn("NFP measure 'scs' (SharpenedCosine) mixes batch elements in the reference; it runs as "
                  "PyTorch ops on the GPU, not through the HIP kernels", RuntimeWarning, stacklevel=4)


def nfp(x, cfg):
    """[B,C,H,W] -> [B, k*k-1, H', W'] neighbour-similarity maps (NFPPooling.forward, nfp.py:132-134)."""
    if x.dim() != 4:
        raise RuntimeError(f"NFP expects a 4-D [B,C,H,W] feature map, got {tuple(x.shape)}")
    native = _autocast_native(x, cfg)
    if native is not None:
        xd, plan, mcfg = native
        need_grad = x.requires_grad and torch.is_grad_enabled()
        with torch.autocast("cuda", enabled=False):
            cpp = _cpp_nodes()
            if cpp:
                return _cpp_call(cpp.nfp_apply, xd, plan.desc_tensor, list(plan.oshape),
                                 _saved_len(plan, mcfg, x.dtype, need_grad), plan.nhwc)
            return _NfpHip.apply(xd, mcfg, need_grad)     # (xd is dense: the node's own `_dense` copies nothing)
    xin, cast = _amp_input(x)
    if xin is not x:
        with torch.autocast("cuda", enabled=False):
            out = nfp(xin, cfg)
        return out if cast is None else out.to(cast)
    if x.is_cuda and torch.compiler.is_compiling() and cfg.measure != "scs":
        # under torch.compile: the registered custom op (one node in the compiled graph, no graph break) — _ops.py
        from . import _ops
        need_grad = x.requires_grad and torch.is_grad_enabled()
        return torch.ops.nfp_amd.nfp(x, *_ops.cfg_args(cfg), bool(need_grad))[0]
    if x.is_cuda and cfg.measure == "scs":
        # The one measure without a kernel, on purpose: the reference's SharpenedCosine divides
        # (B,N,H,W) by (B,1,N,H,W) and so averages over the BATCH (nfp.py:359-374).  Its exact behaviour
        # is reproduced with torch ops on the tensor's own device, and said out loud; every other
        # measure on a CUDA tensor is served by libnfp_hip.so or raises.
        _warn_scs()
        return nfp_host(x, cfg)
    if x.is_cuda:
        need_grad = x.requires_grad and torch.is_grad_enabled()
        cpp = _cpp_nodes()
        if cpp:
            xd, plan = _planned(x, cfg)
            return _cpp_call(cpp.nfp_apply, xd, plan.desc_tensor, list(plan.oshape),
                             _saved_len(plan, cfg, x.dtype, need_grad), plan.nhwc)
        return _NfpHip.apply(x, cfg, need_grad)
    if cfg.inner_R:
        import dataclasses
        return torch.cat([nfp_host(x, dataclasses.replace(cfg, R=cfg.inner_R, padding=cfg.inner_R, inner_R=0)),
                          nfp_host(x, dataclasses.replace(cfg, inner_R=0))], dim=1)
    return nfp_host(x, cfg)


# ---- GAP(x) beside the full maps — the first step of an NFP head (include/nfp.h: nfp_gap_*) ------------------------------
def nfp_gap_fused_ok(x, cfg):
    """True when one pass can yield GAP(x) and the NFP maps of this call: the set `nfp_pool_fused_ok` describes and, for
    radii (1, 2) together (cfg.inner_R = 1), its maps of at most 512 pixels with C % 4 == 0 — the library's answer."""
    return cfg.measure != "scs" and _fused_ok(x, cfg, "nfp_gap_supported")


def gap_servable_static(shape, stride, dtype, cfg):
    """The trace-time form of `nfp_gap_fused_ok` (torch.compile: no data pointer, no workspace yet): nfp_gap_supported on
    the static shape and strides, with the workspace the descriptor is entitled to stood in for — a host-only dry run."""
    if dtype not in _DTYPES or len(shape) != 4 or cfg.measure == "scs":
        return False
    shape = tuple(int(v) for v in shape)
    st = tuple(int(v) for v in stride)
    if shape[0] == 1:
        st = (shape[1] * shape[2] * shape[3],) + st[1:]
    layout = _in_place_layout(shape, st, dtype.itemsize)
    if layout is None:
        return False
    L = _abi.load()
    d = build_desc(shape, _canon(shape, layout, st[0]), dtype, cfg)
    if int(L.nfp_workspace_bytes(ctypes.byref(d))) > 0:
        d.ws = 0x1000       # (never dereferenced: the dry run launches nothing)
    return bool(L.nfp_gap_supported(ctypes.byref(d)))


@torch.compiler.assume_constant_result
def _gap_servable_traced(shape, stride, dtype, cfg_fields):
    """`gap_servable_static` as Dynamo sees it: run at trace time on the static shape, its answer a constant of the graph."""
    from . import _ops
    return gap_servable_static(shape, stride, dtype, _ops._cfg(*cfg_fields))


def gap_servable(x, cfg):
    """Will `nfp_with_gap` run this CUDA call on the fused kernels?  `nfp_gap_fused_ok`, or under torch.compile its trace-time
    form.  For callers whose composition is not `nfp(x, cfg)` itself (NFPWithGap over two radii: the layer's own forward)."""
    if torch.compiler.is_compiling():
        from . import _ops
        return _gap_servable_traced(tuple(x.shape), tuple(x.stride()), x.dtype, _ops.cfg_args(cfg))
    return x.dim() == 4 and nfp_gap_fused_ok(x, cfg)


def gap_forward_call(x, cfg, ns=None):
    """(gap, maps, saved) from nfp_gap_forward on a call `nfp_gap_fused_ok` accepted; `saved` holds ns floats (at least
    nfp_gap_saved_floats) and is torch-allocated (graph-capture safe)."""
    L = _abi.load()
    xd, plan = _planned(x, cfg)
    d, oshape = plan.desc, plan.oshape
    need = max(plan.ask("nfp_gap_saved_floats"), 1)
    ns = need if ns is None else max(int(ns), need)
    with _on_device(x.device):
        gap = torch.empty(x.shape[0], x.shape[1], dtype=torch.float32, device=x.device)
        maps = torch.empty(oshape, dtype=x.dtype, device=x.device)
        saved = torch.empty(ns, dtype=torch.float32, device=x.device)
        _abi.check(L.nfp_gap_forward(ctypes.byref(d), xd.data_ptr(), gap.data_ptr(), maps.data_ptr(), saved.data_ptr(),
                                     saved.numel(), _raw_stream(x.device)))
    return gap, maps, saved


def gap_backward_call(x, cfg, maps, saved, grad_gap, grad_out):
    """grad_x from nfp_gap_backward.  grad_gap None: GAP(x) took no part in the loss (ggap = NULL in the library);
    grad_out None (only the mean was used): a zero map."""
    L = _abi.load()
    xd, plan = _planned(x, cfg)
    gg = grad_gap.contiguous().float() if grad_gap is not None else None
    go = torch.zeros_like(maps) if grad_out is None else _grad_out_as(grad_out, x.dtype)
    with _on_device(x.device):
        gx = _empty_grad_x(xd, plan.nhwc)
        _abi.check(L.nfp_gap_backward(ctypes.byref(plan.desc), xd.data_ptr(), gg.data_ptr() if gg is not None else None,
                                      go.data_ptr(), maps.data_ptr(), saved.data_ptr(), saved.numel(), gx.data_ptr(),
                                      _raw_stream(x.device)))
    return gx


class _NfpGapHip(torch.autograd.Function):
    """(gap [B,C] f32, maps [B,N,H,W]) in one pass over x; one backward kernel takes both gradients."""

    @staticmethod
    def forward(ctx, x, cfg):
        gap, maps, saved = gap_forward_call(x, cfg)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)    # an unused output arrives as None, not as a zero tensor
        ctx.save_for_backward(x, maps, saved)
        return gap, maps

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_gap, g_maps):
        x, maps, saved = ctx.saved_tensors
        if g_gap is None and g_maps is None:
            return None, None
        return gap_backward_call(x, ctx.cfg, maps, saved, g_gap, g_maps), None


def nfp_with_gap(x, cfg):
    """(GAP(x) [B,C] float32, NFP(x) [B,N,H',W']) — the first step of every NFP head (models/nfp_heads.py: `gap(fmap)` and
    `nfp(fmap)` of one feature map; with cfg.inner_R = 1 the 8 + 24 maps of radii 1 and 2, MultiRadiusNFPHead's
    concatenation).  On the GPU one pass over x yields both, and one backward kernel takes the gradients
    of both (either may be missing); where the fused kernels do not serve the call — CPU tensors, SCS, measures or
    geometries outside `nfp_pool`'s set — the composition `(x.mean((2, 3)).float(), nfp(x, cfg))`.  The maps come out typed
    exactly as `nfp(x, cfg)` types them."""
    if x.dim() != 4:
        raise RuntimeError(f"NFP expects a 4-D [B,C,H,W] feature map, got {tuple(x.shape)}")
    xin, cast = _amp_input(x)
    if xin is not x:
        with torch.autocast("cuda", enabled=False):
            gap, maps = nfp_with_gap(xin, cfg)
        return gap, (maps if cast is None else maps.to(cast))
    if x.is_cuda and torch.compiler.is_compiling():
        # under torch.compile: servability is decided NOW, on the static shape (a host-only dry run); a call the fused
        # kernels refuse is traced as the composition, so nothing can raise inside the compiled graph that eager serves
        from . import _ops
        if _gap_servable_traced(tuple(x.shape), tuple(x.stride()), x.dtype, _ops.cfg_args(cfg)):
            gap, maps, _ = torch.ops.nfp_amd.nfp_gap(x, *_ops.cfg_args(cfg))
            return gap, maps
    elif x.is_cuda and nfp_gap_fused_ok(x, cfg):
        try:
            if x.requires_grad and torch.is_grad_enabled():
                # the C++ node where the module has it (an older _nfp_torch.so: the Python node below)
                apply = getattr(_cpp_nodes() or None, "nfp_gap_apply", None)
                if apply is not None:
                    xd, plan = _planned(x, cfg)
                    gap, maps = _cpp_call(apply, xd, plan.desc_tensor, list(plan.oshape),
                                          max(plan.ask("nfp_gap_saved_floats"), 1), plan.nhwc)
                    return gap, maps
                return _NfpGapHip.apply(x, cfg)
            gap, maps, _ = gap_forward_call(x, cfg)
            return gap, maps
        except _abi.NfpUnsupported:
            pass    # (nfp_gap_supported is a dry run of both launchers; should it ever disagree, the composition serves)
    return x.mean((2, 3)).float(), nfp(x, cfg)


# ---- NFPPooling(bias=True) — include/nfp.h, ABI 7 (csrc/nfp_bias.hip) ------------------------------------------------------
def bias_no_centre(cfg):
    """Norm and RMSE never call center_value (nfp.py:141-148, 172-179): its bias gets no gradient (None, as in the reference)."""
    return cfg.measure in ("norm", "rmse")


def _bias_plan(x, layout, cfg):
    """The _Plan of a biased call — a plan of its own, without a workspace (the biased kernels keep no tables); its sizes
    are `ask("nfp_bias_saved_floats")` and `ask("nfp_bias_scratch_floats")`."""
    key = ("bias", tuple(x.shape), x.stride(0), layout, x.dtype, cfg, x.device.index)
    plan = _plans_get(key)
    if plan is None:
        plan = _Plan(make_desc(x, cfg, layout), layout)
        _plans_put(key, plan)
    return plan


def _bias_f32(t):
    return t.detach().float().contiguous()


def bias_forward_call(x, centre_bias, neighbour_bias, cfg):
    """(out, saved) from nfp_bias_forward; saved is torch-allocated (graph capture safe)."""
    L = _abi.load()
    xd, layout = _dense(x)
    plan = _bias_plan(xd, layout, cfg)
    d, oshape, ns = plan.desc, plan.oshape, plan.ask("nfp_bias_saved_floats")
    cb, nb = _bias_f32(centre_bias), _bias_f32(neighbour_bias)
    with _on_device(x.device):
        out = torch.empty(oshape, dtype=x.dtype, device=x.device)
        saved = torch.empty(max(ns, 0), dtype=torch.float32, device=x.device)
        _abi.check(L.nfp_bias_forward(ctypes.byref(d), xd.data_ptr(), cb.data_ptr(), nb.data_ptr(), out.data_ptr(),
                                      saved.data_ptr() if ns > 0 else None, max(ns, 0), _raw_stream(x.device)))
    return out, saved


def bias_backward_call(x, centre_bias, neighbour_bias, out, saved, grad_out, cfg):
    """(grad_x, grad_centre_bias or None for Norm / RMSE, grad_neighbour_bias) from nfp_bias_backward, the bias gradients
    float32 in the biases' shapes."""
    L = _abi.load()
    xd, layout = _dense(x)
    plan = _bias_plan(xd, layout, cfg)
    d, nsc = plan.desc, plan.ask("nfp_bias_scratch_floats")
    cb, nb = _bias_f32(centre_bias), _bias_f32(neighbour_bias)
    go = _grad_out_as(grad_out, x.dtype)
    with _on_device(x.device):
        gx = _empty_grad_x(xd, plan.nhwc)
        gcb = None if bias_no_centre(cfg) else torch.empty(cb.shape, dtype=torch.float32, device=x.device)
        gnb = torch.empty(nb.shape, dtype=torch.float32, device=x.device)
        scratch = torch.empty(max(nsc, 0), dtype=torch.float32, device=x.device)
        _abi.check(L.nfp_bias_backward(ctypes.byref(d), xd.data_ptr(), cb.data_ptr(), nb.data_ptr(), go.data_ptr(),
                                       out.data_ptr(), saved.data_ptr() if saved.numel() else None, saved.numel(),
                                       gx.data_ptr(), gcb.data_ptr() if gcb is not None else None, gnb.data_ptr(),
                                       scratch.data_ptr(), scratch.numel(), _raw_stream(x.device)))
    return gx, gcb, gnb


class _NfpBiasHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, centre_bias, neighbour_bias, cfg):
        out, saved = bias_forward_call(x, centre_bias, neighbour_bias, cfg)
        ctx.cfg = cfg
        ctx.save_for_backward(x, centre_bias, neighbour_bias, out, saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, cb, nb, out, saved = ctx.saved_tensors
        gx, gcb, gnb = bias_backward_call(x, cb, nb, out, saved, grad_out, ctx.cfg)
        return (gx, None if gcb is None else gcb.to(cb.dtype), gnb.to(nb.dtype), None)


def nfp_biased(x, cfg, centre_bias, neighbour_bias):
    """NFPPooling(bias=True).forward: `nfp` with the trainable biases of the reference's two convs — centre_bias [C]
    (center_value.bias) and neighbour_bias [C*N] (comp_neighbors.bias, nfp.py:42-58), added after padding.  CUDA tensors
    run the biased HIP kernels (include/nfp.h, ABI 7; SCS: torch ops, as `nfp`), CPU tensors `_host.nfp_host`.  Returns
    gradients for x and both biases (None for the centre bias of Norm / RMSE, which never read it)."""
    if x.dim() != 4:
        raise RuntimeError(f"NFP expects a 4-D [B,C,H,W] feature map, got {tuple(x.shape)}")
    if cfg.inner_R:
        raise ValueError("nfp_biased: one radius per call (inner_R = 0)")
    xin, cast = _amp_input(x)
    if xin is not x:
        with torch.autocast("cuda", enabled=False):
            out = nfp_biased(xin, cfg, centre_bias, neighbour_bias)
        return out if cast is None else out.to(cast)
    if x.is_cuda and cfg.measure == "scs":
        _warn_scs()
        return nfp_host(x, cfg, centre_bias, neighbour_bias)
    if x.is_cuda and torch.compiler.is_compiling():
        from . import _ops
        return torch.ops.nfp_amd.nfp_biased(x, centre_bias, neighbour_bias, *_ops.cfg_args(cfg))[0]
    if x.is_cuda:
        return _NfpBiasHip.apply(x, centre_bias, neighbour_bias, cfg)
    return nfp_host(x, cfg, centre_bias, neighbour_bias)


# ---- the softmax-pool tail of SimilarityAwarePooling — include/nfp.h: nfp_attpool_* (csrc/nfp_attpool.hip) ----------------
def attpool_forward_call(maps, w, b, need_grad):
    """(pooled [B,N] float32, att [B,P] float32 or None) from nfp_attpool_forward on dense CUDA maps [B,N,...] and float32
    w [N], b [1].  need_grad = False: att is not written (NULL in the library)."""
    L = _abi.load()
    B, N = maps.shape[:2]
    P = maps.numel() // (B * N)
    with _on_device(maps.device):
        pooled = torch.empty(B, N, dtype=torch.float32, device=maps.device)
        att = torch.empty(B, P, dtype=torch.float32, device=maps.device) if need_grad else None
        _abi.check(L.nfp_attpool_forward(B, N, P, _DTYPES[maps.dtype], maps.data_ptr(), w.data_ptr(), b.data_ptr(),
                                         pooled.data_ptr(), att.data_ptr() if need_grad else None, _raw_stream(maps.device)))
    return pooled, att


def attpool_backward_call(maps, w, att, grad_pooled, want_maps, want_w, want_b):
    """(grad_maps in the maps' dtype, grad_w [N], grad_b [1]) from nfp_attpool_backward — None for each gradient nobody
    wants (a NULL pointer in the library: neither computed nor written)."""
    L = _abi.load()
    B, N = maps.shape[:2]
    P = maps.numel() // (B * N)
    gp = grad_pooled.contiguous().float()
    with _on_device(maps.device):
        gm = torch.empty_like(maps) if want_maps else None
        gw = torch.empty(N, dtype=torch.float32, device=maps.device) if want_w else None
        gb = torch.empty(1, dtype=torch.float32, device=maps.device) if want_b else None
        ns = int(L.nfp_attpool_scratch_floats(B, N)) if (want_w or want_b) else 0
        scratch = torch.empty(ns, dtype=torch.float32, device=maps.device) if ns else None
        _abi.check(L.nfp_attpool_backward(B, N, P, _DTYPES[maps.dtype], maps.data_ptr(), w.data_ptr(), att.data_ptr(),
                                          gp.data_ptr(), gm.data_ptr() if want_maps else None,
                                          gw.data_ptr() if want_w else None, gb.data_ptr() if want_b else None,
                                          scratch.data_ptr() if ns else None, ns, _raw_stream(maps.device)))
    return gm, gw, gb


class _AttPoolHip(torch.autograd.Function):
    """pooled [B,N] float32 of dense CUDA maps and float32 (w [N], b [1]); one kernel each way plus the batch reduce of the
    parameters' gradients.  need_grad: some input requires a gradient and grad mode is on, sampled by the caller."""

    @staticmethod
    def forward(ctx, maps, w, b, need_grad):
        pooled, att = attpool_forward_call(maps, w, b, need_grad)
        if need_grad:
            ctx.save_for_backward(maps, w, att)
        return pooled

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_pooled):
        maps, w, att = ctx.saved_tensors
        want = ctx.needs_input_grad
        gm, gw, gb = attpool_backward_call(maps, w, att, grad_pooled, want[0], want[1], want[2])
        return gm, gw, gb, None


def _attpool_hip_serves(maps):
    """The HIP tail serves dense CUDA float32 / bfloat16 maps of a non-empty batch, outside torch.compile (where the tail is
    traced as ATen ops), unless NFP_SAP_TORCH=1 (read at call time) asks for the torch formulation."""
    return (not torch.compiler.is_compiling() and maps.is_cuda and maps.dtype in _DTYPES and maps.is_contiguous()
            and maps.shape[0] > 0 and os.environ.get("NFP_SAP_TORCH") != "1")


def nfp_attention_pool(maps, weight, bias):
    """SimilarityAwarePooling's tail (models/nfp_heads.py:224-232): maps [B,N,H',W'] (or [B,N,P]) -> [B,N], the maps summed
    under softmax_over_pixels(att_proj(maps)), att_proj a 1x1 conv N -> 1 given by weight ([1,N,1,1] or [N]) and bias [1].
    Dense CUDA float32 / bfloat16 maps run one HIP kernel each way (include/nfp.h: nfp_attpool_*; float32 arithmetic, the
    result cast once to the maps' dtype; gradients for the maps, the weight and the bias, each only where wanted);
    everything else — CPU, float16, float64, strided maps, torch.compile, NFP_SAP_TORCH=1 — the torch formulation
    `_host.attention_pool_host`.  Under torch.autocast the inputs are taken as float32 and the result is float32, the
    reference's output type there (its softmax is on autocast's float32 list)."""
    if maps.dim() < 3:
        raise RuntimeError(f"nfp_attention_pool expects [B,N,H,W] (or [B,N,P]) maps, got {tuple(maps.shape)}")
    if weight.numel() != maps.shape[1] or bias.numel() != 1:
        raise RuntimeError(f"nfp_attention_pool: {maps.shape[1]} maps need a weight of {maps.shape[1]} elements and a bias "
                           f"of 1, got {tuple(weight.shape)} and {tuple(bias.shape)}")
    if maps.is_cuda and torch.is_autocast_enabled("cuda"):
        with torch.autocast("cuda", enabled=False):
            return nfp_attention_pool(maps.float(), weight.float(), bias.float())
    if not _attpool_hip_serves(maps):
        return attention_pool_host(maps, weight, bias)
    need_grad = torch.is_grad_enabled() and (maps.requires_grad or weight.requires_grad or bias.requires_grad)
    pooled = _AttPoolHip.apply(maps, weight.reshape(-1).float().contiguous(), bias.reshape(-1).float(), need_grad)
    return pooled if pooled.dtype == maps.dtype else pooled.to(maps.dtype)


# ---- valid maps: stride 1, dilation 1, padding 0 — include/nfp.h: nfp_valid_* (csrc/nfp_valid.hip) -------------------------
def _valid_plan(x, layout, cfg):
    """The _Plan of a valid-map call — a plan of its own, without a workspace (the kernels keep no tables); what the library
    says about it is `ask("nfp_valid_supported")` and `ask("nfp_valid_saved_floats")`."""
    key = ("valid", tuple(x.shape), x.stride(0), layout, x.dtype, cfg, x.device.index)
    plan = _plans_get(key)
    if plan is None:
        plan = _Plan(make_desc(x, cfg, layout), layout)
        _plans_put(key, plan)
    return plan


def _valid_layout(x, cfg, family="valid"):
    """The layout in which fwd_valid / bwd_valid read this call in place, or None where `nfp` serves it: NFP_VALID_OFF=1
    (read at call time), torch.compile, a CPU tensor, another dtype, images that are not dense, or a descriptor
    nfp_valid_supported refuses (another measure, rows above 128 pixels, channels-last maps off the alignment rule).
    family="valid_abs": the same question to nfp_valid_abs_supported (Norm p=1 on the difference weights, EMD), whose plan
    has a cache key of its own."""
    if (torch.compiler.is_compiling() or not (x.is_cuda and x.dtype in _DTYPES) or cfg.inner_R or cfg.map_f32
            or os.environ.get("NFP_VALID_OFF") == "1"):
        return None
    if not hasattr(_abi.load(), f"nfp_{family}_forward"):  # (an older library loaded for an A/B run)
        return None
    layout = _in_place_layout(x.shape, x.stride(), x.element_size(), x.data_ptr())
    if layout is None:
        return None
    plan = _valid_plan(x, layout, cfg) if family == "valid" else _valid_abs_plan(x, layout, cfg)
    return layout if plan.ask(f"nfp_{family}_supported") else None


def valid_forward_call(x, layout, cfg, need_grad):
    """(out, saved, plan) from nfp_valid_forward on a call `_valid_layout` accepted; `saved` (|x| per pixel for cosine / gfc)
    is kept only with a backward to follow."""
    L = _abi.load()
    plan = _valid_plan(x, layout, cfg)
    ns = max(plan.ask("nfp_valid_saved_floats"), 0) if need_grad else 0
    with _on_device(x.device):
        out = torch.empty(plan.oshape, dtype=x.dtype, device=x.device)
        saved = torch.empty(ns, dtype=torch.float32, device=x.device)
        _abi.check(L.nfp_valid_forward(ctypes.byref(plan.desc), x.data_ptr(), out.data_ptr(),
                                       saved.data_ptr() if ns > 0 else None, ns, _raw_stream(x.device)))
    return out, saved, plan


def valid_backward_call(x, plan, out, saved, grad_out):
    """grad_x from nfp_valid_backward: dense, in x's inner layout."""
    L = _abi.load()
    go = _grad_out_as(grad_out, out.dtype)
    with _on_device(x.device):
        gx = _empty_grad_x(x, plan.nhwc)
        _abi.check(L.nfp_valid_backward(ctypes.byref(plan.desc), x.data_ptr(), go.data_ptr(), out.data_ptr(),
                                        saved.data_ptr() if saved.numel() else None, saved.numel(), gx.data_ptr(),
                                        _raw_stream(x.device)))
    return gx


class _NfpValidHip(torch.autograd.Function):
    """The maps of an unpadded layer: one fwd_valid launch, one bwd_valid launch."""

    @staticmethod
    def forward(ctx, x, layout, cfg, need_grad):
        out, saved, ctx.plan = valid_forward_call(x, layout, cfg, need_grad)
        if need_grad:
            ctx.save_for_backward(x, out, saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, out, saved = ctx.saved_tensors
        return valid_backward_call(x, ctx.plan, out, saved, grad_out), None, None, None


def _valid_abs_plan(x, layout, cfg):
    """The _Plan of a call on the valid-map kernels' L1 family (nfp_valid_abs_*): the descriptor of `_valid_plan`, cached
    under a key of its own."""
    key = ("valid_abs", tuple(x.shape), x.stride(0), layout, x.dtype, cfg, x.device.index)
    plan = _plans_get(key)
    if plan is None:
        plan = _Plan(make_desc(x, cfg, layout), layout)
        _plans_put(key, plan)
    return plan


def valid_abs_forward_call(x, layout, cfg):
    """(out, plan) from nfp_valid_abs_forward on a call `_valid_layout(..., "valid_abs")` accepted: nothing is saved."""
    L = _abi.load()
    plan = _valid_abs_plan(x, layout, cfg)
    with _on_device(x.device):
        out = torch.empty(plan.oshape, dtype=x.dtype, device=x.device)
        _abi.check(L.nfp_valid_abs_forward(ctypes.byref(plan.desc), x.data_ptr(), out.data_ptr(), _raw_stream(x.device)))
    return out, plan


def valid_abs_backward_call(x, plan, grad_out):
    """grad_x from nfp_valid_abs_backward — of x and grad_out alone: dense, in x's inner layout."""
    L = _abi.load()
    go = _grad_out_as(grad_out, x.dtype)
    with _on_device(x.device):
        gx = _empty_grad_x(x, plan.nhwc)
        _abi.check(L.nfp_valid_abs_backward(ctypes.byref(plan.desc), x.data_ptr(), go.data_ptr(), gx.data_ptr(),
                                            _raw_stream(x.device)))
    return gx


class _NfpValidAbsHip(torch.autograd.Function):
    """The maps of an unpadded L1 layer: one fwd_valid<..l1..> launch, one bwd_valid<..l1..> launch.  Saves x alone — the
    pair coefficient of a sum of |a - b| is -+ grad_out — so the maps it returns may be modified in place."""

    @staticmethod
    def forward(ctx, x, layout, cfg, need_grad):
        out, ctx.plan = valid_abs_forward_call(x, layout, cfg)
        if need_grad:
            ctx.save_for_backward(x)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (x,) = ctx.saved_tensors
        return valid_abs_backward_call(x, ctx.plan, grad_out), None, None, None


def _measure_is_abs(cfg):
    """Norm p=1 on the difference weights, or EMD: what nfp_valid_abs_* serves and nfp_valid_* refuses by its measure."""
    return cfg.measure == "emd" or (cfg.measure == "norm" and cfg.p == 1 and cfg.diff_weights)


def nfp_valid(x, cfg):
    """`nfp(x, cfg)` for an unpadded layer — cfg.padding == 0, stride 1, dilation 1 (ValueError otherwise): [B,C,H,W] ->
    [B, k*k-1, H-2R, W-2R], as models/nfp_heads.py::NFPBottleneck runs it inside every block.  A CUDA call that
    nfp_valid_supported accepts (cosine / dot / gfc / Norm p=2 / rmse, float32 or bfloat16, rows of at most 128 pixels,
    NCHW or aligned channels-last images) runs the valid-map kernels, one launch each way.  So does one that
    nfp_valid_abs_supported accepts: Norm p=1 on the difference weights — the reference's default layer, NFPInsert's — and
    EMD, under the same shape rules (fwd_valid<..l1..> / bwd_valid<..l1..>).  Everything else — CPU tensors, other
    measures, refused shapes, torch.compile, NFP_VALID_OFF=1 in the environment (read at call time) — is `nfp(x, cfg)`
    unchanged.  Under torch.autocast, and for float16 / float64, the float32 upcast of `_amp_input`, as the fused callers.

    The L1 node saves x ALONE (its backward reads neither the maps nor a statistic): the returned maps may be modified in
    place before the backward.  The maps of the other measures are saved for the backward and must not be."""
    if cfg.padding != 0 or cfg.stride != 1 or cfg.dilation != 1:
        raise ValueError(f"nfp_valid: padding 0, stride 1, dilation 1 only (got padding={cfg.padding}, "
                         f"stride={cfg.stride}, dilation={cfg.dilation}); use nfp")
    if x.dim() != 4:
        raise RuntimeError(f"NFP expects a 4-D [B,C,H,W] feature map, got {tuple(x.shape)}")
    xin, cast = _amp_input(x)
    if xin is not x:
        with torch.autocast("cuda", enabled=False):
            out = nfp_valid(xin, cfg)
        return out if cast is None else out.to(cast)
    layout = _valid_layout(x, cfg)
    if layout is None and _measure_is_abs(cfg):
        layout = _valid_layout(x, cfg, "valid_abs")
        if layout is not None:
            need_grad = bool(x.requires_grad and torch.is_grad_enabled())
            apply = getattr(_cpp_nodes() or None, "nfp_valid_abs_apply", None)
            if apply is not None and x.shape[0] > 0:
                plan = _valid_abs_plan(x, layout, cfg)
                return _cpp_call(apply, x, plan.desc_tensor, list(plan.oshape), plan.nhwc, need_grad)
            return _NfpValidAbsHip.apply(x, layout, cfg, need_grad)
    if layout is None:
        return nfp(x, cfg)
    need_grad = bool(x.requires_grad and torch.is_grad_enabled())
    # the C++ node where the module has it (an older _nfp_torch.so, or NFP_PY_NODES=1: the Python node)
    apply = getattr(_cpp_nodes() or None, "nfp_valid_apply", None)
    if apply is not None and x.shape[0] > 0:
        plan = _valid_plan(x, layout, cfg)
        ns = max(plan.ask("nfp_valid_saved_floats"), 0) if need_grad else 0
        return _cpp_call(apply, x, plan.desc_tensor, list(plan.oshape), ns, plan.nhwc)
    return _NfpValidHip.apply(x, layout, cfg, need_grad)


# ---- the heads' compress-BN-ReLU-GAP tail — include/nfp.h: nfp_cpool_* (csrc/nfp_cpool.hip) — and the same projection
# ---- with the map kept — nfp_cproj_* (the cproj kernels): one call path, one autograd node and one set of checks for both
CPOOL_MAX_MAPS = 32     # csrc/nfp_cp_kernels.h: kCpMaxN (a lane keeps two weight rows in registers)
CPOOL_ROUTED_MAPS = 8   # what cpool_hip_serves takes by default: the maps counts that measured faster than the composition
CPOOL_WIDE_MAX_MAPS = 96    # csrc/nfp_cp_kernels.h: kWMaxN (the cpw kernels: rows and maps in LDS, a tile of outputs per lane)
# What cpool_wide_serves takes by default: the (maps, B * P) classes scripts/bench_heads.py measured faster than the
# composition beyond the run-to-run spread on an MI355X ("The wide form") — none: [64,48,7,7] 0.35x, [256,48,7,7]
# 0.60x, [256,80,7,7] 0.42x, [64,48,14,14] 0.49x (-> 512, train-mode forward + backward, graph-timed), so 33 to 96 maps reach
# the wide kernels with NFP_CPOOL_TORCH=0 only.
CPOOL_WIDE_ROUTED_CLASSES = ()      # ((min maps, max maps, min B * P), ...)
# the three kinds' library calls: (forward, backward, the scratch length query)
_CP_ENTRIES = {"pool": ("nfp_cpool_forward", "nfp_cpool_backward", "nfp_cpool_scratch_floats"),
               "wide": ("nfp_cpool_wide_forward", "nfp_cpool_wide_backward", "nfp_cpool_wide_scratch_floats"),
               "proj": ("nfp_cproj_forward_fmt", "nfp_cproj_backward_fmt", "nfp_cproj_scratch_floats")}


# ---- what every call of the family is assembled from, on one rank's statistics or across ranks ----
def _cp_sizes(maps, D, empty_rank=False):
    """(B, N, P, D) of maps [B,N,...]; empty_rank (the nfp_cpsync_* entries): a rank without a value is B = 0 with one pixel."""
    B, N = maps.shape[:2]
    P = maps.shape[2:].numel()
    if empty_rank:
        return (B, N, P, D) if P > 0 else (0, N, 1, D)
    return B, N, (P if B * N else 0), D


def _ptr(t):
    """The pointer the library is handed for `t`: NULL for None and for a tensor without an element."""
    return (t.data_ptr() or None) if t is not None else None


def _cp_in_format(y, channels_last):
    return y.contiguous(memory_format=torch.channels_last) if channels_last else y


def _cp_out(kind, maps, D, channels_last=False):
    """The result of one call, uninitialised: [B,D] float32, or for "proj" [B,D,...] in the maps' dtype and the asked layout."""
    if kind != "proj":
        return torch.empty(maps.shape[0], D, dtype=torch.float32, device=maps.device)
    return torch.empty((maps.shape[0], D) + tuple(maps.shape[2:]), dtype=maps.dtype, device=maps.device,
                       memory_format=torch.channels_last if channels_last else torch.contiguous_format)


def _cp_grad_out(kind, maps, grad_out):
    """(grad_out as the library reads it, whether that is channels-last): dense float32, or for "proj" the maps' dtype in
    the layout it arrives in (cproj_backward_call)."""
    if kind != "proj":
        return grad_out.contiguous().float(), False
    go = grad_out.to(maps.dtype)        # (preserve_format: a dense tensor keeps its layout)
    nhwc = not go.is_contiguous() and go.dim() == 4 and go.is_contiguous(memory_format=torch.channels_last)
    return (go if nhwc else go.contiguous()), nhwc


def _cp_grads(maps, D, want):
    """(grad_maps like the maps, grad_w [D,N], grad_gamma [D], grad_beta [D]), uninitialised — None for each `want` leaves out."""
    dev = maps.device
    return (torch.empty_like(maps) if want[0] else None,
            torch.empty(D, maps.shape[1], dtype=torch.float32, device=dev) if want[1] else None,
            torch.empty(D, dtype=torch.float32, device=dev) if want[2] else None,
            torch.empty(D, dtype=torch.float32, device=dev) if want[3] else None)


def _cp_scratch(kind, sizes, backward, need, device):
    """(scratch, its length) as the length query of `kind` sizes it; (None, 0) where the call needs none."""
    n = int(getattr(_abi.load(), _CP_ENTRIES[kind][2])(*sizes, int(backward))) if need else 0
    return (torch.empty(n, dtype=torch.float32, device=device) if n else None), n


def _cp_invoke(kind, backward, maps, w, gamma, beta, use_batch_stats, relu, nhwc, need_scratch, middle):
    """One call of a _CP_ENTRIES function, on the maps' device — the one place its argument list is built: the sizes, dtype
    and mode (proj: relu), the maps and parameters, `middle` (the direction's own arguments), the scratch with its length,
    the stream (proj: the layout of out / grad_out)."""
    sizes = _cp_sizes(maps, w.shape[0])
    proj = kind == "proj"
    scratch, nscr = _cp_scratch(kind, sizes, backward, need_scratch, maps.device)
    args = [*sizes, _DTYPES[maps.dtype], int(bool(use_batch_stats))] + ([int(bool(relu))] if proj else [])
    args += [_ptr(maps), w.data_ptr(), gamma.data_ptr(), beta.data_ptr(), *middle, _ptr(scratch), nscr, _raw_stream(maps.device)]
    args += [_abi.ACT_NHWC if nhwc else _abi.ACT_NCHW] if proj else []
    _abi.check(getattr(_abi.load(), _CP_ENTRIES[kind][int(backward)])(*args))


def _cp_forward_call(kind, maps, w, gamma, beta, rm, rv, use_batch_stats, momentum, eps, relu=True, nhwc=False):
    """(out, saved) of the forward of `kind`; saved: the O(N*N + D) state the backward reads (None in eval)."""
    N, D = maps.shape[1], w.shape[0]
    with _on_device(maps.device):
        out = _cp_out(kind, maps, D, nhwc)
        ns = int(_abi.load().nfp_cpool_saved_floats(N, D)) if use_batch_stats else 0
        saved = torch.empty(ns, dtype=torch.float32, device=maps.device) if ns else None
        _cp_invoke(kind, False, maps, w, gamma, beta, use_batch_stats, relu, nhwc, use_batch_stats,
                   [_ptr(rm), _ptr(rv), float(momentum), float(eps), _ptr(out), _ptr(saved), ns])
    return out, saved


def _cp_backward_call(kind, maps, w, gamma, beta, rm, rv, saved, use_batch_stats, eps, grad_out, want, relu=True):
    """(grad_maps, grad_w, grad_gamma, grad_beta) of `kind` (_cp_grads) under grad_out (_cp_grad_out)."""
    go, nhwc = _cp_grad_out(kind, maps, grad_out)
    with _on_device(maps.device):
        grads = _cp_grads(maps, w.shape[0], want)
        sums = use_batch_stats or want[1] or want[2] or want[3]
        _cp_invoke(kind, True, maps, w, gamma, beta, use_batch_stats, relu, nhwc, sums,
                   [None if use_batch_stats else _ptr(rm), None if use_batch_stats else _ptr(rv), float(eps), _ptr(saved),
                    saved.numel() if saved is not None else 0, _ptr(go), *map(_ptr, grads)])
    return grads


def cpool_forward_call(maps, w, gamma, beta, rm, rv, use_batch_stats, momentum, eps, kind="pool"):
    """(out [B,D] float32, saved) from nfp_cpool_forward on dense CUDA maps [B,N,...] and float32 w [D,N], gamma, beta [D].
    use_batch_stats: train-mode statistics, the running ones (float32 [D], or both None) updated by the same call; `saved`
    is then the O(N*N + D) state the backward reads (None in eval, where rm / rv stand for the statistics).
    kind="wide": nfp_cpool_wide_forward (up to 96 maps), the same arguments and `saved`."""
    return _cp_forward_call(kind, maps, w, gamma, beta, rm, rv, use_batch_stats, momentum, eps)


def cpool_backward_call(maps, w, gamma, beta, rm, rv, saved, use_batch_stats, eps, grad_out, want, kind="pool"):
    """(grad_maps in the maps' dtype, grad_w [D,N], grad_gamma [D], grad_beta [D]) from nfp_cpool_backward — None for each
    gradient `want` (four flags) leaves out: a NULL pointer in the library, neither computed nor written.  kind="wide":
    nfp_cpool_wide_backward, on the `saved` of a wide forward."""
    return _cp_backward_call(kind, maps, w, gamma, beta, rm, rv, saved, use_batch_stats, eps, grad_out, want)


class _CpHip(torch.autograd.Function):
    """What the nodes of both kinds share, on dense CUDA maps and float32 (w [D,N], gamma [D], beta [D]).  Saved for the
    backward: the maps, the three parameters and the O(N*N + D) statistics — nothing of the size of the [B,D,P]
    activation, and not the output.  `stats` = (rm, rv), the running statistics or (None, None): buffers the forward kernel
    updates in place, handed over outside autograd's view.  need_grad: some input requires a gradient and grad mode is on,
    sampled by the caller."""

    @staticmethod
    def _save(ctx, maps, w, gamma, beta, saved, stats, use_batch_stats, eps):
        ctx.save_for_backward(maps, w, gamma, beta, *([saved] if saved is not None else []))
        ctx.stats, ctx.use_batch_stats, ctx.eps = stats, use_batch_stats, eps

    @staticmethod
    def _state(ctx):
        """The leading arguments of c*_backward_call: (maps, w, gamma, beta, rm, rv, saved, use_batch_stats, eps)."""
        saved = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
        return (*ctx.saved_tensors[:4], ctx.stats[0], ctx.stats[1], saved, ctx.use_batch_stats, ctx.eps)


class _CPoolHip(_CpHip):
    """out [B,D] float32; kind: "pool" or "wide"."""

    @staticmethod
    def forward(ctx, maps, w, gamma, beta, stats, use_batch_stats, momentum, eps, need_grad, kind):
        out, saved = cpool_forward_call(maps, w, gamma, beta, stats[0], stats[1], use_batch_stats, momentum, eps, kind)
        if need_grad:
            _CpHip._save(ctx, maps, w, gamma, beta, saved, stats, use_batch_stats, eps)
            ctx.kind = kind
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        grads = cpool_backward_call(*_CpHip._state(ctx), grad_out, ctx.needs_input_grad[:4], ctx.kind)
        return (*grads, None, None, None, None, None, None)


def _cp_can_serve(maps, gamma, beta, momentum, max_maps=CPOOL_MAX_MAPS):
    """What the kernels of every kind can serve: dense CUDA float32 / bfloat16 maps [B >= 1, N <= max_maps, ...] under an affine
    BatchNorm with a float momentum, outside torch.compile and torch.autocast."""
    return (not torch.compiler.is_compiling() and maps.is_cuda and not torch.is_autocast_enabled("cuda")
            and maps.dtype in _DTYPES and maps.is_contiguous() and maps.shape[0] > 0 and 1 <= maps.shape[1] <= max_maps
            and maps.numel() > 0 and gamma is not None and beta is not None and isinstance(momentum, float))


def _cp_check_args(name, maps, weight, use_batch_stats, running_mean, running_var):
    if maps.dim() < 3:
        raise RuntimeError(f"{name} expects [B,N,H,W] (or [B,N,P]) maps, got {tuple(maps.shape)}")
    if weight.dim() < 2 or weight.shape[1] != maps.shape[1] or weight.numel() != weight.shape[0] * maps.shape[1]:
        raise RuntimeError(f"{name}: {maps.shape[1]} maps need a 1x1 conv weight [D,{maps.shape[1]},1,1], got "
                           f"{tuple(weight.shape)}")
    if not use_batch_stats and (running_mean is None or running_var is None):
        raise RuntimeError(f"{name}: without batch statistics the running mean and variance are required")


def _cp_prepare(maps, weight, gamma, beta, rm, rv, own_stats):
    """What a served call hands its node: float32, contiguous (w [D,N], gamma, beta) — or None where the running statistics
    are not float32 and contiguous, which is the host composition's.  own_stats (batch statistics of this rank alone):
    ValueError as F.batch_norm raises it for a single value per channel in training."""
    B, N = maps.shape[:2]
    D = weight.shape[0]
    if own_stats and maps.numel() // N == 1:     # torch/nn/functional.py::_verify_batch_size, on the conv's output
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {torch.Size([B, D, 1, 1])}")
    if rm is not None and (rm.dtype != torch.float32 or rv.dtype != torch.float32 or not rm.is_contiguous() or not rv.is_contiguous()):
        return None
    f32 = lambda t: t if t.dtype == torch.float32 else t.float()     # noqa: E731
    return f32(weight).reshape(D, N).contiguous(), f32(gamma).contiguous(), f32(beta).contiguous()


def _bn_call_mode(bn, training):
    """(use_batch_stats, rm, rv, factor) of one call of `bn` in mode `training`, as nn.modules.batchnorm._BatchNorm.forward
    decides them — num_batches_tracked moved on by it.  factor: None with a float bn.momentum; with momentum=None the
    cumulative average's factor, a function of the step count (the composition's to apply)."""
    factor = 0.0 if bn.momentum is None else None
    if training and bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
        if bn.momentum is None:
            factor = 1.0 / float(bn.num_batches_tracked)
    use_batch_stats = training or (bn.running_mean is None and bn.running_var is None)
    track = not training or bn.track_running_stats
    rm, rv = (bn.running_mean, bn.running_var) if track else (None, None)
    return use_batch_stats, rm, rv, factor


def cpool_hip_serves(maps, gamma, beta, momentum):
    """The HIP tail can serve dense CUDA float32 / bfloat16 maps [B >= 1, N <= 32, ...] under an affine BatchNorm with a float
    momentum, outside torch.compile and torch.autocast.  Of those it takes, by default, the ones with at most 8 maps: with 32
    maps it measured slower than the torch composition ([256,32,7,7] -> 512: 327 against 185 us graph-timed), and
    16 and 24 maps run the same register-heavy forms (measured since: 161 against 157 and 248 against 167 us).  NFP_CPOOL_TORCH (read at call time) is the A/B
    switch: "1" the torch composition everywhere, "0" the HIP tail wherever it can serve."""
    env = os.environ.get("NFP_CPOOL_TORCH")
    if env == "1":
        return False
    return _cp_can_serve(maps, gamma, beta, momentum) and (env == "0" or maps.shape[1] <= CPOOL_ROUTED_MAPS)


def cpool_wide_serves(maps, gamma, beta, momentum):
    """The wide HIP tail (nfp_cpool_wide_*) can serve what cpool_hip_serves describes with up to 96 maps.  It is asked after
    cpool_hip_serves has declined, and takes by default the classes of CPOOL_WIDE_ROUTED_CLASSES (none so far), so 33 to 96
    maps run it under NFP_CPOOL_TORCH=0 and the composition otherwise.  NFP_CPOOL_WIDE=1 (read at call time, for
    measurement): 9 to 32 maps run the wide form too, wherever the tail is served — it is then asked first."""
    env = os.environ.get("NFP_CPOOL_TORCH")
    if env == "1" or not _cp_can_serve(maps, gamma, beta, momentum, CPOOL_WIDE_MAX_MAPS):
        return False
    N, M = maps.shape[1], maps.numel() // maps.shape[1]
    return env == "0" or any(lo <= N <= hi and M >= m for lo, hi, m in CPOOL_WIDE_ROUTED_CLASSES)


def _cpool_kind(maps, gamma, beta, momentum):
    """"pool", "wide" or None (the composition) for one call of the tail."""
    hip = cpool_hip_serves(maps, gamma, beta, momentum)
    if hip and not (os.environ.get("NFP_CPOOL_WIDE") == "1" and maps.shape[1] > CPOOL_ROUTED_MAPS):
        return "pool"
    if hip or cpool_wide_serves(maps, gamma, beta, momentum):
        return "wide"
    return None


def nfp_compress_pool_tensors(maps, weight, gamma, beta, running_mean, running_var, use_batch_stats, momentum=0.1, eps=1e-5,
                              *, process_group=None):
    """`nfp_compress_pool` on loose tensors: maps [B,N,H,W] (or [B,N,P]) -> [B,D] = GAP(relu(batch_norm(conv1x1(maps)))), the
    1x1 conv given by weight ([D,N,1,1] or [D,N]), the BatchNorm by gamma / beta [D] (None: affine=False), its running
    statistics (updated in place when use_batch_stats; both None: not tracked) and `momentum` — the exponential factor
    F.batch_norm takes; None, a cumulative average, is the caller's to resolve.  use_batch_stats=False reads the running
    statistics instead (eval).  Where `cpool_hip_serves`, three HIP launches forward and at most three backward that never form
    the [B,D,H,W] activation (include/nfp.h: nfp_cpool_*; float32 arithmetic, the result cast once to the maps' dtype);
    where it does not and `cpool_wide_serves` (33 to 96 maps under NFP_CPOOL_TORCH=0), the wide kernels: five launches
    forward, at most three backward (nfp_cpool_wide_*); everything else — by default also more than 8 maps, see
    cpool_hip_serves — is `_host.compress_pool_host`.
    process_group: a torch.distributed group of more than one rank over whose batches the batch statistics are taken
    (`_cp_sync_tensors_call`); None, a one-rank group or use_batch_stats=False: this rank's alone, as above."""
    _cp_check_args("nfp_compress_pool", maps, weight, use_batch_stats, running_mean, running_var)
    if _cp_sync_applies(process_group, use_batch_stats):
        return _cp_sync_tensors_call("pool", maps, weight, gamma, beta, running_mean, running_var, momentum, eps, process_group)
    kind = _cpool_kind(maps, gamma, beta, momentum)
    prepared = kind and _cp_prepare(maps, weight, gamma, beta, running_mean, running_var, use_batch_stats)
    if not prepared:
        return compress_pool_host(maps, weight, gamma, beta, running_mean, running_var, use_batch_stats, momentum, eps)
    need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (maps, weight, gamma, beta))
    out = _CPoolHip.apply(maps, *prepared, (running_mean, running_var), bool(use_batch_stats), float(momentum), float(eps),
                          need_grad, kind)
    return out if out.dtype == maps.dtype else out.to(maps.dtype)


def nfp_compress_pool(maps, weight, bn, training=None):
    """The tail the trained heads of models/nfp_heads.py share behind their NFP maps (NFPHead nfp_heads.py:28-32,42-43;
    MultiRadiusNFPHead 98-102,114-115; AdaptiveFusionNFP 301-305,323-324): maps [B,N,H,W] -> [B,D] =
    GAP(relu(bn(conv1x1(maps)))), `weight` the 1x1 conv's ([D,N,1,1], no bias) and `bn` its nn.BatchNorm2d — whose mode
    (`training`: None = bn.training), running statistics and num_batches_tracked are used and updated exactly as
    bn.forward does.  An nn.SyncBatchNorm takes its batch statistics over every rank of its process group where
    SyncBatchNorm.forward would (cp_sync_group): see "SyncBatchNorm in the two tails" below.
    See nfp_compress_pool_tensors."""
    training = bn.training if training is None else bool(training)
    group = cp_sync_group(bn, training)         # (asked before the step counter moves)
    if group is not None:
        return _cp_sync_module_call("pool", maps, weight, bn, training, group)
    use_batch_stats, rm, rv, factor = _bn_call_mode(bn, training)
    if factor is not None:
        return compress_pool_host(maps, weight, bn.weight, bn.bias, rm, rv, use_batch_stats, factor, bn.eps)
    return nfp_compress_pool_tensors(maps, weight, bn.weight, bn.bias, rm, rv, use_batch_stats, float(bn.momentum), bn.eps)


# What cproj_hip_serves takes by default — the classes scripts/bench_insert.py measured faster than the composition beyond
# the run-to-run spread on an MI355X: with at most 8 maps, the forward that keeps no state for a backward on
# running statistics (every row: 1.9x to 4.0x), and the train-mode step from 64 images of 54 x 54 map pixels up
# ([64,8,54,54] -> 24: 1.49x, -> 64 without the ReLU: 1.41x, [64,8,110,110] -> 16: 2.13x).  The smaller train-mode rows
# lost (0.64x to 0.96x), and so did the 24-map step (0.42x): the composition's.
CPROJ_ROUTED_MAPS = 8
CPROJ_ROUTED_TRAIN_PIXELS = 64 * 54 * 54      # B * P of the smallest train-mode row that won
# A channels-last result (memory_format=torch.channels_last) has its own measurement, scripts/bench_insert.py
# --channels-last (float32 and bf16 alike), routed by the same rule: the forward on running statistics that no
# backward follows won every row, the 24-map one included (1.5x to 5.7x); the train-mode step won with 8 maps from 256
# images of 12 x 12 map pixels up ([256,8,12,12] -> 256 without the ReLU: 1.66x, [64,8,26,26] -> 40: 1.13x, up to 2.44x at
# [64,8,110,110] -> 16) and lost or tied below that ([64,8,12,12] and [64,8,5,5]: 0.75x to 1.0x) and with 24 maps (0.50x).
CPROJ_ROUTED_NHWC_EVAL_MAPS = 24
CPROJ_ROUTED_NHWC_TRAIN_PIXELS = 256 * 12 * 12    # B * P of the smallest channels-last train-mode row that won


def _cproj_memory_format(memory_format, maps):
    """True for torch.channels_last, False for torch.contiguous_format; ValueError for anything else and for channels_last
    on maps that are not [B,N,H,W]."""
    if memory_format == torch.contiguous_format:
        return False
    if memory_format != torch.channels_last:
        raise ValueError(f"nfp_compress_map: memory_format must be torch.contiguous_format or torch.channels_last, got "
                         f"{memory_format!r}")
    if maps.dim() != 4:
        raise ValueError(f"nfp_compress_map: memory_format=torch.channels_last needs [B,N,H,W] maps, got {tuple(maps.shape)}")
    return True


def cproj_forward_call(maps, w, gamma, beta, rm, rv, use_batch_stats, momentum, eps, relu, channels_last=False):
    """(out [B,D,...] in the maps' dtype, saved) from nfp_cproj_forward_fmt on dense CUDA maps [B,N,...] and float32 w
    [D,N], gamma, beta [D] — cpool_forward_call's arguments and `saved`, plus `relu`; channels_last: `out` [B,D,H,W] is
    written channels-last (the maps stay NCHW)."""
    return _cp_forward_call("proj", maps, w, gamma, beta, rm, rv, use_batch_stats, momentum, eps, relu, channels_last)


def cproj_backward_call(maps, w, gamma, beta, rm, rv, saved, use_batch_stats, eps, relu, grad_out, want):
    """(grad_maps in the maps' dtype, grad_w [D,N], grad_gamma [D], grad_beta [D]) from nfp_cproj_backward_fmt, grad_out
    [B,D,...] in the maps' dtype — None for each gradient `want` (four flags) leaves out: a NULL pointer in the library,
    neither computed nor written.  The layout grad_out arrives in selects the kernels, whatever the forward wrote: NCHW-dense
    (also where H = W = 1 or D = 1 make it both) the NCHW ones, channels-last-dense the channels-last ones, neither a
    copy; anything else is made NCHW-dense first."""
    return _cp_backward_call("proj", maps, w, gamma, beta, rm, rv, saved, use_batch_stats, eps, grad_out, want, relu)


class _CProjHip(_CpHip):
    """out [B,D,...] in the maps' dtype, which the caller may modify in place (ReLU(inplace=True) behind it,
    `out += identity`): the backward recomputes the pre-activation from the maps.  channels_last: the layout `out` is
    written in; the backward goes by its grad_out's."""

    @staticmethod
    def forward(ctx, maps, w, gamma, beta, stats, use_batch_stats, momentum, eps, relu, need_grad, channels_last=False):
        out, saved = cproj_forward_call(maps, w, gamma, beta, stats[0], stats[1], use_batch_stats, momentum, eps, relu,
                                        channels_last)
        if need_grad:
            _CpHip._save(ctx, maps, w, gamma, beta, saved, stats, use_batch_stats, eps)
            ctx.relu = relu
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        grads = cproj_backward_call(*_CpHip._state(ctx), ctx.relu, grad_out, ctx.needs_input_grad[:4])
        return (*grads, None, None, None, None, None, None, None)


def cproj_hip_serves(maps, weight, gamma, beta, momentum, use_batch_stats=True, need_grad=True, channels_last=False):
    """The cproj kernels can serve dense CUDA float32 / bfloat16 maps [B >= 1, N <= 32, ...] with N * P and D * P below 2^31
    per image and D <= 2^22, under an affine BatchNorm with a float momentum, outside torch.compile and torch.autocast.  Of
    those they take, by default, what measured faster than the composition (CPROJ_ROUTED_MAPS and
    CPROJ_ROUTED_TRAIN_PIXELS above): at most 8 maps, and either a forward on running statistics that no
    backward follows, or batch statistics over B * P >= 64 * 54 * 54 map pixels; a backward on running statistics was not
    measured.  A channels_last result is routed by its own measurement (CPROJ_ROUTED_NHWC_* above): that forward with at
    most 24 maps, or batch statistics with at most 8 maps over B * P >= 256 * 12 * 12 map pixels.
    NFP_CPROJ_TORCH (read at call time) is the A/B switch for both layouts: "1" the torch composition everywhere, "0" the
    HIP kernels wherever they can serve."""
    env = os.environ.get("NFP_CPROJ_TORCH")
    if env == "1" or not _cp_can_serve(maps, gamma, beta, momentum):
        return False
    B, N = maps.shape[:2]
    P = maps.numel() // (B * N)
    if N * P >= 2 ** 31 or weight.shape[0] * P >= 2 ** 31 or weight.shape[0] > 2 ** 22:
        return False
    if env == "0":
        return True
    if channels_last:
        if not use_batch_stats:
            return N <= CPROJ_ROUTED_NHWC_EVAL_MAPS and not need_grad
        return N <= CPROJ_ROUTED_MAPS and B * P >= CPROJ_ROUTED_NHWC_TRAIN_PIXELS
    if N > CPROJ_ROUTED_MAPS:
        return False
    return B * P >= CPROJ_ROUTED_TRAIN_PIXELS if use_batch_stats else not need_grad


def nfp_compress_map_tensors(maps, weight, gamma, beta, running_mean, running_var, use_batch_stats, momentum=0.1, eps=1e-5,
                             relu=True, *, memory_format=torch.contiguous_format, process_group=None):
    """`nfp_compress_map` on loose tensors: maps [B,N,H,W] (or [B,N,P]) -> [B,D,H,W] ([B,D,P]) =
    [relu](batch_norm(conv1x1(maps))), the arguments those of nfp_compress_pool_tensors plus `relu`.  Where
    `cproj_hip_serves`, three HIP launches forward and at most three backward: the [B,D,H,W] result is stored once, and the
    backward reads grad_out twice and nothing else of that size — autograd keeps the maps, the parameters and O(N*N + D)
    statistics, so the result may be modified in place (include/nfp.h: nfp_cproj_*; float32 arithmetic, the result rounded
    once to the maps' dtype).  Everything else — by default also what measured slower, see cproj_hip_serves — is
    `_host.compress_map_host`.
    memory_format: torch.contiguous_format (the default) or torch.channels_last — the same [B,D,H,W] values, dense
    channels-last, for a network that runs in that format: the kernels store them so and read a channels-last grad_out as
    it comes, without a converting copy either way; the composition's result is converted.  It needs [B,N,H,W] maps, which
    themselves stay NCHW; ValueError otherwise, and for any other value.
    process_group: as in nfp_compress_pool_tensors."""
    channels_last = _cproj_memory_format(memory_format, maps)
    _cp_check_args("nfp_compress_map", maps, weight, use_batch_stats, running_mean, running_var)
    if _cp_sync_applies(process_group, use_batch_stats):
        return _cp_sync_tensors_call("proj", maps, weight, gamma, beta, running_mean, running_var, momentum, eps, process_group,
                                     relu, channels_last)
    need_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (maps, weight, gamma, beta))
    prepared = (cproj_hip_serves(maps, weight, gamma, beta, momentum, bool(use_batch_stats), need_grad, channels_last)
                and _cp_prepare(maps, weight, gamma, beta, running_mean, running_var, use_batch_stats))
    if not prepared:
        y = compress_map_host(maps, weight, gamma, beta, running_mean, running_var, use_batch_stats, momentum, eps, relu)
        return _cp_in_format(y, channels_last)
    return _CProjHip.apply(maps, *prepared, (running_mean, running_var), bool(use_batch_stats), float(momentum), float(eps),
                           bool(relu), need_grad, channels_last)


def nfp_compress_map(maps, weight, bn, relu=True, training=None, *, memory_format=torch.contiguous_format):
    """The projection behind the NFP maps where the network carries on from the projected map: NFPInsert's nfp_proj
    (models/mobilenetv3.py:346-350) and, with relu=False, NFPBottleneck's bn2(conv2(.)) (models/nfp_heads.py:270-272).
    maps [B,N,H,W] -> [B,D,H,W] = [relu](bn(conv1x1(maps))), `weight` the 1x1 conv's ([D,N,1,1], no bias) and `bn` its
    nn.BatchNorm2d — whose mode (`training`: None = bn.training), running statistics and num_batches_tracked are used and
    updated exactly as bn.forward does.  memory_format: torch.contiguous_format or torch.channels_last, the layout of the
    result.  An nn.SyncBatchNorm synchronises as in nfp_compress_pool.  See nfp_compress_map_tensors."""
    channels_last = _cproj_memory_format(memory_format, maps)       # (refused before the step counter moves)
    training = bn.training if training is None else bool(training)
    group = cp_sync_group(bn, training)
    if group is not None:
        return _cp_sync_module_call("proj", maps, weight, bn, training, group, relu, channels_last)
    use_batch_stats, rm, rv, factor = _bn_call_mode(bn, training)
    if factor is not None:
        y = compress_map_host(maps, weight, bn.weight, bn.bias, rm, rv, use_batch_stats, factor, bn.eps, relu)
        return _cp_in_format(y, channels_last)
    return nfp_compress_map_tensors(maps, weight, bn.weight, bn.bias, rm, rv, use_batch_stats, float(bn.momentum), bn.eps, relu,
                                    memory_format=memory_format)


# ---- SyncBatchNorm in the two tails — include/nfp.h: nfp_cpsync_*  ----
# The batch statistics of the tail come from the mean and covariance of the N maps, so a rank hands the others 1 + N + N*N
# float64 numbers forward (its count, mean and scatter) and N + N*N float32 backward (its share of k and Q) — and gets every
# rank's back, joined in rank order by the same kernel from the same bits on all of them.
def cp_sync_group(bn, training=None):
    """The process group over whose ranks one call of `bn` in mode `training` (None: bn.training) takes its batch
    statistics, or None where the call is rank-local — the rule of nn.SyncBatchNorm.forward: an nn.SyncBatchNorm, in
    training mode, torch.distributed available and initialised, and more than one rank in bn.process_group (None: WORLD)."""
    if not isinstance(bn, torch.nn.SyncBatchNorm):
        return None
    dist = torch.distributed
    if not (bn.training if training is None else training) or not dist.is_available() or not dist.is_initialized():
        return None
    group = bn.process_group if bn.process_group is not None else dist.group.WORLD
    return group if dist.get_world_size(group) > 1 else None


def _cp_sync_applies(process_group, use_batch_stats):
    """cp_sync_group's rule for the loose-tensor forms, which are handed the group."""
    return bool(process_group is not None and use_batch_stats and torch.distributed.get_world_size(process_group) > 1)


def cp_sync_serves(kind, maps, gamma, beta, momentum):
    """The staged kernels (nfp_cpsync_*) take a call of `kind` ("pool" or "proj") whose statistics span a process group.
    Every rank of the group must answer alike — ranks that disagree would enter different collectives and hang — so the
    answer reads only what the ranks share: the device type, dtype and number of maps, affine parameters and a float
    momentum, torch.compile / torch.autocast, and NFP_CPOOL_TORCH / NFP_CPROJ_TORCH ("1": the composition; "0": the
    kernels up to 32 maps; unset: up to 8).  It never reads the local batch or map size: an empty rank, a rank with one
    pixel and a rank with thousands take the same route, and the pixel-count thresholds of cproj_hip_serves do not apply.
    For "proj" that default is a decision — the form that exchanges 73 + 72 numbers at 8 maps where SyncBatchNorm exchanges
    2 D + 1 and 2 D — not a measurement: no run over more than one GPU has been made."""
    env = os.environ.get("NFP_CPROJ_TORCH" if kind == "proj" else "NFP_CPOOL_TORCH")
    if env == "1" or torch.compiler.is_compiling() or not maps.is_cuda or torch.is_autocast_enabled("cuda"):
        return False
    if maps.dtype not in _DTYPES or gamma is None or beta is None or not isinstance(momentum, float):
        return False
    return 1 <= maps.shape[1] <= (CPOOL_MAX_MAPS if env == "0" else CPOOL_ROUTED_MAPS)


def _cps_head(kind, maps, w, gamma, beta, relu):
    """The leading arguments of nfp_cpsync_forward / _reduce / _maps."""
    return [_abi.CP_PROJ if kind == "proj" else _abi.CP_POOL, *_cp_sizes(maps, w.shape[0], True), _DTYPES[maps.dtype],
            int(bool(relu)), _ptr(maps), w.data_ptr(), gamma.data_ptr(), beta.data_ptr()]


def cp_sync_moments_call(maps):
    """A rank's record from nfp_cpsync_moments: float64 [1 + N + N*N] — count, mean and scatter of its dense CUDA maps
    [B,N,...], B = 0 included."""
    L = _abi.load()
    B, N, P, _ = sizes = _cp_sizes(maps, 1, True)
    with _on_device(maps.device):
        nr = int(L.nfp_cpsync_record_doubles(N))
        record = torch.empty(nr, dtype=torch.float64, device=maps.device)
        scratch, ns = _cp_scratch("pool", sizes, False, B, maps.device)
        _abi.check(L.nfp_cpsync_moments(B, N, P, _DTYPES[maps.dtype], _ptr(maps), record.data_ptr(), nr, _ptr(scratch), ns,
                                        _raw_stream(maps.device)))
    return record


def cp_sync_forward_call(kind, maps, w, gamma, beta, rm, rv, momentum, eps, records, relu=True, channels_last=False,
                         global_count=0):
    """(out, saved) from nfp_cpsync_forward: the rank's rows of the result — [B,D] float32 for "pool", [B,D,...] in the
    maps' dtype for "proj" — under the statistics joined from `records` [world, 1 + N + N*N] (float64, row r rank r's),
    and the state the backward reads.  rm / rv: the running statistics (float32 [D], or both None), updated in place."""
    L = _abi.load()
    dev = maps.device
    with _on_device(dev):
        out = _cp_out(kind, maps, w.shape[0], channels_last)
        ns = int(L.nfp_cpsync_saved_floats(maps.shape[1], w.shape[0]))
        saved = torch.empty(ns, dtype=torch.float32, device=dev)
        records = records.contiguous()
        _abi.check(L.nfp_cpsync_forward(*_cps_head(kind, maps, w, gamma, beta, relu), _ptr(rm), _ptr(rv), float(momentum),
                                        float(eps), records.data_ptr(), records.shape[0], records.numel(), int(global_count),
                                        _ptr(out), saved.data_ptr(), ns, _raw_stream(dev),
                                        _abi.ACT_NHWC if channels_last else _abi.ACT_NCHW))
    return out, saved


def cp_sync_reduce_call(kind, maps, w, gamma, beta, saved, eps, grad_out, want=(True, True, True), relu=True):
    """(grad_w [D,N], grad_gamma [D], grad_beta [D], row) from nfp_cpsync_reduce: the rank's parameter gradients — None for
    each `want` leaves out; their sum over the ranks is the batch's — and its row [N + N*N] of k and Q."""
    L = _abi.load()
    sizes = _cp_sizes(maps, w.shape[0], True)
    dev = maps.device
    go, nhwc = _cp_grad_out(kind, maps, grad_out)
    with _on_device(dev):
        grads = _cp_grads(maps, w.shape[0], (False, *want))[1:]
        nk = int(L.nfp_cpsync_kq_floats(maps.shape[1]))
        row = torch.empty(nk, dtype=torch.float32, device=dev)
        scratch, ns = _cp_scratch(kind, sizes, True, sizes[0], dev)
        _abi.check(L.nfp_cpsync_reduce(*_cps_head(kind, maps, w, gamma, beta, relu), float(eps), saved.data_ptr(), saved.numel(),
                                       _ptr(go), *map(_ptr, grads), row.data_ptr(), nk, _ptr(scratch), ns, _raw_stream(dev),
                                       _abi.ACT_NHWC if nhwc else _abi.ACT_NCHW))
    return (*grads, row)


def cp_sync_maps_call(kind, maps, w, gamma, beta, saved, eps, grad_out, rows, relu=True):
    """grad_maps of the rank, in the maps' dtype, from nfp_cpsync_maps under `rows` [world, N + N*N] (row r rank r's)."""
    L = _abi.load()
    dev = maps.device
    go, nhwc = _cp_grad_out(kind, maps, grad_out)
    with _on_device(dev):
        gm = torch.empty_like(maps)
        rows = rows.contiguous()
        _abi.check(L.nfp_cpsync_maps(*_cps_head(kind, maps, w, gamma, beta, relu), float(eps), saved.data_ptr(), saved.numel(),
                                     _ptr(go), rows.data_ptr(), rows.shape[0], rows.numel(), _ptr(gm), _raw_stream(dev),
                                     _abi.ACT_NHWC if nhwc else _abi.ACT_NCHW))
    return gm


def _cps_gather(row, group):
    """[world, len(row)]: every rank's `row`, row r rank r's — one all-reduce (SUM) of a zeroed buffer in which a rank fills
    its own row.  Exact, since every other addend of an element is 0; the same bits on every rank; served by NCCL / RCCL and
    by gloo for CUDA tensors.  Blocking, on the row's device and current stream."""
    dist = torch.distributed
    with _on_device(row.device):
        buf = torch.zeros(dist.get_world_size(group), row.numel(), dtype=row.dtype, device=row.device)
        buf[dist.get_rank(group)].copy_(row)
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    return buf


class _CpSyncHip(_CpHip):
    """_CPoolHip / _CProjHip in training mode with the statistics of every rank of `group`: moments -> gather -> finish and
    the main forward; part and reduce -> gather -> grad_maps.  Both gathers are entered by every rank, whatever its batch
    and whichever gradients it needs.  Saved: the maps, the parameters and the O(N*N + D) statistics."""

    @staticmethod
    def forward(ctx, maps, w, gamma, beta, stats, momentum, eps, relu, need_grad, kind, channels_last, group):
        records = _cps_gather(cp_sync_moments_call(maps), group)
        out, saved = cp_sync_forward_call(kind, maps, w, gamma, beta, stats[0], stats[1], momentum, eps, records, relu,
                                          channels_last)
        if need_grad:
            _CpHip._save(ctx, maps, w, gamma, beta, saved, stats, True, eps)
            ctx.relu, ctx.kind, ctx.group = relu, kind, group
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        maps, w, gamma, beta, _, _, saved, _, eps = _CpHip._state(ctx)
        gw, gg, gb, row = cp_sync_reduce_call(ctx.kind, maps, w, gamma, beta, saved, eps, grad_out, ctx.needs_input_grad[1:4],
                                              ctx.relu)
        rows = _cps_gather(row, ctx.group)
        gm = None
        if ctx.needs_input_grad[0]:
            gm = cp_sync_maps_call(ctx.kind, maps, w, gamma, beta, saved, eps, grad_out, rows, ctx.relu)
        return (gm, gw, gg, gb, None, None, None, None, None, None, None, None)


def _cp_sync_node_call(kind, maps, weight, gamma, beta, rm, rv, momentum, eps, group, relu, channels_last):
    """The sync node on what cp_sync_serves took, or None where the running statistics are not float32 and contiguous."""
    prepared = _cp_prepare(maps, weight, gamma, beta, rm, rv, False)
    if prepared is None:
        return None
    need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (maps, weight, gamma, beta))
    out = _CpSyncHip.apply(maps.contiguous(), *prepared, (rm, rv), float(momentum), float(eps), bool(relu), need_grad, kind,
                           channels_last, group)
    return out if out.dtype == maps.dtype else out.to(maps.dtype)


def _cp_sync_finish_composition(kind, y, maps, relu, channels_last):
    return _cp_in_format(compress_finish(y, maps, relu, kind == "pool"), channels_last and kind != "pool")


def _cp_sync_module_call(kind, maps, weight, bn, training, group, relu=True, channels_last=False):
    """One call of the tail under `bn`, an nn.SyncBatchNorm that synchronises over `group` (cp_sync_group).  Where
    cp_sync_serves, the staged kernels; else the composition with bn.forward itself on the conv's output, in the call's
    mode: torch synchronises, and raises its own ValueError for CPU tensors."""
    if cp_sync_serves(kind, maps, bn.weight, bn.bias, bn.momentum) and maps.dim() >= 3 and maps.shape[1] == weight.shape[1]:
        rm, rv = (bn.running_mean, bn.running_var) if bn.track_running_stats else (None, None)
        out = _cp_sync_node_call(kind, maps, weight, bn.weight, bn.bias, rm, rv, bn.momentum, bn.eps, group, relu, channels_last)
        if out is not None:
            _bn_call_mode(bn, training)          # (num_batches_tracked, once per call)
            return out
    was = bn.training
    bn.training = training
    try:
        y = bn(compress_conv(maps, weight))
    finally:
        bn.training = was
    return _cp_sync_finish_composition(kind, y, maps, relu, channels_last)


def _cp_sync_tensors_call(kind, maps, weight, gamma, beta, rm, rv, momentum, eps, group, relu=True, channels_last=False):
    """The same on loose tensors (use_batch_stats, a group of more than one rank); the composition runs torch's own
    SyncBatchNorm function on the conv's output."""
    if cp_sync_serves(kind, maps, gamma, beta, momentum):
        out = _cp_sync_node_call(kind, maps, weight, gamma, beta, rm, rv, momentum, eps, group, relu, channels_last)
        if out is not None:
            return out
    if not maps.is_cuda:
        raise ValueError("SyncBatchNorm expected input tensor to be on GPU or privateuseone")
    from torch.nn.modules._functions import SyncBatchNorm as sync_batch_norm
    y = sync_batch_norm.apply(compress_conv(maps, weight), gamma, beta, rm, rv, eps, momentum, group,
                              torch.distributed.get_world_size(group))
    return _cp_sync_finish_composition(kind, y, maps, relu, channels_last)
