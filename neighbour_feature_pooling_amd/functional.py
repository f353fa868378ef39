"""Functional NFP: `nfp(x, cfg)` — the autograd op behind NFPPooling.forward.

CUDA tensors go through libnfp_hip.so (include/nfp.h) — one fused forward kernel,
one fused backward kernel, saved state = the output map plus one float per input
pixel.  Nothing else can serve a CUDA tensor: if the library is missing or refuses
the configuration the call raises.  CPU tensors use `_host.nfp_host` (see there).
"""
import ctypes
import dataclasses
import os
import warnings
from collections import OrderedDict
from dataclasses import dataclass

import torch

from . import _abi
from ._host import attention_pool_host, deepten_host, nfp_host


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


def _cpp_entry(name, x=None):
    """The C++ node `name` of _nfp_torch.so, or None where the Python node serves: no module or NFP_PY_NODES=1
    (`_cpp_nodes`), an older module without that entry and, with `x` given, an empty batch."""
    if x is not None and x.shape[0] == 0:
        return None
    return getattr(_cpp_nodes() or None, name, None)


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


def _plan(x, layout, cfg, tables=True):
    """The _Plan of this input signature — cached (LRU): in eager mode the host side of a call (a few ctypes round trips)
    otherwise costs more than the two kernels.  tables=False: the plan of the families whose kernels keep no tables (the
    biased and the valid-map ones) — the descriptor and its output shape alone, no workspace (`desc.ws` stays NULL), no
    dry run, an entry of its own in the one cache; what the library says about it is `ask`ed (nfp_bias_saved_floats,
    nfp_valid_supported, nfp_valid_abs_supported, ...)."""
    key = (tuple(x.shape), x.stride(0), layout, x.dtype, cfg, x.device.index)
    if not tables:
        key = ("no tables",) + key
        plan = _plans_get(key)
        if plan is None:
            plan = _Plan(make_desc(x, cfg, layout), layout)
            _plans_put(key, plan)
        return plan
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


def _need_grad(*tensors):
    """Will a backward follow?  Grad mode is on and one of the tensors (None: an absent one) requires a gradient — sampled
    by the caller of a node: grad mode is always off inside an autograd.Function, and ctx.needs_input_grad ignores
    torch.no_grad()."""
    if not torch.is_grad_enabled():
        return False
    for t in tensors:
        if t is not None and t.requires_grad:
            return True
    return False


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


# ---- the "x -> maps" families: one launch sequence each way, one autograd node, one choice of the node's flavour ---------
@dataclass(frozen=True)
class _MapsFamily:
    """A family of ABI entries that turn x into its maps and grad_out into grad_x: the names, and the facts in which
    their calls differ.  A new family of this shape is one more record (and one more `MapsNode<...>` in nfp_torch.cpp)."""
    forward: str
    backward: str
    apply: str              # the C++ node's entry in _nfp_torch.so
    tables: bool            # its plans carry the workspace tables and their own count of saved floats (`_saved_len`)
    saved_with_len: bool    # `saved` travels with its length
    reads_maps: bool        # the backward reads out + saved; False: x and grad_out alone — there is no `saved`, and the node
                            # saves x alone, so the maps it returned may be modified in place
    supported: str = ""     # a table-less family's queries of its plan: does it serve the descriptor ...
    saved_floats: str = ""  # ... and with how many floats of saved state ("": none)


NFP = _MapsFamily("nfp_forward", "nfp_backward", "nfp_apply", True, False, True)
VALID = _MapsFamily("nfp_valid_forward", "nfp_valid_backward", "nfp_valid_apply", False, True, True,
                    "nfp_valid_supported", "nfp_valid_saved_floats")
VALID_ABS = _MapsFamily("nfp_valid_abs_forward", "nfp_valid_abs_backward", "nfp_valid_abs_apply", False, False, False,
                        "nfp_valid_abs_supported")
STRIDED = _MapsFamily("nfp_strided_forward", "nfp_strided_backward", "nfp_strided_apply", False, True, True,
                      "nfp_strided_supported", "nfp_strided_saved_floats")


def maps_saved_len(fam, plan, cfg, dtype, need_grad):
    """Floats of saved state the family's forward gets for this call (NFP: or the refusal of a call whose backward is not
    served); the valid-map kernels keep |x| per pixel only with a backward to follow, their L1 family nothing."""
    if fam.tables:
        return _saved_len(plan, cfg, dtype, need_grad)
    return max(plan.ask(fam.saved_floats), 0) if need_grad and fam.saved_floats else 0


def maps_forward_call(fam, x, plan, ns):
    """(out, saved or None) from the family's forward on (x, plan) as `_planned` / `_valid_route` gave them; ns floats of
    saved state (`maps_saved_len`, or the compiled graph's bound)."""
    args = [ctypes.byref(plan.desc), x.data_ptr()]
    with _on_device(x.device):
        out = torch.empty(plan.oshape, dtype=torch.float32 if plan.desc.map_f32 else x.dtype, device=x.device)
        args.append(out.data_ptr())
        saved = None
        if fam.reads_maps:
            saved = torch.empty(ns, dtype=torch.float32, device=x.device)
            args.append(saved.data_ptr() if ns > 0 else None)
            if fam.saved_with_len:
                args.append(ns)
        _abi.check(getattr(_abi.load(), fam.forward)(*args, _raw_stream(x.device)))
    return out, saved


def maps_backward_call(fam, x, plan, out, saved, grad_out):
    """grad_x from the family's backward — dense, in x's inner layout; (out, saved) as the forward call gave them (not read
    where the family's backward does not)."""
    go = _grad_out_as(grad_out, out.dtype if fam.reads_maps else x.dtype)   # (the maps' type: x's, or float32 for map_f32)
    args = [ctypes.byref(plan.desc), x.data_ptr(), go.data_ptr()]
    if fam.reads_maps:
        args += (out.data_ptr(), saved.data_ptr() if saved.numel() else None)
        if fam.saved_with_len:
            args.append(saved.numel())
    with _on_device(x.device):
        gx = _empty_grad_x(x, plan.nhwc)
        _abi.check(getattr(_abi.load(), fam.backward)(*args, gx.data_ptr(), _raw_stream(x.device)))
    return gx


class _MapsHip(torch.autograd.Function):
    """The Python node of the four families: one forward launch, one backward launch.  It holds its forward's plan and
    saves what its backward reads — nothing without a gradient to follow."""

    @staticmethod
    def forward(ctx, x, fam, plan, ns, need_grad):
        out, saved = maps_forward_call(fam, x, plan, ns)
        if need_grad:
            ctx.fam, ctx.plan = fam, plan
            ctx.save_for_backward(*((x, out, saved) if fam.reads_maps else (x,)))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, out, saved = ctx.saved_tensors if ctx.fam.reads_maps else (*ctx.saved_tensors, None, None)
        return maps_backward_call(ctx.fam, x, ctx.plan, out, saved, grad_out), None, None, None, None


def _maps_node(fam, x, plan, cfg, need_grad):
    """The maps of (x, plan) from the family's autograd node — the C++ one where `_cpp_entry` has it (the valid families: for
    a batch that is not empty), else `_MapsHip`."""
    ns = maps_saved_len(fam, plan, cfg, x.dtype, need_grad)
    apply = _cpp_entry(fam.apply, None if fam.tables else x)
    if apply is None:
        return _MapsHip.apply(x, fam, plan, ns, need_grad)
    if fam.reads_maps:
        return _cpp_call(apply, x, plan.desc_tensor, list(plan.oshape), ns, plan.nhwc)
    return _cpp_call(apply, x, plan.desc_tensor, list(plan.oshape), plan.nhwc, need_grad)


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
            warnings.warn("NFP: float64 feature maps are computed in float32 by the HIP kernels and returned as float64",
                          RuntimeWarning, stacklevel=5)     # (_upcast, the public op, the module's forward, its caller)
            _WARNED_F64 = True
        return x.float(), torch.float64
    return x, None


def _upcast(op, x, *args, keep=()):
    """None where `op` runs on x as it is.  Otherwise — `_amp_input`: torch.autocast, float16, float64 — the results of
    op(x as float32, *args) outside autocast, each cast back to the type `_amp_input` names (if it names one) except a None
    and the positions in `keep`."""
    xin, cast = _amp_input(x)
    if xin is x:
        return None
    with torch.autocast("cuda", enabled=False):
        res = op(xin, *args)
    if cast is None:
        return res
    if isinstance(res, tuple):
        return tuple(r if r is None or i in keep else r.to(cast) for i, r in enumerate(res))
    return res.to(cast)


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
    up = _upcast(nfp_pool, x, cfg, want_gap)
    if up is not None:
        return up
    if x.is_cuda and torch.compiler.is_compiling() and x.dim() == 4:
        # under torch.compile: the registered custom op (one node in the compiled graph, no graph break) — _ops.py
        from . import _ops
        gap, nfpm, _, _ = torch.ops.nfp_amd.nfp_pool(x, *_ops.cfg_args(cfg), bool(want_gap), _need_grad(x))
        return (gap if want_gap else None), nfpm
    if x.dim() == 4 and nfp_pool_fused_ok(x, cfg):
        need_grad = _need_grad(x)
        try:
            apply = _cpp_entry("nfp_pool_apply")
            if apply is not None:
                xd, plan = _planned(x, cfg)
                gap, nfpm = _cpp_call(apply, xd, plan.desc_tensor, list(plan.oshape),
                                      max(plan.ask("nfp_pool_saved_floats"), 0), plan.nhwc, bool(want_gap), need_grad)
            else:
                gap, nfpm = _NfpPoolHip.apply(x, cfg, bool(want_gap), need_grad)
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
    up = _upcast(nfp_multi_radius, x, cfg1, cfg2)   # (autocast / float16: also where the two layers run one by one)
    if up is not None:
        return up
    cfg = multi_radius_config(cfg1, cfg2) if x.is_cuda and x.dim() == 4 else None
    if cfg is not None:
        try:
            return nfp(x, cfg)
        except _abi.NfpUnsupported:
            pass
    return torch.cat([nfp(x, cfg1), nfp(x, cfg2)], dim=1)


def _warn_scs():
    warnings.warn("NFP measure 'scs' (SharpenedCosine) mixes batch elements in the reference; it runs as "
                  "PyTorch ops on the GPU, not through the HIP kernels", RuntimeWarning, stacklevel=4)


def nfp(x, cfg):
    """[B,C,H,W] -> [B, k*k-1, H', W'] neighbour-similarity maps (NFPPooling.forward, nfp.py:132-134)."""
    if x.dim() != 4:
        raise RuntimeError(f"NFP expects a 4-D [B,C,H,W] feature map, got {tuple(x.shape)}")
    native = _autocast_native(x, cfg)
    if native is not None:
        xd, plan, mcfg = native
        with torch.autocast("cuda", enabled=False):
            return _maps_node(NFP, xd, plan, mcfg, _need_grad(x))
    up = _upcast(nfp, x, cfg)
    if up is not None:
        return up
    if x.is_cuda and torch.compiler.is_compiling() and cfg.measure != "scs":
        # under torch.compile: the registered custom op (one node in the compiled graph, no graph break) — _ops.py
        from . import _ops
        return torch.ops.nfp_amd.nfp(x, *_ops.cfg_args(cfg), _need_grad(x))[0]
    if x.is_cuda and cfg.measure == "scs":
        # The one measure without a kernel, on purpose: the reference's SharpenedCosine divides
        # (B,N,H,W) by (B,1,N,H,W) and so averages over the BATCH (nfp.py:359-374).  Its exact behaviour
        # is reproduced with torch ops on the tensor's own device, and said out loud; every other
        # measure on a CUDA tensor is served by libnfp_hip.so or raises.
        _warn_scs()
        return nfp_host(x, cfg)
    if x.is_cuda:
        xd, plan = _planned(x, cfg)
        return _maps_node(NFP, xd, plan, cfg, _need_grad(x))
    if cfg.inner_R:
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
    up = _upcast(nfp_with_gap, x, cfg, keep=(0,))    # (gap stays float32)
    if up is not None:
        return up
    if x.is_cuda and torch.compiler.is_compiling():
        # under torch.compile: servability is decided NOW, on the static shape (a host-only dry run); a call the fused
        # kernels refuse is traced as the composition, so nothing can raise inside the compiled graph that eager serves
        from . import _ops
        if _gap_servable_traced(tuple(x.shape), tuple(x.stride()), x.dtype, _ops.cfg_args(cfg)):
            gap, maps, _ = torch.ops.nfp_amd.nfp_gap(x, *_ops.cfg_args(cfg))
            return gap, maps
    elif x.is_cuda and nfp_gap_fused_ok(x, cfg):
        try:
            if _need_grad(x):
                apply = _cpp_entry("nfp_gap_apply")
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


def _bias_f32(t):
    return t.detach().float().contiguous()


def bias_forward_call(x, centre_bias, neighbour_bias, cfg):
    """(out, saved) from nfp_bias_forward; saved is torch-allocated (graph capture safe)."""
    L = _abi.load()
    xd, layout = _dense(x)
    plan = _plan(xd, layout, cfg, tables=False)     # (the biased kernels keep no tables)
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
    plan = _plan(xd, layout, cfg, tables=False)     # (the biased kernels keep no tables)
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
    up = _upcast(nfp_biased, x, cfg, centre_bias, neighbour_bias)
    if up is not None:
        return up
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
    need_grad = _need_grad(maps, weight, bias)
    pooled = _AttPoolHip.apply(maps, weight.reshape(-1).float().contiguous(), bias.reshape(-1).float(), need_grad)
    return pooled if pooled.dtype == maps.dtype else pooled.to(maps.dtype)


# ---- the Deep-TEN encoding layer — include/nfp.h: nfp_deepten_* (csrc/nfp_deepten.hip) -------------------------------------
DEEPTEN_MAX_CODES = 64      # K the kernels serve (csrc/nfp_deepten.hip: kDtMaxK)


def _deepten_geometry(x, codewords):
    """(B, N, K, D, layout id, batch stride) of a [B,D,H,W] x whose images are dense in NCHW or channels-last order."""
    B, D, H, W = x.shape
    layout = _in_place_layout(x.shape, x.stride())
    return (B, H * W, codewords.shape[0], D, _abi.ACT_NHWC if layout == "nhwc" else _abi.ACT_NCHW,
            x.stride(0) if B > 1 else D * H * W)


def deepten_forward_call(x, codewords, scale):
    """(out [B,K*D] in x's dtype, saved: A and dist, 2*B*N*K float32) from nfp_deepten_forward on a CUDA x [B,D,H,W] of
    dense images and float32 codewords [K,D], scale [K].  `saved` hands A from the first launch to the second, so it is
    made also when no backward follows."""
    L = _abi.load()
    B, N, K, D, layout, sxB = _deepten_geometry(x, codewords)
    with _on_device(x.device):
        out = torch.empty(B, K * D, dtype=x.dtype, device=x.device)
        ns = int(L.nfp_deepten_saved_floats(B, N, K))
        saved = torch.empty(ns, dtype=torch.float32, device=x.device)
        _abi.check(L.nfp_deepten_forward(B, N, K, D, _DTYPES[x.dtype], layout, sxB, x.data_ptr(), codewords.data_ptr(),
                                         scale.data_ptr(), out.data_ptr(), saved.data_ptr(), ns, _raw_stream(x.device)))
    return out, saved


def deepten_backward_call(x, codewords, scale, saved, grad_out, want_x, want_c, want_s):
    """(grad_x dense in x's layout and dtype, grad_codewords [K,D], grad_scale [K]) from nfp_deepten_backward — None for
    each gradient nobody wants (a NULL pointer in the library: neither computed nor written)."""
    L = _abi.load()
    B, N, K, D, layout, sxB = _deepten_geometry(x, codewords)
    go = grad_out.contiguous().float()
    with _on_device(x.device):
        gx = None
        if want_x:
            fmt = torch.channels_last if layout == _abi.ACT_NHWC else torch.contiguous_format
            gx = torch.empty(x.shape, dtype=x.dtype, device=x.device, memory_format=fmt)
        gc = torch.empty(K, D, dtype=torch.float32, device=x.device) if want_c else None
        gs = torch.empty(K, dtype=torch.float32, device=x.device) if want_s else None
        ns = int(L.nfp_deepten_scratch_floats(B, N, K, D, int(want_c or want_s)))
        scratch = torch.empty(ns, dtype=torch.float32, device=x.device)
        _abi.check(L.nfp_deepten_backward(B, N, K, D, _DTYPES[x.dtype], layout, sxB, x.data_ptr(), codewords.data_ptr(),
                                          scale.data_ptr(), saved.data_ptr(), saved.numel(), go.data_ptr(),
                                          gx.data_ptr() if want_x else None, gc.data_ptr() if want_c else None,
                                          gs.data_ptr() if want_s else None, scratch.data_ptr(), ns, _raw_stream(x.device)))
    return gx, gc, gs


class _DeepTenHip(torch.autograd.Function):
    """out [B,K*D] of a CUDA x [B,D,H,W] of dense images and float32 (codewords [K,D], scale [K]): two kernels forward, two
    to three backward.  need_grad: some input requires a gradient and grad mode is on, sampled by the caller."""

    @staticmethod
    def forward(ctx, x, codewords, scale, need_grad):
        out, saved = deepten_forward_call(x, codewords, scale)
        if need_grad:
            ctx.save_for_backward(x, codewords, scale, saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, codewords, scale, saved = ctx.saved_tensors
        want = ctx.needs_input_grad
        gx, gc, gs = deepten_backward_call(x, codewords, scale, saved, grad_out, want[0], want[1], want[2])
        return gx, gc, gs, None


def _deepten_hip_serves(x, codewords):
    """The kernels serve CUDA float32 / bfloat16 x of a non-empty batch whose images are dense in NCHW or channels-last
    order (any batch stride that keeps them apart) and up to 64 codewords, outside torch.compile (where the layer is traced
    as ATen ops), unless NFP_DEEPTEN_TORCH=1 (read at call time) asks for the torch formulation."""
    return (not torch.compiler.is_compiling() and x.is_cuda and x.dtype in _DTYPES and x.shape[0] > 0 and x.numel() > 0
            and codewords.shape[0] <= DEEPTEN_MAX_CODES and os.environ.get("NFP_DEEPTEN_TORCH") != "1"
            and _in_place_layout(x.shape, x.stride()) is not None)


def nfp_deepten_encode(x, codewords, scale):
    """The Deep-TEN encoding layer (models/deepten.py::DeepTENEncoding.forward): x [B,D,H,W], codewords [K,D], scale [K] ->
    [B, K*D], the residuals x - c summed over the pixels under softmax_k(-scale_k |x - c_k|^2).
    CUDA float32 / bfloat16 x in a served layout runs the HIP kernels (include/nfp.h: nfp_deepten_*; float32 arithmetic, the
    result and grad_x rounded once to x's dtype; a gradient for x, the codewords and the scale, each only where wanted),
    which never form the [B,N,K,D] residual tensor.  Everything else — CPU, float16, float64, other strides, K > 64,
    torch.compile, torch.autocast, NFP_DEEPTEN_TORCH=1 — runs the torch formulation `_host.deepten_host`."""
    if x.dim() != 4:
        raise RuntimeError(f"nfp_deepten_encode expects a 4-D [B,D,H,W] feature map, got {tuple(x.shape)}")
    if codewords.dim() != 2 or codewords.shape[1] != x.shape[1] or scale.shape != codewords.shape[:1]:
        raise RuntimeError(f"nfp_deepten_encode: x of {x.shape[1]} channels needs codewords [K,{x.shape[1]}] and scale [K], "
                           f"got {tuple(codewords.shape)} and {tuple(scale.shape)}")
    if (x.is_cuda and torch.is_autocast_enabled("cuda")) or not _deepten_hip_serves(x, codewords):
        return deepten_host(x, codewords, scale)
    need_grad = _need_grad(x, codewords, scale)
    return _DeepTenHip.apply(x, codewords.float().contiguous(), scale.float().contiguous(), need_grad)


# ---- valid maps: stride 1, dilation 1, padding 0 — include/nfp.h: nfp_valid_*, nfp_valid_abs_* (csrc/nfp_valid.hip) ---------
def _valid_route(x, cfg, fam, off="NFP_VALID_OFF"):
    """The table-less plan on which the family's kernels (VALID: fwd_valid / bwd_valid; VALID_ABS: their l1 forms; STRIDED:
    fwd_strided / bwd_strided) read this call in place, or None where `nfp` serves it: `off`=1 in the environment (read at
    call time), torch.compile, a CPU tensor, another dtype, images that are not dense, or a descriptor the family's
    `supported` query refuses (another measure, rows above 128 pixels, channels-last maps off the alignment rule).  The
    families ask the one plan of the signature."""
    if (torch.compiler.is_compiling() or not (x.is_cuda and x.dtype in _DTYPES) or cfg.inner_R or cfg.map_f32
            or os.environ.get(off) == "1"):
        return None
    if not hasattr(_abi.load(), fam.forward):  # (an older library loaded for an A/B run)
        return None
    layout = _in_place_layout(x.shape, x.stride(), x.element_size(), x.data_ptr())
    if layout is None:
        return None
    plan = _plan(x, layout, cfg, tables=False)
    return plan if plan.ask(fam.supported) else None


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
    unchanged.  Under torch.autocast, and for float16 / float64, the float32 upcast of `_upcast`, as the fused callers.

    The L1 node saves x ALONE (its backward reads neither the maps nor a statistic): the returned maps may be modified in
    place before the backward.  The maps of the other measures are saved for the backward and must not be."""
    if cfg.padding != 0 or cfg.stride != 1 or cfg.dilation != 1:
        raise ValueError(f"nfp_valid: padding 0, stride 1, dilation 1 only (got padding={cfg.padding}, "
                         f"stride={cfg.stride}, dilation={cfg.dilation}); use nfp")
    if x.dim() != 4:
        raise RuntimeError(f"NFP expects a 4-D [B,C,H,W] feature map, got {tuple(x.shape)}")
    up = _upcast(nfp_valid, x, cfg)
    if up is not None:
        return up
    for fam in (VALID, VALID_ABS) if _measure_is_abs(cfg) else (VALID,):
        plan = _valid_route(x, cfg, fam)
        if plan is not None:
            return _maps_node(fam, x, plan, cfg, _need_grad(x))
    return nfp(x, cfg)


# ---- strided maps: stride 2 to 4, dilation 1 — include/nfp.h: nfp_strided_* (csrc/nfp_strided.hip) --------------------------
def nfp_strided(x, cfg):
    """`nfp(x, cfg)` for a layer with cfg.stride >= 2 and dilation 1 (ValueError otherwise): the `--nfp_stride` layers of the
    reference's demo.py.  A CUDA call that nfp_strided_supported accepts (cosine / dot / gfc / Norm p=2 / rmse, stride 2 to
    4, R = 1 or 2, padding 0 or R with zeros / reflect / replicate, float32 or bfloat16, padded rows of at most 128
    positions, NCHW or aligned channels-last images) runs the strided row-band kernels, one launch each way.  Everything
    else — CPU tensors, other measures, refused shapes, torch.compile, NFP_STRIDED_OFF=1 in the environment (read at call
    time: the A/B switch) — is `nfp(x, cfg)` unchanged: the any-geometry kernels.  Under torch.autocast, and for float16 /
    float64, the float32 upcast of `_upcast`, as nfp_valid.  The maps are saved for the backward and must not be modified
    in place."""
    if cfg.stride < 2 or cfg.dilation != 1:
        raise ValueError(f"nfp_strided: stride >= 2 and dilation 1 only (got stride={cfg.stride}, "
                         f"dilation={cfg.dilation}); use nfp, or nfp_valid for an unpadded stride-1 layer")
    if x.dim() != 4:
        raise RuntimeError(f"NFP expects a 4-D [B,C,H,W] feature map, got {tuple(x.shape)}")
    up = _upcast(nfp_strided, x, cfg)
    if up is not None:
        return up
    plan = _valid_route(x, cfg, STRIDED, off="NFP_STRIDED_OFF")
    if plan is not None:
        return _maps_node(STRIDED, x, plan, cfg, _need_grad(x))
    return nfp(x, cfg)


# ---- the compress-BN family (compress.py), under the names it has always had here ------------------------------------------
from .compress import (cp_sync_forward_call, cp_sync_group, cp_sync_maps_call, cp_sync_moments_call,  # noqa: E402,F401
                       cp_sync_reduce_call, cp_sync_serves, cpool_backward_call, cpool_forward_call, cpool_hip_serves,
                       cpool_wide_serves, cproj_backward_call, cproj_forward_call, cproj_hip_serves, nfp_compress_map,
                       nfp_compress_map_tensors, nfp_compress_pool, nfp_compress_pool_tensors)
# ... and its limits and routing thresholds, to be READ here as before: the family reads its own, so patch them in compress
from .compress import (CPOOL_MAX_MAPS, CPOOL_ROUTED_MAPS, CPOOL_WIDE_MAX_MAPS, CPOOL_WIDE_ROUTED_CLASSES,  # noqa: E402,F401
                       CPROJ_ROUTED_MAPS, CPROJ_ROUTED_NHWC_EVAL_MAPS, CPROJ_ROUTED_NHWC_TRAIN_PIXELS,
                       CPROJ_ROUTED_TRAIN_PIXELS)


