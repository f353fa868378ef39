"""The compress-BN family: the heads' tail GAP(relu(bn(conv1x1(maps)))) (`nfp_compress_pool`), the same projection with the
map kept (`nfp_compress_map`), and both across the ranks of an nn.SyncBatchNorm (nfp_cpsync_*).  It consumes NFP maps and
shares nothing with the maps' own binding (functional.py) but the dtype table and the device / stream helpers;
`functional` re-exports the public functions below and, to be read, the constants (patch them here).
"""
import os

import torch

from . import _abi
from ._host import compress_conv, compress_finish, compress_map_host, compress_pool_host
from .functional import _DTYPES, _need_grad, _on_device, _raw_stream


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
    need_grad = _need_grad(maps, weight, gamma, beta)
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
    need_grad = _need_grad(maps, weight, gamma, beta)
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
    need_grad = _need_grad(maps, weight, gamma, beta)
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
