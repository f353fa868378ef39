"""torch.library registration of the NFP op — what keeps the drop-in promise under torch.compile.

The reference's NFP is a chain of ATen ops (nfp.py:132-159): Dynamo traces through it and a model holding it compiles
as one graph.  Here the op is a pair of HIP kernels behind a C ABI; as a `torch.autograd.Function` over ctypes / a pybind
module it is a graph BREAK per call.  Registered as custom ops — `nfp_amd::nfp`, `nfp_amd::nfp_pool` and their backward
ops, each with a fake (shape-only) implementation and an autograd formula — the same kernels sit inside one compiled
graph: `torch.compile(model, fullgraph=True)` works on a model that holds NFPPooling / nfp_pooling.

`functional.nfp` / `functional.nfp_pool` route CUDA tensors here only while Dynamo / export is tracing
(`torch.compiler.is_compiling()`); eager calls keep the C++ autograd nodes (csrc/nfp_torch.cpp), whose host cost is
lower.  The implementations below are the same C-ABI calls the eager nodes make — CUDA only: a CPU tensor runs
`_host.nfp_host`, plain torch ops that Dynamo traces natively (the probes the reference's heads run on CPU dummies,
nfp_heads.py:24-27).  Nothing here touches oracle/.
"""
import ctypes

import torch

from . import _abi
from . import functional as F

_CFG_SCHEMA = ("int R, str measure, float p, int stride, int padding, int dilation, str padding_mode, bool similarity, "
               "float eps, float q_scs, bool diff_weights, int inner_R")


def _cfg(R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R):
    return F.NfpConfig(R=R, measure=measure, p=p, stride=stride, padding=padding, dilation=dilation,
                       padding_mode=padding_mode, similarity=similarity, eps=eps, q_scs=q_scs, diff_weights=diff_weights,
                       inner_R=inner_R)


def cfg_args(cfg):
    """NfpConfig -> the positional arguments of the ops (schema types only: int / float / bool / str)."""
    return (int(cfg.R), str(cfg.measure), float(cfg.p), int(cfg.stride), int(cfg.padding), int(cfg.dilation),
            str(cfg.padding_mode), bool(cfg.similarity), float(cfg.eps), float(cfg.q_scs), bool(cfg.diff_weights),
            int(cfg.inner_R))


def _out_hw(H, W, cfg):
    span = cfg.dilation * (2 * cfg.R) + 1
    return (H + 2 * cfg.padding - span) // cfg.stride + 1, (W + 2 * cfg.padding - span) // cfg.stride + 1


def _nchw_desc(shape, dtype, cfg):
    """The descriptor of a dense NCHW tensor: enough for the library's sizes that follow from the shape and the measure."""
    return ctypes.byref(F.build_desc(shape, F._canon(shape, "nchw"), dtype, cfg))


def _saved_floats(shape, dtype, cfg, need_grad):
    """Floats of forward-to-backward state of nfp_forward for this call — a function of the shape and the measure alone
    (include/nfp.h: nfp_saved_floats), so the fake implementation can state it without a GPU."""
    if not F._keeps_state(cfg, dtype, need_grad):
        return 0
    return max(int(_abi.load().nfp_saved_floats(_nchw_desc(shape, dtype, cfg))), 0)


def _pool_saved_bound(shape, dtype, cfg):
    """An upper bound, from the shape alone, of nfp_pool_saved_floats (per-pixel state + every row band's share of the two
    pooled sums: at most H bands of C + N floats per image): what the compiled graph allocates."""
    B, C, H, W = shape
    return _saved_floats(shape, dtype, cfg, True) + B * H * (C + cfg.out_channels)


# ---- nfp: x -> (maps, saved) ------------------------------------------------------------------------------------------
@torch.library.custom_op("nfp_amd::nfp", mutates_args=(), device_types="cuda", schema=f"(Tensor x, {_CFG_SCHEMA}, bool need_grad) -> (Tensor, Tensor)")
def nfp_op(x, R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R, need_grad):
    cfg = _cfg(R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R)
    xd, plan = F._planned(x, cfg)
    bound = _saved_floats(tuple(x.shape), x.dtype, cfg, need_grad)   # (what the fake implementation states)
    return F.maps_forward_call(F.NFP, xd, plan, F._scratch_len(F.maps_saved_len(F.NFP, plan, cfg, x.dtype, need_grad), bound))


@nfp_op.register_fake
def _(x, R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R, need_grad):
    cfg = _cfg(R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R)
    B, _, H, W = x.shape
    Ho, Wo = _out_hw(H, W, cfg)
    ns = _saved_floats(tuple(x.shape), x.dtype, cfg, need_grad)
    return x.new_empty((B, cfg.out_channels, Ho, Wo)), x.new_empty((ns,), dtype=torch.float32)


@torch.library.custom_op("nfp_amd::nfp_backward", mutates_args=(), device_types="cuda",
                         schema=f"(Tensor x, Tensor out, Tensor saved, Tensor grad_out, {_CFG_SCHEMA}) -> Tensor")
def nfp_backward_op(x, out, saved, grad_out, R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs,
                    diff_weights, inner_R):
    cfg = _cfg(R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R)
    return F.maps_backward_call(F.NFP, *F._planned(x, cfg), out, saved, grad_out)


@nfp_backward_op.register_fake
def _(x, out, saved, grad_out, *cfg_fields):
    return torch.empty_like(x)


def _nfp_setup(ctx, inputs, output):
    x = inputs[0]
    ctx.cfg_fields = inputs[1:13]
    ctx.save_for_backward(x, output[0], output[1])


def _nfp_bwd(ctx, g_out, g_saved):
    x, out, saved = ctx.saved_tensors
    gx = torch.ops.nfp_amd.nfp_backward(x, out, saved, g_out, *ctx.cfg_fields)
    return (gx,) + (None,) * 13


nfp_op.register_autograd(_nfp_bwd, setup_context=_nfp_setup)


# ---- nfp_pool: x -> (gap, nfpm, maps, saved) — the fused tail of models/NFP_Pooling.py:27-31 ------------------------------
@torch.library.custom_op("nfp_amd::nfp_pool", mutates_args=(), device_types="cuda",
                         schema=f"(Tensor x, {_CFG_SCHEMA}, bool want_gap, bool need_grad) -> (Tensor, Tensor, Tensor, Tensor)")
def nfp_pool_op(x, R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R,
                want_gap, need_grad):
    cfg = _cfg(R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R)
    f32 = dict(dtype=torch.float32, device=x.device)
    if not F.nfp_pool_fused_ok(x, cfg):
        # (calls the fused kernels do not serve: the two means of the maps' own op.  The state buffer has the size the fake
        # implementation states — a function of the shape alone — with the maps' state in front)
        maps, sv = nfp_op(x, *cfg_args(cfg), need_grad)
        saved = torch.empty(_pool_saved_bound(tuple(x.shape), x.dtype, cfg), **f32)
        saved[:sv.numel()] = sv
        gap = x.float().mean((2, 3)) if want_gap else torch.empty(0, x.shape[1], **f32)
        return gap, maps.float().mean((2, 3)), maps if need_grad else maps.new_empty(0), saved
    return F.pool_forward_call(x, cfg, want_gap, need_grad, _pool_saved_bound(tuple(x.shape), x.dtype, cfg))[:4]


@nfp_pool_op.register_fake
def _(x, R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R, want_gap,
      need_grad):
    cfg = _cfg(R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R)
    B, C, H, W = x.shape
    Ho, Wo = _out_hw(H, W, cfg)
    N = cfg.out_channels
    return (x.new_empty((B if want_gap else 0, C), dtype=torch.float32), x.new_empty((B, N), dtype=torch.float32),
            x.new_empty((B, N, Ho, Wo)) if need_grad else x.new_empty((0,)),
            x.new_empty((_pool_saved_bound(tuple(x.shape), x.dtype, cfg),), dtype=torch.float32))


@torch.library.custom_op("nfp_amd::nfp_pool_backward", mutates_args=(), device_types="cuda",
                         schema=f"(Tensor x, Tensor out_map, Tensor saved, Tensor? grad_gap, Tensor grad_nfpm, {_CFG_SCHEMA}) -> Tensor")
def nfp_pool_backward_op(x, out_map, saved, grad_gap, grad_nfpm, R, measure, p, stride, padding, dilation, padding_mode,
                         similarity, eps, q_scs, diff_weights, inner_R):
    cfg = _cfg(R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R)
    P = out_map.shape[2] * out_map.shape[3]
    if not F.nfp_pool_fused_ok(x, cfg):
        go = (grad_nfpm.to(out_map.dtype) / P)[:, :, None, None].expand_as(out_map).contiguous()
        gx = nfp_backward_op(x, out_map, saved, go, *cfg_args(cfg)).float()
        if grad_gap is not None:
            gx = gx + (grad_gap.float() / (x.shape[2] * x.shape[3]))[:, :, None, None]
        return gx.to(x.dtype)
    return F.pool_backward_call(*F._planned(x, cfg), out_map, saved, grad_gap, grad_nfpm)


@nfp_pool_backward_op.register_fake
def _(x, out_map, saved, grad_gap, grad_nfpm, *cfg_fields):
    return torch.empty_like(x)


def _pool_setup(ctx, inputs, output):
    ctx.cfg_fields = inputs[1:13]
    ctx.want_gap = inputs[13]
    ctx.save_for_backward(inputs[0], output[2], output[3])


def _pool_bwd(ctx, g_gap, g_nfpm, g_map, g_saved):
    x, out_map, saved = ctx.saved_tensors
    gx = torch.ops.nfp_amd.nfp_pool_backward(x, out_map, saved, g_gap if ctx.want_gap else None, g_nfpm, *ctx.cfg_fields)
    return (gx,) + (None,) * 14


nfp_pool_op.register_autograd(_pool_bwd, setup_context=_pool_setup)


# ---- nfp_gap: x -> (gap, maps, saved) — GAP(x) beside the full maps, the first step of an NFP head -------------------------
def _gap_saved_bound(shape, dtype, cfg):
    """An upper bound, from the shape alone, of nfp_gap_saved_floats (per-pixel state + at most H row bands of C partial
    channel sums per image): what the compiled graph allocates."""
    B, C, H, W = shape
    return max(_saved_floats(shape, dtype, cfg, True) + B * H * C, 1)


@torch.library.custom_op("nfp_amd::nfp_gap", mutates_args=(), device_types="cuda",
                         schema=f"(Tensor x, {_CFG_SCHEMA}) -> (Tensor, Tensor, Tensor)")
def nfp_gap_op(x, R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R):
    cfg = _cfg(R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R)
    ns = _gap_saved_bound(tuple(x.shape), x.dtype, cfg)
    if not F.nfp_gap_fused_ok(x, cfg):
        # (functional.nfp_with_gap asked the library at trace time; what only the run shows — a misaligned channels-last
        # pointer, a geometry first seen inside a graph capture — is served here by the maps' own op and a mean, never an
        # error.  The state buffer has the size the fake implementation states, the maps' state in front)
        maps, sv = nfp_op(x, *cfg_args(cfg), True)
        saved = torch.empty(ns, dtype=torch.float32, device=x.device)
        saved[:sv.numel()] = sv
        return x.float().mean((2, 3)), maps, saved
    return F.gap_forward_call(x, cfg, ns)


@nfp_gap_op.register_fake
def _(x, R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R):
    cfg = _cfg(R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R)
    B, C, H, W = x.shape
    Ho, Wo = _out_hw(H, W, cfg)
    return (x.new_empty((B, C), dtype=torch.float32), x.new_empty((B, cfg.out_channels, Ho, Wo)),
            x.new_empty((_gap_saved_bound(tuple(x.shape), x.dtype, cfg),), dtype=torch.float32))


@torch.library.custom_op("nfp_amd::nfp_gap_backward", mutates_args=(), device_types="cuda",
                         schema=f"(Tensor x, Tensor maps, Tensor saved, Tensor? grad_gap, Tensor? grad_maps, {_CFG_SCHEMA}) -> Tensor")
def nfp_gap_backward_op(x, maps, saved, grad_gap, grad_maps, R, measure, p, stride, padding, dilation, padding_mode,
                        similarity, eps, q_scs, diff_weights, inner_R):
    cfg = _cfg(R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R)
    if not F.nfp_gap_fused_ok(x, cfg):
        go = torch.zeros_like(maps) if grad_maps is None else grad_maps
        ns = _saved_floats(tuple(x.shape), x.dtype, cfg, True)
        gx = nfp_backward_op(x, maps, saved[:ns], go, *cfg_args(cfg))
        if grad_gap is not None:
            gx = (gx.float() + (grad_gap.float() / (x.shape[2] * x.shape[3]))[:, :, None, None]).to(x.dtype)
        return gx
    return F.gap_backward_call(x, cfg, maps, saved, grad_gap, grad_maps)


@nfp_gap_backward_op.register_fake
def _(x, maps, saved, grad_gap, grad_maps, *cfg_fields):
    return torch.empty_like(x)


def _gap_setup(ctx, inputs, output):
    ctx.cfg_fields = inputs[1:13]
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(inputs[0], output[1], output[2])


def _gap_bwd(ctx, g_gap, g_maps, g_saved):
    x, maps, saved = ctx.saved_tensors
    if g_gap is None and g_maps is None:
        return (None,) * 13
    gx = torch.ops.nfp_amd.nfp_gap_backward(x, maps, saved, g_gap, g_maps, *ctx.cfg_fields)
    return (gx,) + (None,) * 12


nfp_gap_op.register_autograd(_gap_bwd, setup_context=_gap_setup)


# ---- nfp_biased: (x, centre_bias, neighbour_bias) -> (maps, saved) — NFPPooling(bias=True), include/nfp.h ABI 7 ------------
def _bias_saved_floats(shape, dtype, cfg):
    """nfp_bias_saved_floats for this call — a function of the shape and the measure alone."""
    return max(int(_abi.load().nfp_bias_saved_floats(_nchw_desc(shape, dtype, cfg))), 0)


@torch.library.custom_op("nfp_amd::nfp_biased", mutates_args=(), device_types="cuda",
                         schema=f"(Tensor x, Tensor centre_bias, Tensor neighbour_bias, {_CFG_SCHEMA}) -> (Tensor, Tensor)")
def nfp_biased_op(x, centre_bias, neighbour_bias, R, measure, p, stride, padding, dilation, padding_mode, similarity, eps,
                  q_scs, diff_weights, inner_R):
    cfg = _cfg(R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R)
    return F.bias_forward_call(x, centre_bias, neighbour_bias, cfg)


@nfp_biased_op.register_fake
def _(x, centre_bias, neighbour_bias, R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs,
      diff_weights, inner_R):
    cfg = _cfg(R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R)
    B, _, H, W = x.shape
    Ho, Wo = _out_hw(H, W, cfg)
    return (x.new_empty((B, cfg.out_channels, Ho, Wo)),
            x.new_empty((_bias_saved_floats(tuple(x.shape), x.dtype, cfg),), dtype=torch.float32))


@torch.library.custom_op("nfp_amd::nfp_biased_backward", mutates_args=(), device_types="cuda",
                         schema=f"(Tensor x, Tensor centre_bias, Tensor neighbour_bias, Tensor out, Tensor saved, "
                                f"Tensor grad_out, {_CFG_SCHEMA}) -> (Tensor, Tensor, Tensor)")
def nfp_biased_backward_op(x, centre_bias, neighbour_bias, out, saved, grad_out, R, measure, p, stride, padding, dilation,
                           padding_mode, similarity, eps, q_scs, diff_weights, inner_R):
    cfg = _cfg(R, measure, p, stride, padding, dilation, padding_mode, similarity, eps, q_scs, diff_weights, inner_R)
    gx, gcb, gnb = F.bias_backward_call(x, centre_bias, neighbour_bias, out, saved, grad_out, cfg)
    if gcb is None:     # (Norm / RMSE: no centre-bias gradient; the autograd formula below returns None for it)
        gcb = torch.zeros(centre_bias.shape, dtype=torch.float32, device=x.device)
    return gx, gcb.to(centre_bias.dtype), gnb.to(neighbour_bias.dtype)


@nfp_biased_backward_op.register_fake
def _(x, centre_bias, neighbour_bias, out, saved, grad_out, *cfg_fields):
    return torch.empty_like(x), torch.empty_like(centre_bias), torch.empty_like(neighbour_bias)


def _biased_setup(ctx, inputs, output):
    ctx.cfg_fields = inputs[3:15]
    ctx.save_for_backward(inputs[0], inputs[1], inputs[2], output[0], output[1])


def _biased_bwd(ctx, g_out, g_saved):
    x, cb, nb, out, saved = ctx.saved_tensors
    gx, gcb, gnb = torch.ops.nfp_amd.nfp_biased_backward(x, cb, nb, out, saved, g_out, *ctx.cfg_fields)
    no_centre = ctx.cfg_fields[1] in ("norm", "rmse")
    return (gx, None if no_centre else gcb, gnb) + (None,) * 12


nfp_biased_op.register_autograd(_biased_bwd, setup_context=_biased_setup)
