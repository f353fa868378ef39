"""The cases of the per-element bf16 bars (tests/bf16_bars.py): every kernel family that stores bf16 maps, in its layouts, with
the forward and backward variant strings the family's own test file asserts, and `run_case`, which runs one of them on the GPU
and asserts both bars.  tests/test_bf16_bars_host.py pins the bars on these geometries without a GPU; scripts/bf16_bars.py
runs every case on an MI355X and prints the excesses (DESIGN §2 records them).  The cases are NOT part of the GPU suite: see
DESIGN §2.

Each case: bf16-rounded synth.feature_map inputs (kinds `normal` and `relu`, alternating along each family's list; cosine on
`relu` + 0.25, see inputs_of).  `slack` is 1e-5, the float32 bar of every x -> maps family (test_gpu_poison.F32,
test_gpu_valid.TOL).  L2 cases avoid self-pairs (no replicate padding, no reflect padding with a reach of 2 or more): a
distance of 0 is another test's subject.  The float64 formulation runs on the CPU, once per (geometry, measure, kind), shared by
the layouts and settings.

Shapes: the smallest the existing files route to each kernel (test_gpu_poison.TABLE_SHAPES and its row-band and matrix-core
cases, test_gpu_r3, test_gpu_valid, test_gpu_strided, scripts/gather_bits.py), with two found by the plan query
(tests/test_dispatch_plan.py::plan on a CPU-only machine):
  * bwd_fast<...,mfma2>: [B,192,14,14] R2 channels-last plans `mfma2` from B = 256 on and `mfma` below — the config-5 shape
    itself is the smallest;
  * fwd_tile<...,dma>: (1,64,24,24) plans the register-staged fwd_tile (several channel groups per position on a map that
    does not fill the chip); on the default dispatch the 24 x 24 map of 64 channels is staged by LDS-DMA from B = 158 on.  That
    case's backward is bwd_tile<...,dense>."""
import re

import numpy as np
import torch

import bf16_bars as BB

DEV = "cuda:0"
SLACK = 1e-5
MFMA2_BATCH = 256       # the smallest batch of [B,192,14,14] R2 nfp_plan names bwd_fast<...,mfma2> for
DMA_BATCH = 158         # the smallest batch of [B,64,24,24] R1 nfp_plan names fwd_tile<...,dma> for

MEAS = {"cos": dict(measure="cosine"), "cos_dissim": dict(measure="cosine", similarity=False), "l2": dict(measure="norm", p=2),
        "dot": dict(measure="dot")}
TAG = {"cos": "cos", "cos_dissim": "cos", "l2": "l2", "dot": "dot"}
GATHER_SETTINGS = {       # test_gpu_poison.GATHER_SETTINGS, under NFP_FORCE_GENERIC=1
    "default": ({}, "fwd_pairs", "bwd_gather"),
    "banded": ({"NFP_BWD_BANDS": "3"}, "fwd_pairs", "bwd_gather_banded"),
    "direct": ({"NFP_BWD_ATOMIC": "1", "NFP_FWD_SCALAR": "1"}, "fwd_direct", "bwd_direct"),
}


def _geo(shape, R=1, mode="reflect", padding=None, stride=1, dilation=1):
    return dict(shape=shape, R=R, padding=R if padding is None else padding, padding_mode=mode, stride=stride, dilation=dilation)


def _cases():
    """(id, family, geometry, measure, kind, layout, op, switches, forward regex, backward regex, gram, mfma)"""
    out = []

    def add(family, geos, measures, layouts, fwd, bwd, op="nfp", env=None, gram=False, mfma=False, tag=""):
        for gi, g in enumerate(geos):
            for mi, m in enumerate(measures):
                gm = dict(g, padding_mode="zeros") if (m == "l2" and g["padding_mode"] == "reflect" and g["R"] * g["dilation"] >= 2) else g
                kind = ("normal", "relu")[(gi + mi) % 2]
                for lay in layouts:
                    cid = "%s%s-%s-R%d%s-%s-%s-%s" % (family, tag, "x".join(map(str, g["shape"])), g["R"], gm["padding_mode"][:4], m, kind, lay)
                    fmt = dict(R=g["R"], tag=TAG[m], lay=lay, fam="dist" if m == "l2" else "prod")
                    out.append((cid, family, gm, m, kind, lay, op, env or {}, fwd.format(**fmt), bwd.format(**fmt),
                                gram and m == "l2", mfma))

    both = ("nchw", "nhwc")
    add("table", [_geo((3, 12, 5, 7)), _geo((2, 8, 6, 5), R=2, mode="zeros"), _geo((2, 8, 2, 2))], ("cos", "l2", "dot", "cos_dissim"), both,
        r"fwd_band<R{R},{tag},bf16,{lay}>x\d+$", r"bwd_fast<R{R},{tag},bf16,{lay}>$")
    add("mfma", [_geo((5, 32, 7, 7))], ("cos", "l2"), ("nhwc",), r"fwd_gram<R{R},{tag},bf16,{lay}>$", r"bwd_fast<R{R},{tag},bf16,{lay},mfma>$",
        env={"NFP_MFMA": "1"}, gram=True, mfma=True)
    add("mfma2", [_geo((MFMA2_BATCH, 192, 14, 14), R=2)], ("l2", "cos"), ("nhwc",), r"fwd_gram<R{R},{tag},bf16,{lay}>$",
        r"bwd_fast<R{R},{tag},bf16,{lay},mfma2>$", gram=True, mfma=True)
    add("tile", [_geo((2, 8, 24, 24)), _geo((1, 8, 30, 37)), _geo((1, 8, 30, 37), R=2, mode="zeros")], ("cos", "l2"), both,
        r"fwd_tile<R{R},{tag},bf16,{lay}>x\d+$", r"bwd_tile<R{R},{tag},bf16,{lay}>x\d+$")
    add("tile_dma", [_geo((DMA_BATCH, 64, 24, 24))], ("cos",), ("nhwc",), r"fwd_tile<R{R},{tag},bf16,{lay},dma>x\d+$",
        r"bwd_tile<R{R},{tag},bf16,{lay},dense>x\d+$")
    r3 = {"NFP_TILE_R3": "1"}
    add("tile_r3", [_geo((2, 8, 7, 7), R=3), _geo((2, 8, 14, 14), R=3)], ("cos", "l2", "dot"), both,
        r"fwd_tile<R3,{tag},bf16,{lay}>x\d+$", r"bwd_tile<R3,{tag},bf16,{lay}>x\d+$", env=r3)
    add("valid", [_geo((2, 8, 5, 5), padding=0), _geo((2, 8, 7, 7), R=2, padding=0)], ("cos", "l2"), both,
        r"fwd_valid<{R},{fam},bf16,{lay}>", r"bwd_valid<{R},{fam},bf16,{lay}>", op="valid")
    add("strided", [_geo((2, 8, 7, 7), mode="zeros", stride=2), _geo((2, 8, 9, 9), R=2, padding=0, stride=3)], ("cos", "l2"), both,
        r"fwd_strided<{R},{fam},bf16,{lay}>", r"bwd_strided<{R},{fam},bf16,{lay}>", op="strided")
    gather = [_geo((2, 8, 9, 8), padding=2, dilation=2), _geo((2, 8, 9, 8), mode="circular")]     # gather_bits.CASES: dilation2, circular_dot
    for name, (env, fwd, bwd) in GATHER_SETTINGS.items():
        add("gather", gather, ("cos", "l2"), ("nchw",), fwd + "$", bwd + "$", env=dict(env, NFP_FORCE_GENERIC="1"), tag="_" + name)
    add("gap", [_geo((2, 8, 7, 7))], ("cos",), ("nhwc",), r"fwd_band<R{R},{tag},bf16,{lay},gap>", r"bwd_fast<R{R},{tag},bf16,{lay},gap>", op="gap")
    add("gap", [_geo((2, 8, 24, 24))], ("cos",), ("nhwc",), r"fwd_tile<R{R},{tag},bf16,{lay},gap>x\d+\+pool_fold$",
        r"bwd_tile<R{R},{tag},bf16,{lay},gap>x\d+$", op="gap")
    return out


CASES = _cases()


def ctor_of(g, m):
    c = {k: g[k] for k in ("R", "padding", "padding_mode", "stride", "dilation")}
    c.update(MEAS[m])
    return c


def config_of(g, m):
    from neighbour_feature_pooling_amd import NFPPooling
    return NFPPooling(g["shape"][1], **ctor_of(g, m)).config


def _bf16_round(a):
    return torch.from_numpy(a).bfloat16().float().numpy()


def inputs_of(g, m, kind, images=None):
    """(x, grad_out), bf16-rounded; `images`: the first images only (tests/test_bf16_bars_host.py trims the two large batches)."""
    from neighbour_feature_pooling_amd.synth import feature_map
    B, C, H, W = g["shape"]
    span = g["dilation"] * 2 * g["R"] + 1
    Ho, Wo = ((v + 2 * g["padding"] - span) // g["stride"] + 1 for v in (H, W))
    N = (2 * g["R"] + 1) ** 2 - 1
    x = feature_map((B, C, H, W), 5 * H + W + 3 * C + B, kind)
    if kind == "relu" and m in ("cos", "cos_dissim"):
        # cosine needs pixels away from zero: at an all-zero pixel (8 channels of a relu map: one pixel in 256) its gradient is
        # grad_out / eps, 1e6 times the rest of the tensor, and `slack max|ref|` would then cover every other element whole
        x = x + np.float32(0.25)
    x = _bf16_round(x)
    go = _bf16_round(feature_map((B, N, Ho, Wo), 3 * H + W + 1000 + g["stride"]))
    return (x, go) if images is None else (x[:images].copy(), go[:images].copy())


_REF = {}


def _reference(g, m, kind):
    """tests/bf16_bars.py::reference of the case's inputs: computed once, shared by the layouts and settings, read-only (the
    two large batches have one case each: not kept)."""
    key = (tuple(sorted(g.items())), m, kind)
    if key in _REF:
        return _REF[key]
    x, go = inputs_of(g, m, kind)
    ref = BB.reference(x, go, config_of(g, m))
    for a in (x, go) + tuple(ref.values()):
        a.setflags(write=False)
    if x.size <= 1 << 20:
        _REF[key] = (x, go, ref)
    return x, go, ref


def run_case(case, monkeypatch):
    """One case on the GPU: the variants and both bars asserted, both excesses printed and returned.  `monkeypatch`: a
    pytest.MonkeyPatch the caller undoes; the caller also clears functional._PLANS around the call (a cached plan carries what
    the library answered under the previous switches)."""
    from conftest import nfp_switch
    from neighbour_feature_pooling_amd import _abi, functional as Fn
    cid, family, g, m, kind, lay, op, env, fwd_re, bwd_re, gram, mfma = case
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    L = _abi.load()
    for k, v in env.items():
        nfp_switch(monkeypatch, k, v)
    x, go, ref = _reference(g, m, kind)
    cfg = config_of(g, m)
    xt = torch.from_numpy(x).to(DEV).bfloat16()
    if lay == "nhwc":
        xt = xt.contiguous(memory_format=torch.channels_last)
    xt.requires_grad_(True)
    got = torch.from_numpy(go).to(DEV).bfloat16()
    if op == "gap":
        out = Fn.nfp_with_gap(xt, cfg)[1]           # maps only: GAP(x) takes no gradient
    else:
        out = {"nfp": Fn.nfp, "valid": Fn.nfp_valid, "strided": Fn.nfp_strided}[op](xt, cfg)
    fv = L.nfp_last_variant().decode()
    gx, = torch.autograd.grad(out, xt, got)
    torch.cuda.synchronize()
    bv = L.nfp_last_variant().decode()
    assert out.dtype == torch.bfloat16 and gx.dtype == torch.bfloat16 and gx.shape == xt.shape
    assert re.match(fwd_re, fv), (fv, fwd_re)       # (the patterns carry the storage type and the layout)
    assert re.match(bwd_re, bv), (bv, bwd_re)
    o, gxh = out.detach().float().cpu().numpy(), gx.float().cpu().numpy()
    e_out = BB.out_excess(o, ref["out"], SLACK, ref["gram_out"] if gram else None)
    e_gx = BB.grad_x_excess(gxh, ref["grad_x"], ref["S_gram"] if gram else ref["S"], SLACK, ref["T"] if mfma else None,
                            BB.MFMA_EPS if mfma else 0.0)
    print(f"{cid} [{fv} | {bv}]: out {e_out:.3f} grad_x {e_gx:.3f} of the one-rounding bars")
    assert e_out <= 1.0, (fv, e_out)
    assert e_gx <= 1.0, (bv, e_gx)
    return e_out, e_gx
