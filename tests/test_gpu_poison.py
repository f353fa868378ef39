"""Every buffer the binding hands the HIP kernels, poisoned and fenced (tests/poison.py; DESIGN.md, "Caller-allocated
buffers"): a kernel writes every element of every buffer it owns, and never lets a value it did not write reach a result.

ONE assertion for every case (poison.run_fills): forward and backward run three times on fresh, fenced copies of the same
inputs, the binding's `torch.empty` / `torch.empty_like` buffers filled with zeros, with quiet NaNs and with +-3e38; every
tensor the caller can see — outputs, every gradient asked for, the running statistics, the records and rows the staged
calls exchange — is bit for bit the same in the three runs, nfp_last_variant() after the forward and after the backward is
the same and names the kernel the case is meant for, and no guard byte around any buffer, input or output, has changed.
`saved` and scratch are exempt from the comparison (their sizes are upper bounds), not from the guards.  The "zero" run is
also held to the float64 host formulation of the same inputs at the bar of the family's own test file.

Only the Python autograd nodes allocate in Python, so they serve here (NFP_PY_NODES=1 and functional._CPP = None, as
tests/test_gpu_valid_abs.py selects them); the suite holds the C++ nodes bitwise equal to them.

What the float buffers carry, read in the kernels before poisoning them: `saved` (per-pixel norms and statistics, the row
bands' partial sums, bf16 Attention's raw dots), the scratch of the biased, attention-pool and compress-BN backwards
(partial sums), the staged calls' records (float64 count, mean, scatter: the count is summed as a double, never converted
to an index) and rows (k, Q) — float data only.  The arrival counters and index tables live in the uint8 workspace of
functional._workspace alone, which the harness zero-fills in every run.
"""
import hashlib
import importlib.util
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import poison as P
import test_gpu_cpool as KP
import test_gpu_cproj as KJ
from conftest import ROOT, nfp_switch, rel_err

pytestmark = pytest.mark.gpu

F32, BF_OUT, BF_GRAD = 1e-5, 1e-2, 2e-2          # test_gpu_parity.py, test_gpu_tile.py, test_gpu_valid.py, test_gpu_gap.py
BIAS_F32, BIAS_F32_LOOSE = 1e-4, 5e-4            # test_gpu_bias.py (LOOSE: its list of measures)
BIAS_LOOSE = ("geman", "pearson", "hellinger", "squaredchord", "jeffrey", "smith", "canberra", "chisquared1", "chisquared2")
DEV = "cuda:0"


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GB = _script("gather_bits")      # CASES: the any-geometry table
CB = _script("cp_bits")          # cases(), SYNC_CASES, inputs, on_device, shifted_out: the compress-BN table


@pytest.fixture(autouse=True)
def _python_nodes_and_fresh_plans(monkeypatch):
    from neighbour_feature_pooling_amd import _abi, functional
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _abi.load()
    monkeypatch.setenv("NFP_PY_NODES", "1")
    monkeypatch.setattr(functional, "_CPP", None)
    assert not functional._cpp_nodes()
    # (a cached plan carries what the library said under the previous test's switches: the pooled scratch size of the other arm)
    monkeypatch.setattr(functional, "_PLANS", OrderedDict())
    yield


def _variant():
    from neighbour_feature_pooling_amd import _abi
    return _abi.load().nfp_last_variant().decode()


def _seed(name):
    return int(hashlib.sha256(name.encode()).hexdigest()[:6], 16)


def _np(t):
    return t.detach().double().cpu().numpy()


def _placed(x0, layout):
    """x0 (CPU, already in its dtype) on the device as the case reads it: NCHW, channels-last, or the [B,C,H,W] view of
    [B, 1 + HW, C] tokens behind a class token (batch stride (1 + HW) C — `fenced` poisons the class tokens)."""
    x = x0.to(DEV)
    if layout == "nhwc":
        return x.contiguous(memory_format=torch.channels_last)
    if layout == "tokens":
        B, C, H, W = x.shape
        buf = torch.zeros(B, 1 + H * W, C, device=DEV, dtype=x.dtype)
        buf[:, 1:] = x.flatten(2).transpose(1, 2)
        return buf[:, 1:].transpose(1, 2).unflatten(2, (H, W))
    assert layout == "nchw", layout
    return x


# ---- the "x -> maps" families: nfp, nfp_valid, nfp_biased ----------------------------------------------------------------
class MapsCase:
    """One layer call on seeded inputs made on the CPU (positive: valid for every measure), as scripts/gather_bits.py makes
    them: flags "nhwc" / "tokens", "bf16", "mix" (bf16 under autocast with float32 maps)."""

    def __init__(self, name, shape, ctor, flags=(), op="layer"):
        from neighbour_feature_pooling_amd import NFPPooling
        self.name, self.shape, self.flags, self.op = name, shape, flags, op
        self.bias = bool(ctor.get("bias"))
        seed = _seed(name)
        torch.manual_seed(seed)        # (bias=True draws its biases from the global generator)
        self.layer = NFPPooling(shape[1], **ctor)
        self.g = torch.Generator().manual_seed(seed + 1)
        low = "bf16" in flags or "mix" in flags
        self.x0 = (torch.rand(*shape, generator=self.g) + 0.25).to(torch.bfloat16 if low else torch.float32)
        self.layout = "nhwc" if "nhwc" in flags else ("tokens" if "tokens" in flags else "nchw")
        self.go0 = None

    def __call__(self, poison):
        from neighbour_feature_pooling_amd import functional as Fn
        xd = _placed(self.x0, self.layout)
        x = poison.fenced(xd).requires_grad_(True)
        assert x.stride() == xd.stride() and x.data_ptr() % P.GUARD == xd.data_ptr() % P.GUARD
        cfg, params = self.layer.config, []
        if self.bias:
            params = [poison.fenced(p.detach().to(DEV)).requires_grad_(True)
                      for p in (self.layer.center_value.bias, self.layer.comp_neighbors.bias)]
        with torch.autocast("cuda", torch.bfloat16, enabled="mix" in self.flags):
            if self.bias:
                out = Fn.nfp_biased(x, cfg, *params)
            else:
                out = (Fn.nfp_valid if self.op == "valid" else Fn.nfp)(x, cfg)
        fv = _variant()
        assert out.dtype == (torch.float32 if "mix" in self.flags else x.dtype), (self.name, out.dtype)
        if self.go0 is None:
            self.go0 = torch.randn(out.shape, generator=self.g).to(out.dtype)
        go = poison.fenced(self.go0.to(DEV))
        grads = torch.autograd.grad(out, [x] + params, go, allow_unused=True)
        torch.cuda.synchronize()
        res = dict(out=out.detach(), grad_x=grads[0], fwd=fv, bwd=_variant(), grad_x_strides=str(grads[0].stride()))
        if self.bias:
            res.update(grad_centre_bias=grads[1], grad_neighbour_bias=grads[2])
        return res

    def reference(self):
        """(out, grad_x[, grad_centre_bias or None, grad_neighbour_bias]) of _host.nfp_host in float64 on the same (already
        rounded) inputs."""
        from neighbour_feature_pooling_amd._host import nfp_host
        x = self.x0.double().requires_grad_(True)
        params = []
        if self.bias:
            params = [p.detach().double().requires_grad_(True) for p in (self.layer.center_value.bias, self.layer.comp_neighbors.bias)]
        out = nfp_host(x, self.layer.config, *params)
        return (out.detach(),) + torch.autograd.grad(out, [x] + params, self.go0.double(), allow_unused=True)

    def check(self, fwd, bwd, no_bwd=()):
        res = P.run_fills(self, self.name)
        print(self.name, res["fwd"], "|", res["bwd"])
        assert res["fwd"].startswith(fwd), (res["fwd"], fwd)
        assert res["bwd"].startswith(bwd), (res["bwd"], bwd)
        assert not any(res["bwd"].startswith(n) for n in no_bwd), (res["bwd"], no_bwd)
        ref = self.reference()
        if self.bias:
            t_out = t_g = BIAS_F32_LOOSE if self.layer.config.measure in BIAS_LOOSE else BIAS_F32
        elif "mix" in self.flags:
            t_out, t_g = F32, BF_GRAD
        elif "bf16" in self.flags:
            t_out, t_g = BF_OUT, BF_GRAD
        else:
            t_out = t_g = F32
        # (NaNs as tests/test_gpu_parity.py takes them: a zero Hellinger distance has no derivative — nhwc_stride2's replicated border)
        err = lambda a, r: rel_err(np.nan_to_num(_np(a)), np.nan_to_num(_np(r)))     # noqa: E731
        errs = dict(out=err(res["out"], ref[0]), grad_x=err(res["grad_x"], ref[1]))
        if self.bias:
            assert (res["grad_centre_bias"] is None) == (ref[2] is None)
            if ref[2] is not None:
                errs["grad_centre_bias"] = err(res["grad_centre_bias"], ref[2])
            errs["grad_neighbour_bias"] = err(res["grad_neighbour_bias"], ref[3])
        print(self.name, errs, "bars", t_out, t_g)
        assert errs.pop("out") <= t_out
        assert all(e <= t_g for e in errs.values()), errs
        return res


def _same(R, measure, **kw):
    """A "same" map: stride 1, pad = R."""
    return dict(R=R, measure=measure, padding=R, **kw)


MEASURES = {"cosine": dict(measure="cosine"), "l2": dict(measure="norm", p=2), "l1": dict(measure="norm", p=1),
            "canberra": dict(measure="canberra")}
STORAGE = [("f32", "nchw"), ("f32", "nhwc"), ("bf16", "nchw"), ("bf16", "nhwc")]


def _flags(dtype, layout):
    return tuple(f for f in (dtype, layout) if f not in ("f32", "nchw"))


# ---- table kernels: fwd_band / bwd_fast, fwd_gram / bwd_gemm -------------------------------------------------------------
TABLE_SHAPES = [((3, 12, 5, 7), 1),       # 35 pixels: P % 4 != 0, three channel quads
                ((2, 8, 2, 2), 1),        # the smallest map fast_geometry admits
                ((2, 8, 6, 5), 2)]


@pytest.mark.parametrize("dtype,layout", STORAGE, ids=["-".join(s) for s in STORAGE])
@pytest.mark.parametrize("meas", list(MEASURES))
@pytest.mark.parametrize("shape,R", TABLE_SHAPES, ids=["x".join(map(str, s)) + "-R%d" % r for s, r in TABLE_SHAPES])
def test_table_kernels(shape, R, meas, dtype, layout):
    name = "table_%s_R%d_%s_%s_%s" % ("x".join(map(str, shape)), R, meas, dtype, layout)
    res = MapsCase(name, shape, dict(R=R, padding=R, **MEASURES[meas]), _flags(dtype, layout)).check("fwd_band<", "bwd_fast<")
    assert layout in res["fwd"] and layout in res["bwd"] and dtype in res["fwd"] and dtype in res["bwd"], res


def test_table_kernels_read_tokens_behind_a_class_token_in_place():
    res = MapsCase("table_tokens", (3, 12, 5, 7), _same(1, "cosine"), ("tokens",)).check("fwd_band<", "bwd_fast<")
    assert "nhwc" in res["fwd"] and "nhwc" in res["bwd"], res


@pytest.mark.parametrize("mfma", ["1", "0"], ids=["mfma", "no_mfma"])
def test_matrix_core_kernels(mfma, monkeypatch):
    nfp_switch(monkeypatch, "NFP_MFMA", mfma)
    case = MapsCase("table_5x32x7x7_bf16_nhwc_mfma" + mfma, (5, 32, 7, 7), _same(1, "cosine"), ("bf16", "nhwc"))
    res = case.check("fwd_gram<" if mfma == "1" else "fwd_band<", "bwd_fast<")
    assert ("mfma" in res["bwd"]) == (mfma == "1"), res["bwd"]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("meas", ["cosine", "l2"])
def test_native_autocast_call_on_the_table_kernels(meas, layout, monkeypatch):
    """NFP_AMP_NATIVE=1: bf16 x in, float32 maps out, a bf16 grad_x back (map_f32)."""
    monkeypatch.setenv("NFP_AMP_NATIVE", "1")
    case = MapsCase("table_mix_%s_%s" % (meas, layout), (3, 12, 5, 7), dict(R=1, padding=1, **MEASURES[meas]),
                    _flags("mix", layout))
    res = case.check("fwd_band<", "bwd_fast<")
    assert res["out"].dtype == torch.float32 and res["grad_x"].dtype == torch.bfloat16


# ---- row-band kernels: fwd_tile / bwd_tile -----------------------------------------------------------------------------
BAND_CTORS = {"R1_reflect": _same(1, "cosine", padding_mode="reflect"), "R2_zeros": _same(2, "norm", p=2, padding_mode="zeros")}
BAND_STORAGE = [("f32", "nchw"), ("f32", "nhwc"), ("bf16", "nhwc")]


@pytest.mark.parametrize("dtype,layout", BAND_STORAGE, ids=["-".join(s) for s in BAND_STORAGE])
@pytest.mark.parametrize("shape,ctor", [((2, 8, 24, 24), "R1_reflect"),        # the first size above 512 pixels
                                        ((1, 8, 30, 37), "R1_reflect"),        # odd rows, a short last band
                                        ((1, 8, 30, 37), "R2_zeros")],
                         ids=["2x8x24x24-R1_reflect", "1x8x30x37-R1_reflect", "1x8x30x37-R2_zeros"])
def test_row_band_kernels(shape, ctor, dtype, layout):
    name = "band_%s_%s_%s_%s" % ("x".join(map(str, shape)), ctor, dtype, layout)
    res = MapsCase(name, shape, BAND_CTORS[ctor], _flags(dtype, layout)).check("fwd_tile<", "bwd_tile<")
    assert layout in res["fwd"] and layout in res["bwd"], res


@pytest.mark.parametrize("shape,ctor", [((2, 8, 24, 24), "R1_reflect"), ((1, 8, 30, 37), "R1_reflect"), ((1, 8, 30, 37), "R2_zeros")],
                         ids=["2x8x24x24-R1_reflect", "1x8x30x37-R1_reflect", "1x8x30x37-R2_zeros"])
def test_row_band_forward_staged_by_lds_dma(shape, ctor, monkeypatch):
    nfp_switch(monkeypatch, "NFP_TILE_DMA", "1")
    name = "band_dma_%s_%s" % ("x".join(map(str, shape)), ctor)
    MapsCase(name, shape, BAND_CTORS[ctor], ("nhwc",)).check("fwd_tile<", "bwd_tile<")


def test_row_band_kernels_read_tokens_behind_a_class_token_in_place():
    MapsCase("band_tokens", (2, 8, 24, 24), BAND_CTORS["R1_reflect"], ("tokens",)).check("fwd_tile<", "bwd_tile<")


# ---- any-geometry kernels: the table of scripts/gather_bits.py, three settings ---------------------------------------------
GATHER_SETTINGS = {
    "default": ({}, "fwd_pairs", "bwd_gather", ("bwd_gather_banded",)),
    "banded": ({"NFP_BWD_BANDS": "3"}, "fwd_pairs", ("bwd_gather_banded", "bwd_direct"), ()),     # (bwd_direct: the launcher declines)
    "direct": ({"NFP_BWD_ATOMIC": "1", "NFP_FWD_SCALAR": "1"}, "fwd_direct", "bwd_direct", ()),
}


@pytest.mark.parametrize("setting", list(GATHER_SETTINGS))
@pytest.mark.parametrize("case", GB.CASES, ids=[c[0] for c in GB.CASES])
def test_any_geometry_kernels(case, setting, monkeypatch):
    name, shape, ctor, flags = case
    env, fwd, bwd, no_bwd = GATHER_SETTINGS[setting]
    nfp_switch(monkeypatch, "NFP_FORCE_GENERIC", "1")
    for k in ("NFP_BWD_BANDS", "NFP_BWD_ATOMIC", "NFP_FWD_SCALAR"):
        nfp_switch(monkeypatch, k, env.get(k))
    monkeypatch.setenv("NFP_AMP_NATIVE", "1")      # (the map_f32 cases: the native autocast call is opt-in)
    if ctor.get("bias"):
        fwd, bwd, no_bwd = "bias_fwd<", "bias_bwd<", ()
    MapsCase(name, shape, ctor, flags).check(fwd, bwd, no_bwd)


# ---- biased kernels on the default dispatch -------------------------------------------------------------------------------
BIAS_CASES = [c for c in GB.CASES if c[2].get("bias")] + [
    ("bias_norm_no_centre", (2, 6, 7, 8), dict(R=1, measure="norm", p=2, padding=1, bias=True), ()),
    ("bias_rmse_no_centre_nhwc", (2, 5, 9, 8), dict(R=1, measure="rmse", padding=1, bias=True), ("nhwc",))]


@pytest.mark.parametrize("case", BIAS_CASES, ids=[c[0] for c in BIAS_CASES])
def test_biased_kernels(case):
    from neighbour_feature_pooling_amd.functional import bias_no_centre
    name, shape, ctor, flags = case
    assert len(BIAS_CASES) == 4
    mc = MapsCase("default_" + name, shape, ctor, flags)
    res = mc.check("bias_fwd<", "bias_bwd<")
    assert (res["grad_centre_bias"] is None) == bias_no_centre(mc.layer.config) == ("no_centre" in name)


# ---- valid-map kernels: fwd_valid / bwd_valid and their l1 instantiation -----------------------------------------------
VALID_CASES = [((1, 4, 5, 5), 2, "nchw"),        # a 1 x 1 output
               ((2, 5, 5, 7), 1, "nchw"),
               ((2, 8, 9, 11), 1, "nhwc"), ((2, 8, 9, 11), 2, "nhwc")]
VALID_KIND = {"cosine": "prod", "l2": "dist", "l1": "l1"}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("meas", list(VALID_KIND))
@pytest.mark.parametrize("shape,R,layout", VALID_CASES, ids=["%s-R%d-%s" % ("x".join(map(str, s)), r, l) for s, r, l in VALID_CASES])
def test_valid_map_kernels(shape, R, layout, meas, dtype):
    name = "valid_%s_R%d_%s_%s_%s" % ("x".join(map(str, shape)), R, layout, meas, dtype)
    ctor = dict(R=R, padding=0, **MEASURES[meas])
    res = MapsCase(name, shape, ctor, _flags(dtype, layout), op="valid").check("fwd_valid<%d,%s," % (R, VALID_KIND[meas]),
                                                                                "bwd_valid<%d,%s," % (R, VALID_KIND[meas]))
    assert layout in res["fwd"] and dtype in res["fwd"] and layout in res["bwd"] and dtype in res["bwd"], res
    if shape == (1, 4, 5, 5):
        assert res["out"].shape[2:] == (1, 1)


def test_valid_map_kernels_read_tokens_behind_a_class_token_in_place():
    MapsCase("valid_tokens", (2, 8, 9, 11), dict(R=1, padding=0, **MEASURES["l1"]), ("tokens",), op="valid").check(
        "fwd_valid<1,l1,", "bwd_valid<1,l1,")


# ---- the fused pooling tail (nfp_pool) and nfp_with_gap ---------------------------------------------------------------------
def _host_maps64(x64, cfg):
    import dataclasses
    from neighbour_feature_pooling_amd._host import nfp_host
    if cfg.inner_R:
        return torch.cat([nfp_host(x64, dataclasses.replace(cfg, R=cfg.inner_R, padding=cfg.inner_R, inner_R=0)),
                          nfp_host(x64, dataclasses.replace(cfg, inner_R=0))], dim=1)
    return nfp_host(x64, cfg)


class TailCase:
    """nfp_pool (GAP(x), GAP(NFP(x))) or nfp_with_gap (GAP(x), NFP(x)) under seeded gradients of both outputs; `use`: which
    of the two outputs take part in the backward ("both", "first", "second", or "none": no gradient follows)."""

    def __init__(self, name, op, shape, cfg, use, layout="nchw"):
        self.name, self.op, self.shape, self.cfg, self.use, self.layout = name, op, shape, cfg, use, layout
        self.g = torch.Generator().manual_seed(_seed(name))
        self.x0 = torch.rand(*shape, generator=self.g) + 0.25
        self.w0 = None

    def __call__(self, poison):
        from neighbour_feature_pooling_amd import functional as Fn
        x = poison.fenced(_placed(self.x0, self.layout))
        if self.use != "none":
            x.requires_grad_(True)
        if self.op in ("pool_op", "gap_op"):        # the registered custom ops, called eagerly: the compiled graph's buffers
            from neighbour_feature_pooling_amd import _ops
            if self.op == "pool_op":
                outs = torch.ops.nfp_amd.nfp_pool(x, *_ops.cfg_args(self.cfg), True, self.use != "none")[:2]
            else:
                outs = torch.ops.nfp_amd.nfp_gap(x, *_ops.cfg_args(self.cfg))[:2]
        else:
            outs = (Fn.nfp_pool if self.op == "pool" else Fn.nfp_with_gap)(x, self.cfg)
        fv = _variant()
        if self.w0 is None:
            self.w0 = [torch.randn(o.shape, generator=self.g) for o in outs]
        res = dict(first=outs[0].detach(), second=outs[1].detach(), fwd=fv)
        if self.use != "none":
            pick = {"both": (0, 1), "first": (0,), "second": (1,)}[self.use]
            ws = [poison.fenced(self.w0[i].to(DEV)) for i in pick]
            gx, = torch.autograd.grad([outs[i] for i in pick], x, ws)
            torch.cuda.synchronize()
            res.update(grad_x=gx, bwd=_variant())
        return res

    def check(self, fwd, bwd, tag):
        res = P.run_fills(self, self.name)
        print(self.name, res["fwd"], "|", res.get("bwd"))
        assert res["fwd"].startswith(fwd) and tag in res["fwd"], (res["fwd"], fwd, tag)
        x = self.x0.double().requires_grad_(True)
        maps = _host_maps64(x, self.cfg)
        ref = (x.mean((2, 3)), maps.mean((2, 3)) if self.op.startswith("pool") else maps)
        assert rel_err(_np(res["first"]), _np(ref[0])) <= F32 and rel_err(_np(res["second"]), _np(ref[1])) <= F32
        if self.use != "none":
            assert res["bwd"].startswith(bwd) and tag in res["bwd"], (res["bwd"], bwd, tag)
            pick = {"both": (0, 1), "first": (0,), "second": (1,)}[self.use]
            gref, = torch.autograd.grad([ref[i] for i in pick], x, [self.w0[i].double() for i in pick])
            assert rel_err(_np(res["grad_x"]), _np(gref)) <= F32
        return res


def _cfg(C, **ctor):
    from neighbour_feature_pooling_amd import NFPPooling
    return NFPPooling(C, **ctor).config


@pytest.mark.parametrize("need_grad", [True, False], ids=["grad", "no_grad"])
@pytest.mark.parametrize("ticket", [None, "1"], ids=["product", "ticket"])
@pytest.mark.parametrize("shape", [(3, 8, 7, 7), (2, 8, 24, 24)], ids=["3x8x7x7", "2x8x24x24"])
def test_fused_pooling_tail(shape, ticket, need_grad, monkeypatch):
    """Both arms of the band combine (NFP_POOL_TICKET, as tests/test_gpu_tile.py selects them): pool_fold as a launch of its
    own, and the last band to arrive inside the one launch; without a gradient to follow the maps are not stored."""
    nfp_switch(monkeypatch, "NFP_POOL_TICKET", ticket)
    big = shape[2] * shape[3] > 512
    name = "pool_%s_%s_%s" % ("x".join(map(str, shape)), ticket, need_grad)
    case = TailCase(name, "pool", shape, _cfg(shape[1], **_same(1, "cosine")), "both" if need_grad else "none")
    res = case.check("fwd_tile<" if big else "fwd_band<", "bwd_tile<" if big else "bwd_fast<", ",pool>")
    if ticket:
        assert "pool_fold" not in res["fwd"], res["fwd"]
    elif big:
        assert res["fwd"].endswith("+pool_fold"), res["fwd"]


GAP_CASES = [("gap_3x8x7x7_R1", (3, 8, 7, 7), 0), ("gap_2x8x7x7_R1+2", (2, 8, 7, 7), 1)]


@pytest.mark.parametrize("use", ["both", "first", "second"], ids=["both", "grad_maps_undefined", "grad_gap_undefined"])
@pytest.mark.parametrize("name,shape,inner", GAP_CASES, ids=[c[0] for c in GAP_CASES])
def test_nfp_with_gap(name, shape, inner, use):
    from neighbour_feature_pooling_amd.functional import multi_radius_config
    cfg = _cfg(shape[1], **_same(1, "cosine"))
    if inner:
        cfg = multi_radius_config(cfg, _cfg(shape[1], **_same(2, "cosine")))
        assert cfg is not None and cfg.inner_R == 1
    res = TailCase(name + "_" + use, "gap", shape, cfg, use).check("fwd_band<R1+2" if inner else "fwd_band<R1,", "bwd_fast<", ",gap>")
    assert res["second"].shape[1] == (32 if inner else 8)


def test_nfp_with_gap_reads_tokens_behind_a_class_token_in_place():
    TailCase("gap_tokens", "gap", (3, 8, 7, 7), _cfg(8, **_same(1, "cosine")), "both", "tokens").check("fwd_band<", "bwd_fast<", ",gap>")


# ---- the registered custom ops (_ops.py), called eagerly: what a compiled graph runs, with its shape-only buffer bounds -----
OPS_CASES = [("pool_op", (3, 8, 7, 7), _same(1, "cosine"), "fwd_band<", "bwd_fast<", ",pool>"),
             ("pool_op", (2, 8, 24, 24), _same(1, "cosine"), "fwd_tile<", "bwd_tile<", ",pool>"),     # `saved` longer than the library asks
             ("pool_op", (2, 8, 9, 8), dict(R=1, measure="canberra", padding=1), "fwd_band<", "bwd_fast<", ""),   # not fused: the maps' op
             ("gap_op", (3, 8, 7, 7), _same(1, "cosine"), "fwd_band<", "bwd_fast<", ",gap>"),
             ("gap_op", (2, 8, 24, 24), _same(1, "cosine"), "fwd_tile<", "bwd_tile<", ",gap>"),
             ("gap_op", (2, 8, 9, 8), dict(R=1, measure="cosine", padding=1, stride=2), "fwd_pairs", "bwd_gather", "")]


# (GAP(x) alone of the unfused pooled tail is a torch mean whose gradient needs no kernel: left out)
OPS_GRID = [c + (use,) for c in OPS_CASES for use in ("both", "first", "second") if not (c[0] == "pool_op" and not c[5] and use == "first")]


@pytest.mark.parametrize("op,shape,ctor,fwd,bwd,tag,use", OPS_GRID,
                         ids=["%s-%s-%s%s-%s" % (c[0], "x".join(map(str, c[1])), c[2]["measure"], "_s2" if c[2].get("stride") else "", c[6])
                              for c in OPS_GRID])
def test_custom_ops_on_the_compiled_graphs_buffers(op, shape, ctor, fwd, bwd, tag, use):
    """torch.ops.nfp_amd.nfp_pool / nfp_gap outside torch.compile: the device branches of _ops.py, whose `saved` has the
    length the fake implementation states from the shape alone — an upper bound the kernels must neither rely on nor read
    beyond what they wrote — and, where the fused kernels do not serve, the maps' own op under the same buffers."""
    TailCase("%s_%s_%s_%s" % (op, "x".join(map(str, shape)), ctor["measure"], use), op, shape, _cfg(shape[1], **ctor), use).check(fwd, bwd, tag)


def test_the_maps_custom_op_eagerly():
    from neighbour_feature_pooling_amd import _ops
    x0 = torch.rand(2, 8, 6, 5, generator=torch.Generator().manual_seed(5)) + 0.25
    go0 = torch.randn(2, 8, 6, 5, generator=torch.Generator().manual_seed(6))
    cfg = _cfg(8, **_same(1, "cosine"))

    def case(poison):
        x = poison.fenced(x0.to(DEV)).requires_grad_(True)
        out = torch.ops.nfp_amd.nfp(x, *_ops.cfg_args(cfg), True)[0]
        fv = _variant()
        gx, = torch.autograd.grad(out, x, poison.fenced(go0.to(DEV)))
        torch.cuda.synchronize()
        return dict(out=out.detach(), grad_x=gx, fwd=fv, bwd=_variant())

    res = P.run_fills(case, "nfp_op")
    assert res["fwd"].startswith("fwd_band<") and res["bwd"].startswith("bwd_fast<"), res
    x = x0.double().requires_grad_(True)
    ref = _host_maps64(x, cfg)
    gref, = torch.autograd.grad(ref, x, go0.double())
    assert rel_err(_np(res["out"]), _np(ref)) <= F32 and rel_err(_np(res["grad_x"]), _np(gref)) <= F32


# ---- the harness on the device ------------------------------------------------------------------------------------------------
def test_the_harness_poisons_and_fences_what_the_binding_allocates_on_the_device():
    """What tests/test_poison_host.py shows on CPU tensors, once on the device and through the binding's own call sites: the
    buffers of one forward + backward are served by the harness, named by functional.py's lines, poisoned, 512-aligned as the
    caching allocator's own; a write one element behind `out` (inside the harness's flat buffer) is caught by check()."""
    from neighbour_feature_pooling_amd import functional as Fn
    cfg = _cfg(8, **_same(1, "cosine"))
    x0 = torch.rand(2, 8, 5, 5) + 0.25
    assert torch.empty(5, device=DEV).data_ptr() % P.GUARD == 0
    with P.Poison("nan") as poison:
        x = poison.fenced(x0.to(DEV)).requires_grad_(True)
        probe = Fn._empty_grad_x(x, True)
        assert probe.isnan().all() and probe.data_ptr() % P.GUARD == 0 and probe.is_contiguous(memory_format=torch.channels_last)
        out = Fn.nfp(x, cfg)
        gx, = torch.autograd.grad(out, x, torch.ones_like(out))
        poison.check()
        assert not out.isnan().any() and not gx.isnan().any()
        assert out.data_ptr() % P.GUARD == 0 and gx.data_ptr() % P.GUARD == 0 and type(out) is torch.Tensor
        sites = [b.site for b in poison.buffers if b.what != "fenced"]
        assert poison.served >= 4 and len(sites) >= 4 and all(s.startswith("functional.py:") for s in sites), sites
        torch.as_strided(out.detach(), (1,), (1,), out.storage_offset() + out.numel()).fill_(1.0)
        with pytest.raises(AssertionError, match=r"empty buffer of functional.py:\d+ .*first at offset %d, last at %d"
                           % (out.numel() * 4, out.numel() * 4 + 3)):
            poison.check()
    assert Fn.torch is torch


# ---- SimilarityAwarePooling's softmax-pool tail (nfp_attpool.hip) -----------------------------------------------------------
@pytest.mark.parametrize("want", [0, 1, 2], ids=["want_maps", "want_w", "want_b"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B,N,Pn", [(1, 8, 1), (2, 8, 25)], ids=["1x8x1", "2x8x25"])
def test_attention_pool_tail(B, N, Pn, dt, want):
    """Each gradient asked for alone: the other two are NULL in the library, neither computed nor written."""
    from neighbour_feature_pooling_amd import nfp_attention_pool
    from neighbour_feature_pooling_amd._host import attention_pool_host
    bf = dt == "bf16"
    g = torch.Generator().manual_seed(_seed("sap%d%d%d" % (B, N, Pn)))
    ins0 = [torch.randn(B, N, Pn, generator=g).to(torch.bfloat16 if bf else torch.float32), torch.randn(N, generator=g) * 0.5,
            torch.randn(1, generator=g)]
    gp0 = torch.randn(B, N, generator=g).to(ins0[0].dtype)

    def case(poison):
        ins = [poison.fenced(t.to(DEV)).requires_grad_(i == want) for i, t in enumerate(ins0)]
        pooled = nfp_attention_pool(*ins)
        fv = _variant()
        grad, = torch.autograd.grad(pooled, ins[want], poison.fenced(gp0.to(DEV)))
        torch.cuda.synchronize()
        return dict(pooled=pooled.detach(), grad=grad, fwd=fv, bwd=_variant())

    res = P.run_fills(case, "attpool")
    assert res["fwd"] == "attpool_fwd<%s>" % dt and res["bwd"] == "attpool_bwd<%s>" % dt, res
    ref_in = [t.double().requires_grad_(True) for t in ins0]
    ref = attention_pool_host(*ref_in)
    rg = torch.autograd.grad(ref, ref_in, gp0.double())
    tol_out, tol_g = (BF_OUT, BF_GRAD) if bf else (F32, F32)       # tests/test_gpu_sap.py::_check
    assert rel_err(_np(res["pooled"]), _np(ref)) <= tol_out
    if want == 2:       # (the softmax does not see the bias: the reference is 0, held to grad_w's scale as _check holds it)
        assert float(np.abs(_np(res["grad"])).max()) <= tol_g * float(np.abs(_np(rg[1])).max())
    else:
        assert rel_err(_np(res["grad"]), _np(rg[want])) <= tol_g


# ---- the compress-BN family: rows of scripts/cp_bits.py::cases(), train and eval, the three `want` masks of its run_case ---
def _cp_rows():
    """(kind, B, N, P, D, bf16, relu, nhwc, out at 2 mod 4) of the chosen rows, the mode dropped: each runs in both."""
    rows = []
    for c in CB.cases():
        _, kind, B, N, Pn, D, bf16, train, relu, nhwc, odd = c
        if ((kind == "pool" and Pn == 35) or (kind == "proj" and Pn in (35, 49)) or (kind == "wide" and N in (33, 96) and Pn == 49)):
            row = (kind, B, N, Pn, D, bf16, relu, nhwc, odd)
            if row not in rows:
                rows.append(row)
    return rows


CP_ROWS = _cp_rows()
CP_MASKS = (("", (True, True, True, True)), ("maps_only.", (True, False, False, False)), ("params_only.", (False, True, True, True)))
CP_FWD = {"pool": "cpool_fwd<", "wide": "cpool_wide_fwd<", "proj": "cproj_fwd<"}
CP_BWD = {"pool": "cpool_bwd<", "wide": "cpool_wide_bwd<", "proj": "cproj_bwd<"}


def _cp_id(row):
    kind, B, N, Pn, D, bf16, relu, nhwc, odd = row
    return "%s_B%d_N%d_P%d_D%d_%s_%s_%s%s" % (kind, B, N, Pn, D, "bf16" if bf16 else "f32", "relu" if relu else "lin",
                                               "nhwc" if nhwc else "nchw", "_odd" if odd else "")


def _cp_modules():
    return P.binding_modules() + [CB]       # (shifted_out allocates the odd-start result itself: poisoned and fenced too)


# The seed of every row: the first (searched on the CPU from 0, as tests/test_gpu_cpool.py searches its own) for which the
# float64 reference of a row with a ReLU has min|a| >= 1e-5 max|a| in training and in eval (bf16 rows: on the rounded maps) —
# 0 unless listed; the staged cases likewise, in training on the whole batch.
CP_SEEDS = {"pool_B1_N17_P35_D67_f32_relu_nchw": 1, "proj_B1_N12_P49_D67_f32_relu_nhwc": 2, "wide_B2_N33_P49_D70_f32_relu_nchw": 1,
            "wide_B2_N96_P49_D70_f32_relu_nchw": 1}
SYNC_SEEDS = {"sync_pool_empty": 3, "sync_pool_bf16": 1, "sync_pool_chunked": 1, "sync_proj_relu_chunked": 1618,
              "sync_proj_relu_nhwc_bf16_odd": 2}


def _cp_reference_check(res, ref, relu, bf16, extra=()):
    """Against the float64 composition at the bars of tests/test_gpu_cpool.py / test_gpu_cproj.py, under the precondition
    those files assert on their references: with a ReLU no pre-activation lies within 1e-5 of max|a| of zero (a sign that
    differs between float32 and float64 changes a gradient by a whole term)."""
    assert not relu or ref["guard"] >= KP.GUARD, ref["guard"]
    bars = dict(out=KP.BF_OUT, gm=KP.BF_GRAD, gw=KP.BF_GRAD, gg=KP.BF_GRAD, gb=KP.BF_GRAD) if bf16 else \
        dict(out=KP.F32, gm=KP.F32, gw=KP.F32_GW, gg=KP.F32, gb=KP.F32)
    errs = {k: rel_err(_np(res[k]).reshape(-1), _np(ref[k]).reshape(-1)) for k in tuple(bars) + tuple(extra)}
    print(errs)
    for k, e in errs.items():
        assert e <= bars.get(k, KP.F32), (k, e)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("row", CP_ROWS, ids=[_cp_id(r) for r in CP_ROWS])
def test_compress_bn_family(row, train):
    from neighbour_feature_pooling_amd import compress as C
    kind, B, N, Pn, D, bf16, relu, nhwc, odd = row
    assert len(CP_ROWS) == 24
    ins0 = CB.inputs(CP_SEEDS.get(_cp_id(row), 0), kind, B, N, Pn, D)

    def case(poison):
        maps, w, gamma, beta, rm, rv, go = (poison.fenced(t) for t in CB.on_device(ins0, kind, bf16, nhwc, torch.device(DEV)))
        with CB.shifted_out(C, odd):
            out, saved = C._cp_forward_call(kind, maps, w, gamma, beta, rm, rv, train, CB.MOM, CB.EPS, relu, nhwc)
        assert not odd or out.data_ptr() % 4 == 2
        res = dict(out=out, rm=rm, rv=rv, fwd=_variant(), out_strides=str(out.stride()))
        for tag, want in CP_MASKS:
            grads = C._cp_backward_call(kind, maps, w, gamma, beta, rm, rv, saved, train, CB.EPS, go, want, relu)
            assert [t is not None for t in grads] == list(want)
            res.update({tag + k: t for k, t in zip(("gm", "gw", "gg", "gb"), grads)})
            res[tag + "bwd"] = _variant()
        torch.cuda.synchronize()
        return res

    res = P.run_fills(case, _cp_id(row), modules=_cp_modules())
    assert res["fwd"].startswith(CP_FWD[kind]) and all(res[tag + "bwd"].startswith(CP_BWD[kind]) for tag, _ in CP_MASKS), res
    for k in ("gm", "gw", "gg", "gb"):       # a gradient does not depend on which others were asked for
        other = res[("maps_only." if k == "gm" else "params_only.") + k]
        assert P.raw(other) == P.raw(res[k]), k
    w4 = ins0[1].reshape(D, N, 1, 1)
    ref_ins = (ins0[0], w4) + tuple(ins0[2:])
    dt = torch.bfloat16 if bf16 else torch.float32
    ref = KJ.reference64(ref_ins, train, relu, dt) if kind == "proj" else KP.reference64(ref_ins, train, dt)
    ref["gw"] = ref["gw"].reshape(D, N)
    _cp_reference_check(res, ref, relu or kind != "proj", bf16, ("rm", "rv") if train else ())


@pytest.mark.parametrize("case", CB.SYNC_CASES, ids=[c[0] for c in CB.SYNC_CASES])
def test_compress_bn_family_across_emulated_ranks(case):
    """The staged calls shard by shard, as scripts/cp_bits.py::run_sync drives them: no process group.  A rank without an
    image (sync_pool_empty and three more) still writes its whole record and its whole row of k, Q."""
    from neighbour_feature_pooling_amd import compress as C
    name, shards, kind, N, Pn, D, bf16, relu, nhwc = case[:9]
    odd = len(case) > 9 and case[9]
    ins0 = CB.inputs(SYNC_SEEDS.get(name, 0), kind, sum(shards), N, Pn, D)
    world = range(len(shards))

    def run(poison):
        maps, w, gamma, beta, rm, rv, go = CB.on_device(ins0, kind, bf16, False, torch.device(DEV))
        w, gamma, beta = (poison.fenced(t) for t in (w, gamma, beta))
        ms = [poison.fenced(m.contiguous()) for m in torch.split(maps, shards)]
        gos = [poison.fenced(g.contiguous(memory_format=torch.channels_last) if nhwc else g.contiguous())
               for g in torch.split(go, shards)]
        recs = [C.cp_sync_moments_call(m) for m in ms]
        records = poison.fenced(torch.cat([r[None] for r in recs]))
        res = {"rank%d.record" % r: recs[r] for r in world}
        saved, parts = [], []
        for r, m in enumerate(ms):
            rm_r, rv_r = poison.fenced(rm), poison.fenced(rv)
            with CB.shifted_out(C, odd):
                out, sv = C.cp_sync_forward_call(kind, m, w, gamma, beta, rm_r, rv_r, CB.MOM, CB.EPS, records, relu, nhwc)
            assert not odd or not out.numel() or out.data_ptr() % 4 == 2
            saved.append(sv)
            res.update({"rank%d.out" % r: out, "rank%d.rm" % r: rm_r, "rank%d.rv" % r: rv_r})
        res["fwd"] = _variant()
        for r, m in enumerate(ms):
            parts.append(C.cp_sync_reduce_call(kind, m, w, gamma, beta, saved[r], CB.EPS, gos[r], (True, True, True), relu))
            res.update({"rank%d.%s" % (r, k): t for k, t in zip(("gw", "gg", "gb", "kq_row"), parts[r])})
        rows = poison.fenced(torch.cat([p[3][None] for p in parts]))
        for r, m in enumerate(ms):
            res["rank%d.gm" % r] = C.cp_sync_maps_call(kind, m, w, gamma, beta, saved[r], CB.EPS, gos[r], rows, relu)
        torch.cuda.synchronize()
        res["bwd"] = _variant()
        return res

    res = P.run_fills(run, name, modules=_cp_modules())
    assert res["fwd"].startswith("cpsync_") and res["bwd"].startswith("cpsync_"), (res["fwd"], res["bwd"])
    for r, b in enumerate(shards):
        if b == 0:      # its zero record and zero row, every element written
            assert not res["rank%d.record" % r].any() and not res["rank%d.kq_row" % r].any()
            assert res["rank%d.record" % r].numel() == 1 + N + N * N and res["rank%d.kq_row" % r].numel() == N + N * N
    dt = torch.bfloat16 if bf16 else torch.float32
    ref_ins = (ins0[0], ins0[1].reshape(D, N, 1, 1)) + tuple(ins0[2:])
    ref = KJ.reference64(ref_ins, True, relu, dt) if kind == "proj" else KP.reference64(ref_ins, True, dt)
    ref["gw"] = ref["gw"].reshape(D, N)
    got = dict(out=torch.cat([res["rank%d.out" % r] for r in world]), gm=torch.cat([res["rank%d.gm" % r] for r in world]),
               gw=sum(res["rank%d.gw" % r] for r in world), gg=sum(res["rank%d.gg" % r] for r in world),
               gb=sum(res["rank%d.gb" % r] for r in world), rm=res["rank0.rm"], rv=res["rank0.rv"])
    for r in world:
        assert P.raw(res["rank%d.rm" % r]) == P.raw(res["rank0.rm"]) and P.raw(res["rank%d.rv" % r]) == P.raw(res["rank0.rv"])
    _cp_reference_check(got, ref, relu or kind != "proj", bf16, ("rm", "rv"))
