"""The native torch.autocast call on the GPU (nfp_desc.map_f32): a bf16 feature map in, float32 NFP maps out, a bf16
grad_x back — no float32 copy of x, no cast of the gradient.

Inputs: x bf16-rounded, grad_out float32 (not rounded).  Referee: the oracle on the same values.  Bars: the maps within
TOL of the tensor's magnitude (float32 arithmetic on exactly representable inputs — tests/test_gpu_parity.py's bar for
float32), grad_x within 2e-2 (the suite's bar for a bf16-rounded gradient).  A tighter second check on grad_x: against
the same build's NFP_AMP_UPCAST=1 result — both are round-to-nearest bf16 of float32 values that agree to 1e-5 of the
tensor's magnitude, so they differ by at most one bf16 spacing at the top of the range, 2^-7 max|ref|, plus that 1e-5.

The per-element bar (tests/one_rounding.py): in this mode grad_x is ONE round-to-nearest bf16 of a float32 value computed
from exactly representable inputs and a float32 `out` — within 2^-8 of each element plus the float32 bar the same kernel
family is held to in float32 storage (`slack`: TOL for the fixed hot-path cases, 2 TOL for the any-geometry gradients as in
test_gather_backward_geometry_sweep, 2e-5 inside scripts/stress_mixed.py).  A conversion by truncation or a 2 % error in
one tap's weight pass the two bars above and fail this one (tests/test_one_rounding.py)."""
import random
import re

import numpy as np
import pytest
import torch

from conftest import nfp_switch, rel_err
from neighbour_feature_pooling_amd import NFPPooling, _abi
from neighbour_feature_pooling_amd import functional as F
from neighbour_feature_pooling_amd._host import nfp_host
from neighbour_feature_pooling_amd.synth import feature_map
from one_rounding import one_rounding_excess
from test_gpu_parity import TOL, _load_script

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _native_call_on(monkeypatch):
    """The native call is opt-in (functional._autocast_native: NFP_AMP_NATIVE=1, read at call time)."""
    monkeypatch.setenv("NFP_AMP_NATIVE", "1")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bf16_round(a):
    return torch.from_numpy(a).bfloat16().float().numpy()


def _k3(measure, **kw):
    return dict(R=1, measure=measure, padding=1, **({"p": 2} if measure == "norm" else {}), **kw)


def _k5(measure, **kw):
    return dict(R=2, measure=measure, padding=2, **({"p": 2} if measure == "norm" else {}), **kw)


#        shape, ctor kwargs of a measure, kernel family
SHAPES = [((3, 8, 5, 7), lambda m: _k3(m, padding_mode="reflect"), "table"),
          ((2, 16, 6, 6), lambda m: _k5(m, padding_mode="zeros"), "table"),
          ((300, 8, 4, 4), _k3, "table"),                                    # one band per image
          ((2, 8, 16, 32), _k3, "table"),                                    # 512 pixels
          # N P / 4 = 2904 pair pieces on at most 512 threads: several pair rounds in bwd_fast.  (Cosine keeps two values per
          # pair: its 400 bytes of LDS per pixel hold k = 5 maps of up to 409 pixels — at 484 the backward is the row-band
          # kernel's, as for every storage type; 16 x 16 is the cosine case of several rounds.)
          ((2, 8, 22, 22), _k5, "table/k5"),
          ((2, 8, 16, 16), _k5, "table"),
          ((2, 8, 24, 23), _k3, "band"),
          ((1, 8, 25, 24), lambda m: _k5(m, padding_mode="replicate"), "band"),
          ((2, 40, 24, 24), _k3, "band"),
          ((2, 64, 24, 24), _k3, "band"),                                    # channels-last: the bf16 LDS-DMA class
          ((1, 128, 24, 24), _k3, "band"),                                   # channels-last: dense-store backward
          ((2, 8, 9, 9), lambda m: dict(_k3(m), padding=0), "general"),
          ((2, 8, 9, 9), lambda m: _k3(m, stride=2), "general"),
          ((2, 8, 9, 9), lambda m: _k3(m, padding_mode="circular"), "general")]
CASES = [(s, f(m), fam) for s, f, fam in SHAPES for m in ("cosine", "norm")]
CASES += [((2, 6, 7, 7), _k3("canberra"), "general"), ((2, 8, 7, 7), dict(R=1, measure="norm", p=1, padding=1), "general")]
RIDERS = [(s, f(m), fam) for m in ("dot", "gfc", "rmse")
          for s, f, fam in (((2, 16, 6, 6), _k3, "table"), ((2, 8, 24, 23), _k3, "band"))]
_REF = {}


def _reference(oracle, shape, kw):
    """(x bf16-rounded, grad_out float32, ref maps, ref grad_x) — computed once per case, never modified."""
    key = (shape, tuple(sorted(kw.items())))
    if key not in _REF:
        x = _bf16_round(feature_map(shape, 31))
        ref = oracle.forward(x, **kw)
        go = feature_map(ref.shape, 32)
        _REF[key] = (x, go, ref, oracle.backward(x, go, **kw))
        for a in _REF[key]:
            a.setflags(write=False)
    return _REF[key]


def _as_layout(xh, layout, dev):
    B, C, H, W = xh.shape
    xt = torch.tensor(xh).to(dev, torch.bfloat16)
    if layout == "nhwc":
        return xt.contiguous(memory_format=torch.channels_last)
    if layout == "tokens":      # [B, 1 + HW, C] tokens behind a class token, viewed as [B,C,H,W]
        buf = torch.zeros(B, 1 + H * W, C, device=dev, dtype=torch.bfloat16)
        buf[:, 1:] = xt.flatten(2).transpose(1, 2)
        return buf[:, 1:].transpose(1, 2).unflatten(2, (H, W))
    return xt


def _run(layer, x, go):
    """(maps, grad_x, forward variant, backward variant, launches) of one fwd + bwd under torch.autocast."""
    L = _abi.load()
    x = x.detach().requires_grad_(True)
    n0 = L.nfp_launch_count()
    with torch.autocast("cuda", torch.bfloat16):
        out = layer(x)
    fwd = L.nfp_last_variant().decode()
    (out * go).sum().backward()
    bwd = L.nfp_last_variant().decode()
    return out.detach(), x.grad, fwd, bwd, L.nfp_launch_count() - n0


def _check_variants(fwd, bwd, family, layout):
    lay = "nchw" if layout == "nchw" else "nhwc"
    if family == "table/k5":    # (see SHAPES)
        assert re.match(rf"fwd_band<R2,\w+,mix,{lay}>x\d+$", fwd), fwd
        assert re.match(rf"bwd_fast<R2,l2,mix,{lay}>$|bwd_tile<R2,cos,mix,{lay}>x\d+$", bwd), bwd
    elif family == "table":
        assert re.match(rf"fwd_band<R\d,\w+,mix,{lay}>x\d+$", fwd), fwd
        assert re.match(rf"bwd_fast<R\d,\w+,mix,{lay}>$", bwd), bwd
    elif family == "band":
        assert re.match(rf"fwd_tile<R\d,\w+,mix,{lay}>x\d+$", fwd), fwd
        assert re.match(rf"bwd_tile<R\d,\w+,mix,{lay}(,dense)?>x\d+$", bwd), bwd
    else:
        assert fwd == "fwd_pairs" and bwd == "bwd_gather", (fwd, bwd)


@pytest.mark.parametrize("layout", ["nchw", "nhwc", "tokens"])
@pytest.mark.parametrize("shape,kw,family", CASES + RIDERS)
def test_maps_and_gradient_against_the_oracle_and_the_upcast(shape, kw, family, layout, dev, oracle_lib, monkeypatch):
    xh, goh, ref, ref_gx = _reference(oracle_lib, shape, kw)
    layer = NFPPooling(shape[1], **kw)
    go = torch.tensor(goh).to(dev)
    out, gx, fwd, bwd, launches = _run(layer, _as_layout(xh, layout, dev), go)
    assert out.dtype == torch.float32 and gx.dtype == torch.bfloat16 and gx.shape == tuple(shape)
    _check_variants(fwd, bwd, family, layout)
    if shape == (1, 128, 24, 24) and layout != "nchw":
        assert ",dense>" in bwd, bwd
    assert launches == 2
    monkeypatch.setenv("NFP_AMP_UPCAST", "1")       # (read at call time)
    out_u, gx_u, fwd_u, bwd_u, _ = _run(layer, _as_layout(xh, layout, dev), go)
    assert "mix" not in fwd_u and "mix" not in bwd_u and out_u.dtype == torch.float32 and gx_u.dtype == torch.bfloat16
    e_map = rel_err(out.cpu().numpy(), ref)
    e_gx = rel_err(gx.float().cpu().numpy(), ref_gx)
    top = float(np.abs(ref_gx).max())
    d_up = float((gx.float() - gx_u.float()).abs().max())
    excess = one_rounding_excess(gx.float().cpu().numpy(), ref_gx, TOL)
    print(f"{shape} {kw['measure']} {layout}: maps {e_map:.2e} grad_x {e_gx:.2e} ({excess:.3f} of the one-rounding bar) "
          f"vs upcast {d_up:.3e} (bound {2.0 ** -7 * top + 1e-5 * top:.3e}) [{fwd} | {bwd}]")
    assert e_map <= TOL
    assert e_gx <= 2e-2
    assert d_up <= 2.0 ** -7 * top + 1e-5 * top
    assert excess <= 1.0


_DENSE = CASES[20]       # (1, 128, 24, 24) cosine: channels-last it takes the dense-store backward


@pytest.mark.parametrize("shape,kw,family", [CASES[0], CASES[9], CASES[13], CASES[23], _DENSE])
def test_two_runs_are_bitwise_equal(shape, kw, family, dev):
    xh = _bf16_round(feature_map(shape, 41))
    layer = NFPPooling(shape[1], **kw)
    layout = "nhwc" if (shape, kw) == _DENSE[:2] else "nchw"
    runs = []
    for _ in range(2):
        x = _as_layout(xh, layout, dev)
        go = torch.tensor(feature_map((shape[0], layer.config.out_channels) + _hw(shape, kw), 42)).to(dev)
        out, gx, fwd, bwd, _ = _run(layer, x, go)
        runs.append((out.clone(), gx.clone()))
    _check_variants(fwd, bwd, family, layout)
    assert (",dense>" in bwd) == (layout == "nhwc"), bwd
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _hw(shape, kw):
    k, s, p = 2 * kw["R"] + 1, kw.get("stride", 1), kw["padding"]
    return ((shape[2] + 2 * p - k) // s + 1, (shape[3] + 2 * p - k) // s + 1)


def test_module_takes_the_native_call_for_bf16_only(dev, monkeypatch):
    """NFPPooling under torch.autocast: `mix` variants for a bf16 x; the float32 kernels for a float32 or float16 x (the
    upcast) and with NFP_AMP_UPCAST=1; outside autocast a bf16 x keeps its bf16 maps."""
    L = _abi.load()
    layer = NFPPooling(16, R=1, measure="cosine", padding=1)
    x32 = torch.tensor(feature_map((2, 16, 6, 6), 51)).to(dev)

    def variants(x, autocast=True):
        x = x.detach().requires_grad_(True)
        with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
            out = layer(x)
        fwd = L.nfp_last_variant().decode()
        out.float().sum().backward()
        return out.dtype, x.grad.dtype, fwd, L.nfp_last_variant().decode()

    odt, gdt, fwd, bwd = variants(x32.bfloat16())
    assert (odt, gdt) == (torch.float32, torch.bfloat16)
    assert fwd.startswith("fwd_band<R1,cos,mix,nchw>x") and bwd == "bwd_fast<R1,cos,mix,nchw>"
    for xdt in (torch.float32, torch.float16):
        odt, gdt, fwd, bwd = variants(x32.to(xdt))
        assert (odt, gdt) == (torch.float32, xdt) and ",f32," in fwd and ",f32," in bwd
    odt, gdt, fwd, bwd = variants(x32.bfloat16(), autocast=False)
    assert (odt, gdt) == (torch.bfloat16, torch.bfloat16) and ",bf16," in fwd and ",bf16," in bwd
    monkeypatch.setenv("NFP_AMP_UPCAST", "1")
    odt, gdt, fwd, bwd = variants(x32.bfloat16())
    assert (odt, gdt) == (torch.float32, torch.bfloat16) and ",f32," in fwd and ",f32," in bwd
    monkeypatch.delenv("NFP_AMP_UPCAST")
    monkeypatch.delenv("NFP_AMP_NATIVE")            # without the opt-in: the upcast, as before
    odt, gdt, fwd, bwd = variants(x32.bfloat16())
    assert (odt, gdt) == (torch.float32, torch.bfloat16) and ",f32," in fwd and ",f32," in bwd
    monkeypatch.setenv("NFP_AMP_NATIVE", "1")
    # Attention keeps the upcast (the library refuses map_f32 there), and no_grad launches the forward alone
    att = NFPPooling(16, R=1, measure="attention", padding=1)
    with torch.autocast("cuda", torch.bfloat16):
        out = att(x32.bfloat16())
    assert out.dtype == torch.float32 and "mix" not in L.nfp_last_variant().decode()
    n0 = L.nfp_launch_count()
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        out = layer(x32.bfloat16())
    assert out.dtype == torch.float32 and L.nfp_launch_count() == n0 + 1 and ",mix," in L.nfp_last_variant().decode()


# ---- random draws: scripts/stress_mixed.py ----------------------------------------------------------------------------------
def _stress(family, seed, dev):
    """24 draws of scripts/stress_mixed.py (the long form: python scripts/stress_mixed.py 200).  The seeds are ones whose 24
    descriptors nfp_plan (host only) puts on the family's kernels; a case the library does not run natively fails."""
    sm = _load_script("stress_mixed")
    rnd = random.Random(seed)
    seen = []
    for _ in range(24):
        ok, desc, errs, vs = sm.one_case(rnd, dev, family)
        print(f"{desc}: maps {errs[0]:.2e} grad_x {errs[1]:.3f} of the one-rounding bar, {errs[2]:.3f} of the upcast bound {vs}")
        assert ok, (desc, errs, vs)
        seen.append(vs)
        torch.cuda.empty_cache()
    return seen


def test_random_stress_of_the_table_kernels(dev):
    """Maps of 4 to 512 pixels, k = 3 and 5, C up to 64 and 512, batches up to 300, the five hot measures, three padding
    modes, normal / relu (with all-zero pixels) / smooth inputs, NCHW / channels-last / token views, both signs of
    `similarity` — maps and the one-rounding bar on grad_x against the float64 formulation, and the upcast."""
    for fwd, bwd in _stress("table", 5151, dev):
        assert re.match(r"fwd_band<R\d,\w+,mix,\w+>x\d+$", fwd) and re.match(r"bwd_fast<R\d,\w+,mix,\w+>$", bwd), (fwd, bwd)


def test_random_stress_of_the_row_band_kernels(dev):
    """Maps of 513 to about 2400 pixels: fwd_tile / bwd_tile, the dense-store backward among them."""
    seen = _stress("band", 5152, dev)
    for fwd, bwd in seen:
        assert re.match(r"fwd_tile<R\d,\w+,mix,\w+>x\d+$", fwd), fwd
        assert re.match(r"bwd_tile<R\d,\w+,mix,\w+(,dense)?>x\d+$", bwd), bwd
    assert any(",dense>" in bwd for _, bwd in seen), seen


def test_random_stress_of_the_any_geometry_kernels(dev):
    """Stride, dilation, pad != R, circular padding, C % 4 != 0 and the measures without a hot kernel: a float32 `out`
    beside a bf16 x in fwd_pairs / bwd_gather."""
    seen = _stress("general", 5153, dev)
    assert ("fwd_pairs", "bwd_gather") in seen, seen


# ---- every measure on every any-geometry implementation -------------------------------------------------------------------
MEASURES = ["norm", "cosine", "dot", "rmse", "geman", "emd", "canberra", "hellinger", "chisquared1", "chisquared2", "gfc",
            "pearson", "jeffrey", "squaredchord", "smith"]      # every measure map_f32 takes: all but Attention and SCS
GEOMETRIES = [((3, 6, 7, 9), dict(R=1, padding=1, padding_mode="reflect")),
              ((2, 5, 11, 10), dict(R=1, padding=2, stride=3, dilation=2, padding_mode="zeros"))]


def _positive_case(shape, ctor, seed):
    """(layer, x on the bf16 grid in [0.25, 1.25) — valid for every measure —, float32 grad_out, float64 maps, float64 grad_x)."""
    layer = NFPPooling(shape[1], **ctor)
    g = torch.Generator().manual_seed(seed)
    xh = (torch.rand(*shape, generator=g) + 0.25).bfloat16().float()
    x64 = xh.double().requires_grad_(True)
    ref = nfp_host(x64, layer.config)
    goh = torch.randn(ref.shape, generator=g)
    gref, = torch.autograd.grad(ref, x64, goh.double())
    return layer, xh, goh, ref.detach().numpy(), gref.numpy()


@pytest.mark.parametrize("shape,geo", GEOMETRIES)
@pytest.mark.parametrize("measure", MEASURES)
def test_every_measure_on_every_any_geometry_kernel(measure, shape, geo, dev, monkeypatch):
    """fwd_pairs + bwd_gather, bwd_gather_banded / bwd_direct (NFP_BWD_BANDS=3), then fwd_direct + bwd_direct
    (NFP_FWD_SCALAR=1, NFP_BWD_ATOMIC=1) — the switches of test_gather_backward_geometry_sweep — each reading `out` by
    `odtype`: float32 beside a bf16 x.  Maps at TOL; grad_x at the one-rounding bar over that test's float32 bar, 2 TOL."""
    nfp_switch(monkeypatch, "NFP_FORCE_GENERIC", "1")
    nfp_switch(monkeypatch, "NFP_BWD_ATOMIC", "0")
    nfp_switch(monkeypatch, "NFP_FWD_SCALAR", "0")
    ctor = dict(geo, measure=measure, **({"p": 1} if measure == "norm" else {}))
    layer, xh, goh, ref, gref = _positive_case(shape, ctor, shape[2] * 131 + shape[3] * 17 + shape[1])
    x, go = xh.to(dev, torch.bfloat16), goh.to(dev)

    def check(want_fwd, want_bwd):
        out, gx, fwd, bwd, launches = _run(layer, x, go)
        e_map = rel_err(out.cpu().numpy(), ref)
        excess = one_rounding_excess(gx.float().cpu().numpy(), gref, 2 * TOL)
        print(f"{shape} {measure} [{fwd} | {bwd}]: maps {e_map:.2e} grad_x {excess:.3f} of the one-rounding bar")
        assert out.dtype == torch.float32 and gx.dtype == torch.bfloat16 and launches == 2
        assert fwd == want_fwd and bwd in want_bwd, (fwd, bwd)
        assert e_map <= TOL
        assert excess <= 1.0

    check("fwd_pairs", ("bwd_gather",))
    nfp_switch(monkeypatch, "NFP_BWD_BANDS", "3")
    check("fwd_pairs", ("bwd_gather_banded", "bwd_direct"))
    nfp_switch(monkeypatch, "NFP_BWD_BANDS", None)
    nfp_switch(monkeypatch, "NFP_BWD_ATOMIC", "1")
    nfp_switch(monkeypatch, "NFP_FWD_SCALAR", "1")
    check("fwd_direct", ("bwd_direct",))


def test_a_large_strided_map_takes_the_banded_backward_unforced(dev):
    shape, ctor = (1, 8, 64, 40), dict(R=1, measure="canberra", padding=1, stride=2, padding_mode="zeros")
    layer, xh, goh, ref, gref = _positive_case(shape, ctor, 64 + 40)
    out, gx, fwd, bwd, launches = _run(layer, xh.to(dev, torch.bfloat16), goh.to(dev))
    assert out.dtype == torch.float32 and gx.dtype == torch.bfloat16 and launches == 2
    assert fwd == "fwd_pairs" and bwd == "bwd_gather_banded", (fwd, bwd)
    assert rel_err(out.cpu().numpy(), ref) <= TOL
    assert one_rounding_excess(gx.float().cpu().numpy(), gref, 2 * TOL) <= 1.0


# ---- edge inputs on the hot kernels ------------------------------------------------------------------------------------------
TABLE, BAND = (2, 16, 6, 6), (2, 8, 24, 23)


def _relu_with_zero_pixels(shape, seed):
    x = feature_map(shape, seed, "relu").copy()
    x[-1].reshape(shape[1], -1)[:, 1::3] = 0.0      # every third pixel of the last image: all channels zero
    x[0, :, 0, 0] = 0.0                             # ... and a corner of the first
    return x


def _constant(shape, seed):
    return np.full(shape, 0.625, np.float32)


EDGES = [
    # RMSE of a pixel and its replicated copy is sqrt(0): no subgradient, NaN in the reference — and in the bf16 grad_x
    ("rmse-replicate", (5, 32, 13, 16), "table", _k3("rmse", padding_mode="replicate"), None),
    ("rmse-replicate", BAND, "band", _k3("rmse", padding_mode="replicate"), None),
    # DotProduct keeps no saved norms: its backward reads the (float32) map in their place
    ("dot", TABLE, "table", _k3("dot", padding_mode="zeros"), None),
    ("dot-k5", TABLE, "table", _k5("dot"), None),
    ("dot", BAND, "band", _k3("dot", padding_mode="zeros"), None),
    ("cosine-zero-pixels", TABLE, "table", _k3("cosine", padding_mode="zeros"), _relu_with_zero_pixels),
    ("cosine-zero-pixels", BAND, "band", _k3("cosine", padding_mode="zeros"), _relu_with_zero_pixels),
    ("cosine-eps", TABLE, "table", _k3("cosine", eps=1e-2), _relu_with_zero_pixels),
    ("cosine-eps", BAND, "band", _k3("cosine", eps=1e-2), _relu_with_zero_pixels),
    # every distance exactly 0: the L2 gradient there is 0, not NaN
    ("l2-constant", TABLE, "table", _k3("norm", padding_mode="replicate"), _constant),
    ("l2-constant", BAND, "band", _k3("norm", padding_mode="replicate"), _constant),
    ("dissimilarity", TABLE, "table", _k3("cosine", similarity=False), None),
    ("dissimilarity", TABLE, "table", _k5("norm", similarity=False), None),
    ("dissimilarity", BAND, "band", _k3("cosine", similarity=False), None),
    ("dissimilarity", BAND, "band", _k3("norm", similarity=False), None),
    # the channel chunking of both table kernels, and one workgroup per image
    ("chunks", (3, 512, 7, 7), "table", _k3("cosine"), None),
    ("chunks", (3, 512, 7, 7), "table", _k5("norm"), None),
    ("per-image", (260, 64, 7, 7), "table", _k3("cosine"), None),
    ("per-image", (260, 64, 7, 7), "table", _k3("norm"), None),
]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("name,shape,family,kw,make", EDGES, ids=[f"{e[0]}-{e[2]}-{e[3]['measure']}-R{e[3]['R']}" for e in EDGES])
def test_edge_inputs_on_the_hot_kernels(name, shape, family, kw, make, layout, dev):
    """Against the float64 formulation on the same bf16-rounded x: maps at TOL, NaN patterns equal, grad_x within one
    rounding per element (slack TOL)."""
    layer = NFPPooling(shape[1], **kw)
    xh = _bf16_round(make(shape, 61) if make else feature_map(shape, 61))
    x64 = torch.from_numpy(xh).double().requires_grad_(True)
    ref = nfp_host(x64, layer.config)
    goh = feature_map(tuple(ref.shape), 62)
    gref, = torch.autograd.grad(ref, x64, torch.from_numpy(goh).double())
    ref, gref = ref.detach().numpy(), gref.numpy()
    out, gx, fwd, bwd, launches = _run(layer, _as_layout(xh, layout, dev), torch.from_numpy(goh).to(dev))
    assert out.dtype == torch.float32 and gx.dtype == torch.bfloat16 and launches == 2
    _check_variants(fwd, bwd, family, layout)
    outh, gxh = out.cpu().numpy(), gx.float().cpu().numpy()
    assert not np.isnan(ref).any() and not np.isnan(outh).any()
    e_map = rel_err(outh, ref) if np.abs(ref).max() > 0 else float(np.abs(outh).max())
    excess = one_rounding_excess(gxh, gref, TOL)
    print(f"{name} {shape} {layout}: maps {e_map:.2e} grad_x {excess:.3f} of the one-rounding bar, "
          f"{int(np.isnan(gref).sum())} NaN [{fwd} | {bwd}]")
    if name == "rmse-replicate":
        assert np.isnan(gref).any() and np.array_equal(np.isnan(gxh), np.isnan(gref))
    else:
        assert not np.isnan(gref).any() and not np.isnan(gxh).any()
    if name == "l2-constant":
        assert not ref.any() and not outh.any() and not gref.any() and not gxh.any()
    assert e_map <= TOL
    assert excess <= 1.0


@pytest.mark.parametrize("shape,family", [(TABLE, "table"), (BAND, "band")])
def test_a_grad_out_that_is_not_contiguous(shape, family, dev):
    """out.sum().backward() hands the backward an expanded scalar, a channels-last consumer a channels-last grad_out: the
    kernels read a dense float32 grad_out, and the result equals the contiguous call's bit for bit."""
    layer = NFPPooling(shape[1], **_k3("cosine"))
    x = torch.from_numpy(_bf16_round(feature_map(shape, 71))).to(dev, torch.bfloat16).requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16):
        out = layer(x)
    assert out.dtype == torch.float32
    ones, = torch.autograd.grad(out, x, torch.ones_like(out), retain_graph=True)
    bwd = _abi.load().nfp_last_variant().decode()
    assert re.match(r"bwd_fast<R1,cos,mix,nchw>$" if family == "table" else r"bwd_tile<R1,cos,mix,nchw>x\d+$", bwd), bwd
    out.sum().backward(retain_graph=True)
    assert x.grad.dtype == torch.bfloat16 and torch.equal(x.grad, ones)
    go = torch.from_numpy(feature_map(tuple(out.shape), 72)).to(dev)
    dense, = torch.autograd.grad(out, x, go, retain_graph=True)
    go_cl = go.contiguous(memory_format=torch.channels_last)
    assert not go_cl.is_contiguous()
    strided, = torch.autograd.grad(out, x, go_cl)
    assert torch.equal(strided, dense) and not torch.equal(dense, ones)


# ---- the fused callers keep the upcast ------------------------------------------------------------------------------------
def test_fused_callers_are_untouched_by_the_opt_in(dev, monkeypatch):
    """nfp_pool, nfp_pooled, nfp_with_gap and nfp_multi_radius under torch.autocast: bitwise the same results, gradients
    included, with and without NFP_AMP_NATIVE=1 — they run the float32 kernels on a float32 copy either way, and none of them
    reports a `mix` variant."""
    L = _abi.load()
    cfg1 = NFPPooling(16, R=1, measure="cosine", padding=1).config
    cfg2 = NFPPooling(16, R=2, measure="cosine", padding=2).config
    xh = torch.from_numpy(_bf16_round(feature_map((3, 16, 9, 8), 81)))
    calls = [("nfp_pool", lambda x: F.nfp_pool(x, cfg1)), ("nfp_pooled", lambda x: (F.nfp_pooled(x, cfg1),)),
             ("nfp_with_gap", lambda x: F.nfp_with_gap(x, cfg1)), ("nfp_multi_radius", lambda x: (F.nfp_multi_radius(x, cfg1, cfg2),))]

    def arm():
        res = []
        for name, call in calls:
            x = xh.to(dev, torch.bfloat16).requires_grad_(True)
            with torch.autocast("cuda", torch.bfloat16):
                outs = call(x)
            fwd = L.nfp_last_variant().decode()
            loss = sum((o.float() * torch.from_numpy(feature_map(tuple(o.shape), 82 + i)).to(dev)).sum() for i, o in enumerate(outs))
            gx, = torch.autograd.grad(loss, x)
            bwd = L.nfp_last_variant().decode()
            assert "mix" not in fwd and "mix" not in bwd, (name, fwd, bwd)
            assert gx.dtype == torch.bfloat16
            res.append((name, fwd, bwd, [o.detach().clone() for o in outs] + [gx]))
        return res

    with_opt_in = arm()
    monkeypatch.delenv("NFP_AMP_NATIVE")
    without = arm()
    for (name, fwd, bwd, a), (_, fwd0, bwd0, b) in zip(with_opt_in, without):
        assert (fwd, bwd) == (fwd0, bwd0), name
        for u, v in zip(a, b):
            assert u.dtype == v.dtype and torch.equal(u, v), name
