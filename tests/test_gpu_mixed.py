"""The native torch.autocast call on the GPU (nfp_desc.map_f32): a bf16 feature map in, float32 NFP maps out, a bf16
grad_x back — no float32 copy of x, no cast of the gradient.

Inputs: x bf16-rounded, grad_out float32 (not rounded).  Referee: the oracle on the same values.  Bars: the maps within
TOL of the tensor's magnitude (float32 arithmetic on exactly representable inputs — tests/test_gpu_parity.py's bar for
float32), grad_x within 2e-2 (the suite's bar for a bf16-rounded gradient).  A tighter second check on grad_x: against
the same build's NFP_AMP_UPCAST=1 result — both are round-to-nearest bf16 of float32 values that agree to 1e-5 of the
tensor's magnitude, so they differ by at most one bf16 spacing at the top of the range, 2^-7 max|ref|, plus that 1e-5."""
import re

import numpy as np
import pytest
import torch

from conftest import rel_err
from neighbour_feature_pooling_amd import NFPPooling, _abi
from neighbour_feature_pooling_amd.synth import feature_map
from test_gpu_parity import TOL

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
    print(f"{shape} {kw['measure']} {layout}: maps {e_map:.2e} grad_x {e_gx:.2e} vs upcast {d_up:.3e} "
          f"(bound {2.0 ** -7 * top + 1e-5 * top:.3e}) [{fwd} | {bwd}]")
    assert e_map <= TOL
    assert e_gx <= 2e-2
    assert d_up <= 2.0 ** -7 * top + 1e-5 * top


@pytest.mark.parametrize("shape,kw,family", [CASES[0], CASES[9], CASES[13], CASES[23]])
def test_two_runs_are_bitwise_equal(shape, kw, family, dev):
    xh = _bf16_round(feature_map(shape, 41))
    layer = NFPPooling(shape[1], **kw)
    runs = []
    for _ in range(2):
        x = torch.tensor(xh).to(dev, torch.bfloat16)
        go = torch.tensor(feature_map((shape[0], layer.config.out_channels) + _hw(shape, kw), 42)).to(dev)
        out, gx, fwd, bwd, _ = _run(layer, x, go)
        runs.append((out.clone(), gx.clone()))
    _check_variants(fwd, bwd, family, "nchw")
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
