"""nfp_with_gap on the GPU: GAP(x) and the NFP maps from one pass, one backward kernel for both gradients.

Referee: gap against x.double().mean((2, 3)); maps against the oracle forward; grad_x against the oracle backward of
grad_out plus grad_gap[b,c] / (H*W).  Tolerances are those tests/test_gpu_parity.py applies to the kernels these modes
derive from: its TOL for float32, 1e-2 (maps) / 2e-2 (gradients) for bf16 on the same bf16-rounded inputs."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import rel_err
from neighbour_feature_pooling_amd import NFPPooling, NFPWithGap, _abi, nfp_with_gap
from neighbour_feature_pooling_amd.synth import feature_map
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bf16_round(a):
    return torch.from_numpy(a).bfloat16().float().numpy()


def _two_band_height(W=24, R=1):
    """Smallest H (map above the table kernels' 512 pixels) whose forward nfp_plan shows >= 2 row bands."""
    from test_dispatch_plan import desc, plan
    L = _abi.load()
    for H in range(513 // W + 1, 200):
        rc, text = plan(L, desc((1, 8, H, W), R=R), False)
        m = re.match(r"fwd_tile<[^>]*>x(\d+)", text)
        if rc == 0 and m and int(m.group(1)) >= 2:
            return H
    raise AssertionError("no banded height found")


#        shape            ctor kwargs                                                    dtype   family
CASES = [((2, 8, 5, 5), dict(R=1, measure="cosine", padding=1, padding_mode="reflect"), "f32", "table"),
         ((3, 12, 7, 7), dict(R=2, measure="norm", p=2, padding=2, padding_mode="zeros"), "f32", "table"),
         ((2, 32, 6, 6), dict(R=1, measure="cosine", padding=1), "bf16", "table"),
         ((2, 8, 24, 24), dict(R=1, measure="cosine", padding=1), "f32", "band"),
         ((1, 8, 23, 25), dict(R=2, measure="cosine", padding=2, padding_mode="replicate"), "f32", "band"),
         ((1, 8, "H2", 24), dict(R=1, measure="norm", p=2, padding=1), "f32", "band"),
         ((2, 16, 24, 24), dict(R=1, measure="cosine", padding=1), "bf16", "band")]
_REF = {}


def _reference(oracle, shape, kw, bf):
    """(x, grad_gap, grad_out, ref maps, ref grad_x of grad_out alone) — computed once per case, never modified."""
    key = (shape, tuple(sorted(kw.items())), bf)
    if key not in _REF:
        x = feature_map(shape, 11)
        gg = feature_map(shape[:2], 12)
        if bf:
            x = _bf16_round(x)
        ref = oracle.forward(x, **kw)
        go = feature_map(ref.shape, 13)
        if bf:
            go = _bf16_round(go)
        _REF[key] = tuple(a for a in (x, gg, go, ref, oracle.backward(x, go, **kw)))
        for a in _REF[key]:
            a.setflags(write=False)
    return _REF[key]


def _check_variants(L, fwd, bwd, family, bf, layout):
    if family == "table":
        assert re.match(r"(fwd_band|fwd_gram)<.*,gap>", fwd), fwd
        assert re.match(r"bwd_fast<.*,gap>", bwd), bwd
    else:
        assert re.match(r"fwd_tile<.*,gap>x\d+\+pool_fold", fwd), fwd
        assert re.match(r"bwd_tile<.*,gap>x\d+", bwd), bwd
    assert ("nhwc" if layout != "nchw" else "nchw") in fwd and ("nhwc" if layout != "nchw" else "nchw") in bwd


@pytest.mark.parametrize("layout,grads", [("nchw", "both"), ("nchw", "gap"), ("nchw", "maps"), ("nhwc", "both"), ("nhwc", "gap"),
                                          ("nhwc", "maps"), ("tokens", "both")])
@pytest.mark.parametrize("shape,kw,dt,family", CASES)
def test_values_and_gradients_against_the_oracle(shape, kw, dt, family, layout, grads, dev, oracle_lib):
    if shape[2] == "H2":
        shape = (shape[0], shape[1], _two_band_height(shape[3], kw["R"]), shape[3])
    bf = dt == "bf16"
    xh, ggh, goh, ref, ref_gx_maps = _reference(oracle_lib, shape, kw, bf)
    B, C, H, W = shape
    tdt = torch.bfloat16 if bf else torch.float32
    xt = torch.tensor(xh).to(dev, tdt)
    if layout == "nhwc":
        x = xt.contiguous(memory_format=torch.channels_last)
    elif layout == "tokens":    # [B, 1 + HW, C] tokens behind a class token, viewed as [B,C,H,W]: batch stride (1 + HW) C
        buf = torch.zeros(B, 1 + H * W, C, device=dev, dtype=tdt)
        buf[:, 1:] = xt.flatten(2).transpose(1, 2)
        x = buf[:, 1:].transpose(1, 2).unflatten(2, (H, W))
        assert B == 1 or x.stride(0) == (1 + H * W) * C     # (a size-1 batch carries an arbitrary stride)
    else:
        x = xt
    x = x.detach().requires_grad_(True)
    L = _abi.load()
    layer = NFPPooling(C, **kw)
    n0 = L.nfp_launch_count()
    gap, maps = NFPWithGap(layer)(x)
    fwd = L.nfp_last_variant().decode()
    assert gap.dtype == torch.float32 and maps.dtype == tdt
    gg, go = torch.tensor(ggh).to(dev), torch.tensor(goh).to(dev, tdt)
    loss = (gap * gg).sum() + (maps.float() * go.float()).sum()
    if grads == "gap":
        loss = (gap * gg).sum()
    elif grads == "maps":
        loss = (maps.float() * go.float()).sum()
    loss.backward()
    bwd = L.nfp_last_variant().decode()
    _check_variants(L, fwd, bwd, family, bf, layout)
    assert L.nfp_launch_count() - n0 == (2 if family == "table" else 3)      # (+ pool_fold on the row-band kernels)
    e_gap = rel_err(gap.detach().cpu().numpy(), xh.astype(np.float64).mean((2, 3)))
    e_map = rel_err(maps.detach().float().cpu().numpy(), ref)
    ref_gx = (ref_gx_maps.astype(np.float64) if grads != "gap" else 0.0) + \
        (ggh.astype(np.float64)[:, :, None, None] / (H * W) if grads != "maps" else 0.0) + np.zeros(shape)
    e_gx = rel_err(x.grad.float().cpu().numpy(), ref_gx)
    print(f"{shape} {kw['measure']} {dt} {layout} {grads}: gap {e_gap:.2e} maps {e_map:.2e} grad_x {e_gx:.2e} [{fwd} | {bwd}]")
    assert x.grad.shape == x.shape and x.grad.dtype == tdt
    assert e_gap <= TOL
    assert e_map <= (1e-2 if bf else TOL)
    assert e_gx <= (2e-2 if bf else TOL)


@pytest.mark.parametrize("shape,kw,dt,family", [CASES[0], CASES[2], CASES[3]])
def test_two_runs_are_bitwise_equal(shape, kw, dt, family, dev):
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    xh = feature_map(shape, 21)
    runs = []
    for _ in range(2):
        x = torch.from_numpy(xh).to(dev, tdt).requires_grad_(True)
        gap, maps = nfp_with_gap(x, NFPPooling(shape[1], **kw).config)
        ((gap * 0.5).sum() + maps.float().square().sum()).backward()
        runs.append((gap.detach().clone(), maps.detach().clone(), x.grad.clone()))
    assert ",gap>" in _abi.load().nfp_last_variant().decode()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_outputs_used_alone_or_not_at_all(dev):
    """grad_gap = None reaches the library as ggap = NULL; no_grad builds no graph; maps equal nfp's bit for bit."""
    cfg = NFPPooling(8, R=1, measure="cosine", padding=1).config
    from neighbour_feature_pooling_amd import nfp_op
    x = torch.from_numpy(feature_map((2, 8, 5, 5), 31)).to(dev).requires_grad_(True)
    gap, maps = nfp_with_gap(x, cfg)
    maps.sum().backward()               # gap unused: its gradient is None inside the node
    x2 = x.detach().clone().requires_grad_(True)
    m2 = nfp_op(x2, cfg)
    m2.sum().backward()
    assert torch.equal(maps, m2) and torch.allclose(x.grad, x2.grad, rtol=0, atol=1e-6)
    with torch.no_grad():
        g3, m3 = nfp_with_gap(x, cfg)
    assert not g3.requires_grad and not m3.requires_grad and torch.equal(m3, m2) and torch.equal(g3, gap)


def test_short_saved_is_refused_without_a_launch(dev):
    from neighbour_feature_pooling_amd import functional as F
    L = _abi.load()
    cfg = NFPPooling(8, R=1, measure="cosine", padding=1).config
    x = torch.from_numpy(feature_map((2, 8, 24, 24), 41)).to(dev)
    plan = F._plan(x, "nchw", cfg)
    d, oshape = plan.desc, plan.oshape
    need = int(L.nfp_gap_saved_floats(ctypes.byref(d)))
    assert need > 2 * 576
    gap = torch.empty(2, 8, device=dev)
    maps = torch.empty(oshape, device=dev)
    saved = torch.empty(need, device=dev)
    torch.cuda.synchronize()
    n0 = L.nfp_launch_count()
    rc = L.nfp_gap_forward(ctypes.byref(d), x.data_ptr(), gap.data_ptr(), maps.data_ptr(), saved.data_ptr(), need - 1, None)
    assert rc == -1 and L.nfp_launch_count() == n0
    rc = L.nfp_gap_backward(ctypes.byref(d), x.data_ptr(), None, maps.data_ptr(), maps.data_ptr(), saved.data_ptr(),
                            2 * 576 - 1, maps.data_ptr(), None)
    assert rc == -1 and L.nfp_launch_count() == n0


@pytest.mark.parametrize("kw", [dict(R=1, measure="canberra", padding=1), dict(R=1, measure="cosine", padding=0),
                                dict(R=1, measure="cosine", padding=1, bias=True)])
def test_unsupported_calls_are_the_composition(kw, dev):
    torch.manual_seed(5)
    layer = NFPPooling(8, **kw).to(dev)
    x = torch.from_numpy(feature_map((2, 8, 6, 6), 51)).to(dev).requires_grad_(True)
    L = _abi.load()
    gap, maps = NFPWithGap(layer)(x)
    assert ",gap>" not in L.nfp_last_variant().decode()
    (gap.sum() + maps.square().sum()).backward()
    assert ",gap>" not in L.nfp_last_variant().decode()
    x2 = x.detach().clone().requires_grad_(True)
    gap2, maps2 = x2.mean((2, 3)).float(), layer(x2)
    (gap2.sum() + maps2.square().sum()).backward()
    assert torch.equal(gap, gap2) and torch.equal(maps, maps2) and torch.allclose(x.grad, x2.grad, rtol=0, atol=1e-6)


@pytest.mark.parametrize("measure", ["cosine", "canberra"])
def test_compiled_fullgraph_equals_eager(measure, dev):
    layer = NFPWithGap(NFPPooling(8, R=1, measure=measure, padding=1))
    w = torch.from_numpy(feature_map((2, 8, 5, 5), 62)).to(dev)

    def f(x):
        gap, maps = layer(x)
        return (gap * 0.25).sum() + (maps * w).sum()

    xh = feature_map((2, 8, 5, 5), 61)
    x = torch.from_numpy(xh).to(dev).requires_grad_(True)
    f(x).backward()
    L = _abi.load()
    xc = torch.from_numpy(xh).to(dev).requires_grad_(True)
    yc = torch.compile(f, fullgraph=True, backend="aot_eager")(xc)
    yc.backward()
    assert (",gap>" in L.nfp_last_variant().decode()) == (measure == "cosine")
    assert torch.allclose(yc, f(x.detach()), rtol=1e-6, atol=1e-6) and torch.allclose(xc.grad, x.grad, rtol=0, atol=1e-6)


def test_head_net_train_step(dev):
    from neighbour_feature_pooling_amd.models import NFPHeadNet
    torch.manual_seed(0)
    net = NFPHeadNet("resnet18", num_classes=3, bottleneck_dim=16).to(dev)
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    L = _abi.load()
    seen = []
    loss = torch.nn.functional.cross_entropy(net(torch.randn(4, 3, 128, 128, device=dev)), torch.tensor([0, 2, 1, 1], device=dev))
    seen.append(L.nfp_last_variant().decode())
    loss.backward()
    seen.append(L.nfp_last_variant().decode())
    opt.step()
    assert all(",gap>" in v for v in seen), seen       # [4,512,4,4] -> the table kernels, one pass each way
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
