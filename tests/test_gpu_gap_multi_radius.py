"""nfp_with_gap for radii (1, 2) together on the GPU (MultiRadiusNFPHead: GAP(fmap) beside the 8 + 24 maps, one kernel each
way), and the C++ autograd node of the pair against the Python one.

Referee: the oracle run once per radius, as tests/test_gpu_parity.py::test_multi_radius_fused_matches_oracle_concatenation —
maps = concat(oracle.forward(R=1), oracle.forward(R=2)); grad_x = oracle.backward(go[:, :8], R=1) +
oracle.backward(go[:, 8:], R=2) + grad_gap[b,c] / (H*W); gap against x.double().mean((2, 3)).  Tolerances are the project's
own for the kernels these instantiations derive from: TOL of tests/test_gpu_parity.py for float32, 1e-2 (maps) / 2e-2
(gradients) for bf16 on bf16-rounded inputs."""
import re

import numpy as np
import pytest
import torch

from conftest import rel_err
from neighbour_feature_pooling_amd import MultiRadiusNFPPooling, NFPPooling, NFPWithGap, _abi, nfp_with_gap
from neighbour_feature_pooling_amd import functional as F
from neighbour_feature_pooling_amd.synth import feature_map
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bf16_round(a):
    return torch.from_numpy(a).bfloat16().float().numpy()


#        shape            measure   mode       dtype    the path it reaches
CASES = [((2, 16, 3, 3), "cosine", "reflect", "f32"),      # reflect folds taps onto the pixel itself
         ((2, 24, 5, 6), "cosine", "zeros", "f32"),        # non-square
         ((3, 48, 14, 14), "norm", "reflect", "f32"),      # 12 channel blocks of 4 channels in the backward, many gather rounds
         ((2, 16, 7, 7), "dot", "reflect", "f32"),         # VAR finalize
         ((2, 16, 7, 7), "rmse", "zeros", "f32"),          # VAR finalize (zeros: a reflected radius-2 tap can fold onto its own
                                                           # pixel, distance 0, where RMSE has no gradient — NaN in the reference too)
         ((4, 64, 7, 7), "cosine", "reflect", "bf16"),     # bf16 storage (vector kernels: no matrix-core form of two radii)
         ((300, 8, 5, 5), "cosine", "reflect", "f32")]     # more images than the backward's workgroup target: one block per image
TAGS = {"cosine": "cos", "norm": "l2", "dot": "dot", "rmse": "rmse"}
_REF = {}


def _ctor(measure, mode):
    return dict(measure=measure, padding_mode=mode, **({"p": 2} if measure == "norm" else {}))


def _reference(oracle, shape, measure, mode, bf):
    """(x, grad_gap, grad_out, ref maps, ref grad_x of grad_out alone) — computed once per case, never modified."""
    key = (shape, measure, mode, bf)
    if key not in _REF:
        x, gg = feature_map(shape, 81), feature_map(shape[:2], 82)
        go = feature_map((shape[0], 32, shape[2], shape[3]), 83)
        if bf:
            x, go = _bf16_round(x), _bf16_round(go)
        c1 = dict(_ctor(measure, mode), R=1, padding=1)
        c2 = dict(c1, R=2, padding=2)
        ref = np.concatenate([oracle.forward(x, **c1), oracle.forward(x, **c2)], axis=1)
        gx = oracle.backward(x, go[:, :8].copy(), **c1).astype(np.float64) + oracle.backward(x, go[:, 8:].copy(), **c2)
        _REF[key] = (x, gg, go, ref, gx)
        for a in _REF[key]:
            a.setflags(write=False)
    return _REF[key]


def _as_layout(xt, layout):
    B, C, H, W = xt.shape
    if layout == "nhwc":
        return xt.contiguous(memory_format=torch.channels_last)
    if layout == "tokens":     # [B, 1 + HW, C] tokens behind a class token, viewed as [B,C,H,W]: batch stride (1 + HW) C
        buf = torch.zeros(B, 1 + H * W, C, device=xt.device, dtype=xt.dtype)
        buf[:, 1:] = xt.flatten(2).transpose(1, 2)
        x = buf[:, 1:].transpose(1, 2).unflatten(2, (H, W))
        assert B == 1 or x.stride(0) == (1 + H * W) * C
        return x
    return xt


@pytest.mark.parametrize("grads", ["both", "gap", "maps"])
@pytest.mark.parametrize("layout", ["nchw", "nhwc", "tokens"])
@pytest.mark.parametrize("shape,measure,mode,dt", CASES)
def test_values_and_gradients_against_the_oracle(shape, measure, mode, dt, layout, grads, dev, oracle_lib):
    bf = dt == "bf16"
    xh, ggh, goh, ref, ref_gx_maps = _reference(oracle_lib, shape, measure, mode, bf)
    B, C, H, W = shape
    tdt = torch.bfloat16 if bf else torch.float32
    x = _as_layout(torch.tensor(xh).to(dev, tdt), layout).detach().requires_grad_(True)
    L = _abi.load()
    head = NFPWithGap(MultiRadiusNFPPooling(C, R_list=(1, 2), **_ctor(measure, mode)))
    n0 = L.nfp_launch_count()
    gap, maps = head(x)
    fwd = L.nfp_last_variant().decode()
    assert gap.dtype == torch.float32 and tuple(gap.shape) == (B, C)
    assert maps.dtype == tdt and tuple(maps.shape) == (B, 32, H, W)
    gg, go = torch.tensor(ggh).to(dev), torch.tensor(goh).to(dev, tdt)
    loss = {"both": lambda: (gap * gg).sum() + (maps.float() * go.float()).sum(), "gap": lambda: (gap * gg).sum(),
            "maps": lambda: (maps.float() * go.float()).sum()}[grads]()
    loss.backward()
    bwd = L.nfp_last_variant().decode()
    lay = "nchw" if layout == "nchw" else "nhwc"
    assert fwd == f"fwd_band<R1+2,{TAGS[measure]},{dt},{lay},gap>x1", fwd
    assert bwd == f"bwd_fast<R1+2,{TAGS[measure]},{dt},{lay},gap>", bwd
    assert L.nfp_launch_count() - n0 == 2, (fwd, bwd)           # ONE kernel each way: no pool_fold, no second radius
    e_gap = rel_err(gap.detach().cpu().numpy(), xh.astype(np.float64).mean((2, 3)))
    e_map = rel_err(maps.detach().float().cpu().numpy(), ref)
    ref_gx = (ref_gx_maps if grads != "gap" else 0.0) + \
        (ggh.astype(np.float64)[:, :, None, None] / (H * W) if grads != "maps" else 0.0) + np.zeros(shape)
    e_gx = rel_err(x.grad.float().cpu().numpy(), ref_gx)
    print(f"{shape} {measure} {dt} {layout} {grads}: gap {e_gap:.2e} maps {e_map:.2e} grad_x {e_gx:.2e} [{fwd} | {bwd}]")
    assert x.grad.shape == x.shape and x.grad.dtype == tdt
    assert e_gap <= TOL
    assert e_map <= (1e-2 if bf else TOL)
    assert e_gx <= (2e-2 if bf else TOL)


@pytest.mark.parametrize("shape,measure,mode,dt", [CASES[2], CASES[5]])
def test_two_runs_are_bitwise_equal(shape, measure, mode, dt, dev):
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    xh = feature_map(shape, 91)
    head = NFPWithGap(MultiRadiusNFPPooling(shape[1], **_ctor(measure, mode)))
    runs = []
    for _ in range(2):
        x = torch.from_numpy(xh).to(dev, tdt).requires_grad_(True)
        gap, maps = head(x)
        ((gap * 0.5).sum() + maps.float().square().sum()).backward()
        runs.append((gap.detach().clone(), maps.detach().clone(), x.grad.clone()))
    assert ",gap>" in _abi.load().nfp_last_variant().decode()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _cfg(radii):
    c1 = NFPPooling(16, R=1, measure="cosine", padding=1).config
    return c1 if radii == 1 else F.multi_radius_config(c1, NFPPooling(16, R=2, measure="cosine", padding=2).config)


@pytest.mark.parametrize("use", ["both", "gap", "maps"])
@pytest.mark.parametrize("radii", [1, 2])
def test_cpp_node_equals_python_node_bitwise(radii, use, dev, monkeypatch):
    cpp = F._cpp_nodes()
    assert cpp and callable(getattr(cpp, "nfp_gap_apply", None)), "the build has no C++ gap node"
    cfg = _cfg(radii)
    xh = feature_map((3, 16, 6, 7), 95)
    w = torch.from_numpy(feature_map((3, 8 if radii == 1 else 32, 6, 7), 96)).to(dev)
    res = []
    for nodes in (cpp, False):
        monkeypatch.setattr(F, "_CPP", nodes)
        x = torch.from_numpy(xh).to(dev).requires_grad_(True)
        gap, maps = nfp_with_gap(x, cfg)
        name = gap.grad_fn.name()
        assert ("NfpGapNode" in name) == bool(nodes) and ("_NfpGapHip" in name) == (not nodes), name
        {"both": lambda: (gap * 0.25).sum() + (maps * w).sum(), "gap": lambda: (gap * 0.25).sum(),
         "maps": lambda: (maps * w).sum()}[use]().backward()
        assert ",gap>" in _abi.load().nfp_last_variant().decode()
        res.append((gap.detach().clone(), maps.detach().clone(), x.grad.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape,kw", [((2, 8, 24, 24), dict(R_list=(1, 2), measure="cosine")),         # above 512 pixels
                                      ((2, 8, 6, 6), dict(R_list=(1, 2), measure="canberra")),
                                      ((2, 8, 6, 6), dict(R_list=(1, 2), measure="norm", p=1)),
                                      ((2, 8, 6, 6), dict(R_list=(1, 2), measure="cosine", bias=True)),
                                      ((2, 8, 8, 8), dict(R_list=(2, 3), measure="cosine"))])
def test_unserved_calls_are_the_composition(shape, kw, dev):
    torch.manual_seed(5)
    layer = MultiRadiusNFPPooling(shape[1], **kw).to(dev)
    x = torch.from_numpy(feature_map(shape, 51)).to(dev).requires_grad_(True)
    L = _abi.load()
    gap, maps = NFPWithGap(layer)(x)
    assert ",gap>" not in L.nfp_last_variant().decode()
    (gap.sum() + maps.square().sum()).backward()
    assert ",gap>" not in L.nfp_last_variant().decode()
    x2 = x.detach().clone().requires_grad_(True)
    gap2, maps2 = x2.mean((2, 3)).float(), layer(x2)
    (gap2.sum() + maps2.square().sum()).backward()
    assert torch.equal(gap, gap2) and torch.equal(maps, maps2) and torch.allclose(x.grad, x2.grad, rtol=0, atol=1e-6)


def test_compiled_fullgraph_equals_eager(dev):
    layer = NFPWithGap(MultiRadiusNFPPooling(8))
    w = torch.from_numpy(feature_map((2, 32, 5, 5), 62)).to(dev)

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
    assert re.match(r"bwd_fast<R1\+2,.*,gap>", L.nfp_last_variant().decode())
    assert torch.allclose(yc, f(x.detach()), rtol=1e-6, atol=1e-6) and torch.allclose(xc.grad, x.grad, rtol=0, atol=1e-6)


def test_multi_radius_head_net_train_step(dev):
    from neighbour_feature_pooling_amd.models import NFPHeadNet
    torch.manual_seed(0)
    net = NFPHeadNet("resnet18", num_classes=3, R_list=(1, 2), bottleneck_dim=16).to(dev)
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    L = _abi.load()
    seen = []
    loss = torch.nn.functional.cross_entropy(net(torch.randn(4, 3, 128, 128, device=dev)), torch.tensor([0, 2, 1, 1], device=dev))
    seen.append(L.nfp_last_variant().decode())
    loss.backward()
    seen.append(L.nfp_last_variant().decode())
    opt.step()
    assert all("R1+2" in v and ",gap>" in v for v in seen), seen       # [4,512,4,4]: one NFP kernel each way
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
