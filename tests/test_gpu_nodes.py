"""The two flavours of autograd node — C++ (csrc/nfp_torch.cpp) and Python (functional.py) — for the families that had no
flavour-equality test which also evicts the plan: the valid-map kernels (cosine), their L1 family (Norm p = 1) and GAP(x)
beside the maps.  Bitwise equal outputs and gradients, the same launches, a backward that needs nothing from the plan
cache, no node without a gradient to follow, and an empty batch."""
import gc

import pytest
import torch

from neighbour_feature_pooling_amd import _abi, nfp_valid, nfp_with_gap
from neighbour_feature_pooling_amd import functional as F

pytestmark = pytest.mark.gpu

FAMILIES = {"valid": (lambda x, cfg: (nfp_valid(x, cfg),), F.NfpConfig(R=1, measure="cosine", padding=0, diff_weights=False)),
            "valid_abs": (lambda x, cfg: (nfp_valid(x, cfg),), F.NfpConfig(R=1, measure="norm", p=1, padding=0, diff_weights=True)),
            "gap": (nfp_with_gap, F.NfpConfig(R=1, measure="cosine", padding=1, diff_weights=False))}
OUT_SHAPES = {"valid": lambda B: [(B, 8, 4, 4)], "valid_abs": lambda B: [(B, 8, 4, 4)], "gap": lambda B: [(B, 8), (B, 8, 6, 6)]}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _input(kind, dev):
    g = torch.Generator(device="cpu").manual_seed(23)
    if kind == "f32_nchw":
        return (torch.rand(2, 8, 6, 6, generator=g) + 0.25).to(dev)
    if kind == "bf16_nhwc":     # (8 channels: the fewest whose channels-last images meet the 16-byte rule)
        return (torch.rand(2, 8, 6, 6, generator=g) + 0.25).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    buf = (torch.rand(4, 8, 6, 6, generator=g) + 0.25).to(dev)
    x = buf[::2]
    assert x.stride(0) == 2 * 8 * 36 and not x.is_contiguous()
    return x


def _run(fn, cfg, x0, gos, evict=False):
    """(outputs, grad_x, launches) of one forward + backward; evict: the plan cache is emptied between the two."""
    x = x0.detach().requires_grad_(True)            # (detach keeps the strides of a view)
    n0 = _abi.load().nfp_launch_count()
    outs = fn(x, cfg)
    names = [o.grad_fn.name() for o in outs]
    if evict:
        F._PLANS.clear()
        gc.collect()
    gx, = torch.autograd.grad(outs, x, [g.to(o.dtype) for g, o in zip(gos, outs)])
    torch.cuda.synchronize()
    return [o.detach() for o in outs], gx, _abi.load().nfp_launch_count() - n0, names


@pytest.mark.parametrize("kind", ["f32_nchw", "bf16_nhwc", "batch_strided_view"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_cpp_and_python_nodes_agree_and_outlive_the_plan(family, kind, dev):
    cpp = F._cpp_nodes()
    assert cpp, "the C++ autograd nodes (_nfp_torch.so) are not built / do not load"
    fn, cfg = FAMILIES[family]
    x0 = _input(kind, dev)
    g = torch.Generator(device="cpu").manual_seed(29)
    gos = [torch.randn(s, generator=g).to(dev) for s in OUT_SHAPES[family](2)]
    res = {}
    try:
        for flavour in (cpp, False):
            F._CPP = flavour
            _run(fn, cfg, x0, gos)                  # (a geometry's first call also fills its tables)
            outs, gx, n, names = _run(fn, cfg, x0, gos)
            assert [tuple(o.shape) for o in outs] == OUT_SHAPES[family](2) and gx.shape == x0.shape
            assert all(("CppNode" in name) == bool(flavour) for name in names), names
            assert gx.dtype == x0.dtype and gx.abs().max().item() > 0
            _, gx_evicted, n_evicted, _ = _run(fn, cfg, x0, gos, evict=True)
            assert torch.equal(gx_evicted, gx) and n_evicted == n
            with torch.no_grad():
                assert all(o.grad_fn is None for o in fn(x0.detach().requires_grad_(True), cfg))
            plain = fn(x0.detach(), cfg)
            assert all(o.grad_fn is None and not o.requires_grad for o in plain)
            assert all(torch.equal(a, b) for a, b in zip(plain, outs))
            res[bool(flavour)] = (outs, gx, n)
    finally:
        F._CPP = cpp
    (outs_c, gx_c, n_c), (outs_p, gx_p, n_p) = res[True], res[False]
    assert n_c == n_p >= 2, (n_c, n_p)              # the same launches, whichever node: at least one each way
    assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(outs_c, outs_p))
    assert gx_c.stride() == gx_p.stride() and torch.equal(gx_c, gx_p)


@pytest.mark.parametrize("flavour", ["cpp", "python"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_an_empty_batch_has_the_right_shapes(family, flavour, dev):
    cpp = F._cpp_nodes()
    assert cpp, "the C++ autograd nodes (_nfp_torch.so) are not built / do not load"
    fn, cfg = FAMILIES[family]
    try:
        F._CPP = cpp if flavour == "cpp" else False
        x = torch.zeros(0, 8, 6, 6, device=dev, requires_grad=True)
        outs = fn(x, cfg)
        assert [tuple(o.shape) for o in outs] == OUT_SHAPES[family](0)
        gx, = torch.autograd.grad(outs, x, [torch.zeros_like(o) for o in outs])
        assert tuple(gx.shape) == (0, 8, 6, 6)
    finally:
        F._CPP = cpp
