"""DeepTENEncoding on the host: reference-identical initialisation and state dict, the torch formulation against the
reference's float64 fixtures (tests/golden/deepten_*.npz, make_golden_deepten.py), the nfp_deepten_* declarations with their
argument checks (which run before any HIP call), and a DeepTENNet train step.  No GPU needed.

The bar of every comparison with a float64 reference (here and in test_gpu_deepten.py), per result:
    err = max|got - ref64| / max|ref64|  <=  max(4 * err32, 2e-6)
err32: the same quantity for a float32 run of the reference formulation on the same inputs — the fixture's float32 arrays, or
`_host.deepten_host` in float32 — never the code under test.  Factor 4: another summation order draws another sample of the
same rounding noise; the floor is about 32 float32 roundings of the largest element, for a reference that lands exact."""
import os
import re

import numpy as np
import pytest
import torch

import cases_deepten as KD
from conftest import ROOT, load_golden, rel_err
from neighbour_feature_pooling_amd import DeepTENEncoding, _abi, nfp_deepten_encode
from neighbour_feature_pooling_amd._host import deepten_host

NEW_EXPORTS = {"nfp_deepten_saved_floats", "nfp_deepten_scratch_floats", "nfp_deepten_forward", "nfp_deepten_backward"}
NAMES = ("out", "grad_x", "grad_codewords", "grad_scale")
FLOOR = 2e-6


def bar(err32):
    return max(4.0 * err32, FLOOR)


def deepten_module(c, g=None):
    """The case's module with the fixture's parameters."""
    g = load_golden(c["name"]) if g is None else g
    m = DeepTENEncoding(c["shape"][1], c["K"])
    with torch.no_grad():
        m.codewords.copy_(torch.from_numpy(g["codewords"]))
        m.scale.copy_(torch.from_numpy(g["scale"]))
    return m, g


def run_module(m, x, go):
    """out, grad_x, grad_codewords, grad_scale (float64 numpy) of the module on x (which takes a gradient) and grad_out."""
    x = x.detach().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    out = m(x)
    out.backward(go.to(out.dtype))
    return tuple(t.detach().double().cpu().numpy() for t in (out, x.grad, m.codewords.grad, m.scale.grad))


def check_under_the_bar(got, ref64, ref32, label="", names=NAMES, out=print):
    """Every named result of `got` against ref64, err32 taken from ref32 (dicts or tuples in NAMES order)."""
    def pick(r, i, n):
        return np.asarray(r[n] if isinstance(r, dict) else r[i], np.float64)
    for i, n in enumerate(NAMES):
        if n not in names:
            continue
        r64 = pick(ref64, i, n + "_64" if isinstance(ref64, dict) else n).reshape(-1)
        e32 = rel_err(pick(ref32, i, n).reshape(-1), r64)
        err = rel_err(pick(got, i, n).reshape(-1), r64)
        out(f"{label} {n}: err {err:.3e} err32 {e32:.3e} bar {bar(e32):.3e}")
        assert err <= bar(e32), (label, n, err, e32)


# ---- initialisation and state dict ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,D,K,seed", KD.DEEPTEN_INIT_CASES + [(c["name"], c["shape"][1], c["K"], c["seed"])
                                                                   for c in KD.DEEPTEN_CASES if c["params"] == "init"],
                         ids=lambda v: v if isinstance(v, str) else None)
def test_init_matches_the_reference_bitwise(name, D, K, seed):
    g = load_golden(name)
    torch.manual_seed(seed)
    m = DeepTENEncoding(D, K)
    assert (m.D, m.K) == (D, K)
    assert np.array_equal(m.codewords.detach().numpy(), g["codewords"])
    assert np.array_equal(m.scale.detach().numpy(), g["scale"])
    assert sorted(m.state_dict()) == [str(k) for k in g["sd_keys"]] == ["codewords", "scale"]
    fresh = DeepTENEncoding(D, K)
    fresh.load_state_dict({"codewords": torch.from_numpy(g["codewords"]), "scale": torch.from_numpy(g["scale"])}, strict=True)
    assert torch.equal(fresh.codewords.detach(), m.codewords.detach())


# ---- the torch formulation against the reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in KD.DEEPTEN_CASES])
def test_host_float64_matches_the_reference_float64(name):
    c = KD.DEEPTEN_BY_NAME[name]
    m, g = deepten_module(c)
    got = run_module(m.double(), torch.from_numpy(KD.make_x(c)).double(), torch.from_numpy(KD.make_grad_out(c)).double())
    for a, n in zip(got, NAMES):
        assert rel_err(a.reshape(-1), g[n + "_64"].reshape(-1)) <= 1e-12, n


@pytest.mark.parametrize("name", [c["name"] for c in KD.DEEPTEN_CASES])
def test_cpu_float32_module_is_under_the_bar(name):
    c = KD.DEEPTEN_BY_NAME[name]
    m, g = deepten_module(c)
    got = run_module(m, torch.from_numpy(KD.make_x(c)), torch.from_numpy(KD.make_grad_out(c)))
    check_under_the_bar(got, g, g, name)


def test_functional_checks_shapes_and_takes_any_strides():
    torch.manual_seed(2)
    x = torch.randn(2, 6, 3, 8, dtype=torch.float64)[..., ::2]
    cw, sc = torch.randn(4, 6, dtype=torch.float64), -torch.rand(4, dtype=torch.float64)
    a = nfp_deepten_encode(x, cw, sc)
    assert a.shape == (2, 24) and a.dtype == torch.float64
    assert torch.equal(a, deepten_host(x.contiguous(), cw, sc))
    # the reference's op sequence (deepten.py:31-58)
    X = x.reshape(2, 6, -1).transpose(1, 2)
    r = X.unsqueeze(2) - cw
    A = torch.softmax(-sc * (r ** 2).sum(3), dim=2)
    assert torch.allclose(a, (A.unsqueeze(3) * r).sum(1).reshape(2, -1), rtol=0, atol=1e-13)
    with pytest.raises(RuntimeError):
        nfp_deepten_encode(x, cw[:, :5], sc)
    with pytest.raises(RuntimeError):
        nfp_deepten_encode(x, cw, sc[:3])
    with pytest.raises(RuntimeError):
        nfp_deepten_encode(x[0], cw, sc)
    empty = nfp_deepten_encode(x[:0], cw.requires_grad_(True), sc)
    assert empty.shape == (0, 24)
    empty.sum().backward()
    assert torch.equal(cw.grad, torch.zeros_like(cw))


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_and_loadable():
    src = open(os.path.join(ROOT, "include", "nfp.h")).read()
    assert "deepten.py:51-58" in src
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(nfp_[a-z_]+)\s*\(", body))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(_abi.EXPORTS)
    from neighbour_feature_pooling_amd import build
    assert "nfp_deepten.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "nfp_deepten.hip"))
    build.build_hip()
    L = _abi.load()
    for n in NEW_EXPORTS:
        assert hasattr(L, n)
    assert L.nfp_abi_version() == _abi.ABI_VERSION == 7


def test_refusals_launch_nothing():
    from neighbour_feature_pooling_amd.build import build_hip
    build_hip()
    L = _abi.load()
    assert L.nfp_deepten_saved_floats(3, 49, 32) == 2 * 3 * 49 * 32 and L.nfp_deepten_saved_floats(0, 49, 32) == 1
    # w alone; with a parameter gradient the [B,K,D] partials and one row of K per pixel tile (16 pixels at K = 32)
    assert L.nfp_deepten_scratch_floats(3, 49, 32, 512, 0) == 3 * 49 * 32
    assert L.nfp_deepten_scratch_floats(3, 49, 32, 512, 1) == 3 * 49 * 32 + 3 * 32 * 512 + 3 * 4 * 32
    assert L.nfp_deepten_scratch_floats(0, 49, 32, 512, 1) == 1
    p = 0x1000      # (never dereferenced: every call below is refused, or returns, before any HIP call)
    n0 = L.nfp_launch_count()
    ns, nscr = 2 * 2 * 9 * 5, 2 * 9 * 5 + 2 * 5 * 20 + 2 * 1 * 5

    def fwd(B=2, N=9, K=5, D=20, dtype=0, layout=0, sxB=180, x=p, cw=p, sc=p, out=p, saved=p, ns=ns):
        return L.nfp_deepten_forward(B, N, K, D, dtype, layout, sxB, x, cw, sc, out, saved, ns, None)

    def bwd(B=2, N=9, K=5, D=20, dtype=0, layout=0, sxB=180, x=p, cw=p, sc=p, saved=p, ns=ns, go=p, gx=p, gc=p, gs=p,
            scratch=p, nscr=nscr):
        return L.nfp_deepten_backward(B, N, K, D, dtype, layout, sxB, x, cw, sc, saved, ns, go, gx, gc, gs, scratch, nscr, None)

    for kw in (dict(x=None), dict(cw=None), dict(sc=None), dict(out=None), dict(saved=None), dict(B=-1), dict(N=0), dict(K=0),
               dict(D=0), dict(dtype=2), dict(dtype=-1), dict(layout=2), dict(layout=-1), dict(sxB=-1), dict(ns=ns - 1)):
        assert fwd(**kw) == -1, kw
        assert L.nfp_last_error()
    for kw in (dict(x=None), dict(cw=None), dict(sc=None), dict(saved=None), dict(go=None), dict(B=-1), dict(N=0), dict(K=0),
               dict(D=0), dict(dtype=7), dict(layout=5), dict(ns=ns - 1), dict(scratch=None), dict(nscr=nscr - 1),
               dict(gc=None, gs=None, nscr=2 * 9 * 5 - 1)):
        assert bwd(**kw) == -1, kw
    assert b"scratch" in L.nfp_last_error()
    assert fwd(K=65) == -2 and bwd(K=65) == -2                                   # more than 64 codewords
    assert fwd(N=1 << 31, ns=1 << 40) == -2 and fwd(N=1 << 20, D=1 << 11, ns=1 << 40) == -2     # extents of 2^31 and more
    assert bwd(N=1 << 20, D=1 << 11, ns=1 << 40, nscr=1 << 42) == -2
    assert fwd(B=0, x=None, out=None, saved=None, ns=0) == 0                     # an empty batch: OK, no launch
    assert bwd(B=0, x=None, saved=None, go=None, gx=None, scratch=None, ns=0, nscr=0) == 0
    assert bwd(gx=None, gc=None, gs=None, scratch=None, nscr=0) == 0             # no gradient asked for: nothing to do
    assert L.nfp_launch_count() == n0


# ---- the nets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone", ["resnet18", "vit_tiny_patch16_224"])
def test_deepten_net_train_step_on_cpu(backbone):
    from neighbour_feature_pooling_amd import train
    from neighbour_feature_pooling_amd.models import DeepTENNet
    torch.manual_seed(0)
    net = train.build(backbone, num_classes=5, image=32, pooling="deepten", num_codes=4)
    assert isinstance(net, DeepTENNet) and isinstance(net.encoding, DeepTENEncoding)
    C = net.backbone.num_features
    assert net.encoding.codewords.shape == (4, C) and net.bn.num_features == net.fc.in_features == 4 * C
    assert {"encoding.codewords", "encoding.scale", "bn.weight", "fc.weight"} <= set(net.state_dict())
    step, _ = train.make_step(net)
    x, y = train.synthetic_batch(4, 3, 32, 5, "cpu", torch.float32, seed=1)
    before = net.encoding.codewords.detach().clone()
    l0 = float(step(x, y))
    l1 = float(step(x, y))
    assert np.isfinite(l0) and np.isfinite(l1)
    assert not torch.equal(before, net.encoding.codewords.detach())
    assert isinstance(train.build("resnet18", num_classes=5, image=32), type(train.build("resnet18", num_classes=5, image=32,
                                                                                        pooling="nfp")))
    with pytest.raises(ValueError):
        train.build("resnet18", pooling="gap")
