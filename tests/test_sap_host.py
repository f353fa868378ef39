"""SimilarityAwarePooling on the host: the module against the reference's fixtures (tests/golden/sap_*.npz,
make_golden_sap.py) through the torch formulation, reference-identical initialisation and state dict, the constructor's
TypeError, and the nfp_attpool_* declarations with their argument checks (which run before any HIP call).  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

import cases as K
import cases_sap as KS
from conftest import ROOT, load_golden, rel_err
from neighbour_feature_pooling_amd import SimilarityAwarePooling, _abi, nfp_attention_pool
from neighbour_feature_pooling_amd._host import attention_pool_host

NEW_EXPORTS = {"nfp_attpool_scratch_floats", "nfp_attpool_forward", "nfp_attpool_backward"}


def sap_module(c, g=None):
    """The case's module with the fixture's parameters."""
    g = load_golden(c["name"]) if g is None else g
    m = SimilarityAwarePooling(c["shape"][1], **c["ctor"])
    with torch.no_grad():
        m.att_proj.weight.copy_(torch.from_numpy(g["w"]))
        m.att_proj.bias.copy_(torch.from_numpy(g["b"]))
        if "nfp_bc" in g:
            m.nfp.center_value.bias.copy_(torch.from_numpy(g["nfp_bc"]))
            m.nfp.comp_neighbors.bias.copy_(torch.from_numpy(g["nfp_nb"]))
    return m, g


def run_sap(m, c, dtype=torch.float32, dev="cpu", channels_last=False):
    """pooled, grad_x, grad_w, grad_b (numpy float32) of the case's seeded input and pooled gradient."""
    x = torch.from_numpy(K.make_input(c)).to(dtype).to(dev)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    m.zero_grad(set_to_none=True)
    pooled = m(x)
    pooled.backward(torch.from_numpy(KS.make_grad_pooled(c, pooled.shape[1])).to(pooled.dtype).to(dev))
    return tuple(t.detach().float().cpu().numpy() for t in (pooled, x.grad, m.att_proj.weight.grad, m.att_proj.bias.grad))


def check_against_fixture(got, g, tol, tol_grad=None, out=print):
    """The issue's bars: `tol` of each tensor's max magnitude; |grad_b| <= tol * max|grad_w| (it is zero in exact
    arithmetic, so it has no magnitude of its own)."""
    tol_grad = tol if tol_grad is None else tol_grad
    pooled, gx, gw, gb = got
    errs = dict(pooled=rel_err(pooled, g["pooled"]), grad_x=rel_err(gx, g["grad_x"]),
                grad_w=rel_err(gw.reshape(-1), g["grad_w"].reshape(-1)), grad_b=float(np.abs(gb).max()),
                grad_b_bar=tol_grad * float(np.abs(g["grad_w"]).max()))
    out(errs)
    assert errs["pooled"] <= tol
    assert errs["grad_x"] <= tol_grad
    assert errs["grad_w"] <= tol_grad
    assert errs["grad_b"] <= errs["grad_b_bar"]


@pytest.mark.parametrize("name", [c["name"] for c in KS.SAP_CASES])
def test_cpu_matches_reference_fixture(name):
    c = KS.SAP_BY_NAME[name]
    m, g = sap_module(c)
    check_against_fixture(run_sap(m, c), g, 1e-5)


def test_one_pixel_maps_pool_to_the_map_itself():
    c = KS.SAP_BY_NAME["sap_cos_one_pixel_2x8x3x3"]
    m, g = sap_module(c)
    x = torch.from_numpy(K.make_input(c))
    assert torch.equal(m(x), m.nfp(x).flatten(1))
    assert np.abs(g["grad_w"]).max() == 0


@pytest.mark.parametrize("name,C,ctor,seed", KS.SAP_INIT_CASES, ids=[c[0] for c in KS.SAP_INIT_CASES])
def test_init_matches_the_reference_bitwise(name, C, ctor, seed):
    g = load_golden(name)
    torch.manual_seed(seed)
    m = SimilarityAwarePooling(C, **ctor)
    assert np.array_equal(m.att_proj.weight.detach().numpy(), g["w"])
    assert np.array_equal(m.att_proj.bias.detach().numpy(), g["b"])
    assert m.nfp_channels == m.att_proj.in_channels == g["w"].shape[1]
    assert isinstance(m.softmax, torch.nn.Softmax)


@pytest.mark.parametrize("name", ["sap_cos_r1_2x16x7x7", "sap_cos_bias_2x8x7x6", "sap_l2_r2_3x8x9x8"])
def test_state_dict_keys_and_strict_load_of_a_reference_state_dict(name):
    c = KS.SAP_BY_NAME[name]
    m, g = sap_module(c)
    sd = m.state_dict()
    assert sorted(sd) == [str(k) for k in g["sd_keys"]]
    assert {"nfp.comp_neighbors.weight", "nfp.center_value.weight", "att_proj.weight", "att_proj.bias"} <= set(sd)
    if c["ctor"].get("bias"):
        assert {"nfp.comp_neighbors.bias", "nfp.center_value.bias"} <= set(sd)
    # a reference-shaped state dict: its frozen one-hot conv weights and the fixture's parameters
    ref_sd = {k: v.clone() for k, v in sd.items()}
    fresh = SimilarityAwarePooling(c["shape"][1], **c["ctor"])
    fresh.load_state_dict(ref_sd, strict=True)
    assert torch.equal(fresh.att_proj.weight.detach(), torch.from_numpy(g["w"]))
    assert torch.equal(fresh.att_proj.bias.detach(), torch.from_numpy(g["b"]))
    if c["ctor"].get("bias"):
        assert torch.equal(fresh.nfp.comp_neighbors.bias.detach(), torch.from_numpy(g["nfp_nb"]))


def test_padding_keyword_is_a_type_error():
    with pytest.raises(TypeError):
        SimilarityAwarePooling(8, R=1, measure="cosine", padding=1)


def test_functional_accepts_both_weight_shapes_and_any_dtype():
    torch.manual_seed(1)
    maps = torch.randn(2, 8, 5, 4, dtype=torch.float64, requires_grad=True)
    w, b = torch.randn(1, 8, 1, 1, dtype=torch.float64), torch.randn(1, dtype=torch.float64)
    a = nfp_attention_pool(maps, w, b)
    assert a.dtype == torch.float64 and a.shape == (2, 8)
    assert torch.equal(a, nfp_attention_pool(maps, w.reshape(-1), b))
    assert torch.equal(a, attention_pool_host(maps, w, b))
    # the reference's op sequence (nfp_heads.py:227-231)
    att = torch.softmax(torch.nn.functional.conv2d(maps, w, b).flatten(2), dim=-1).view(2, 1, 5, 4)
    assert torch.allclose(a, (maps * att).sum(dim=[2, 3]), rtol=0, atol=1e-13)
    strided = torch.randn(2, 8, 5, 8, dtype=torch.float64)[..., ::2]
    assert torch.allclose(nfp_attention_pool(strided, w, b), nfp_attention_pool(strided.contiguous(), w, b))
    with pytest.raises(RuntimeError):
        nfp_attention_pool(maps, w[:, :4], b)


def test_new_exports_are_declared_and_loadable():
    src = open(os.path.join(ROOT, "include", "nfp.h")).read()
    assert "nfp_heads.py:224-232" in src
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(nfp_[a-z_]+)\s*\(", body))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(_abi.EXPORTS)
    assert int(re.search(r"#define NFP_ABI_VERSION (\d+)", src).group(1)) == _abi.ABI_VERSION == 7
    from neighbour_feature_pooling_amd import build
    assert "nfp_attpool.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "nfp_attpool.hip"))
    # no unit can be left out of the library: the list is every csrc/*.hip, once
    assert sorted(build.SOURCES) == sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    build.build_hip()
    L = _abi.load()
    for n in NEW_EXPORTS:
        assert hasattr(L, n)
    assert L.nfp_abi_version() == 7


def test_invalid_arguments_return_minus_one_and_launch_nothing():
    from neighbour_feature_pooling_amd.build import build_hip
    build_hip()
    L = _abi.load()
    assert L.nfp_attpool_scratch_floats(3, 8) == 27 and L.nfp_attpool_scratch_floats(0, 8) == 1
    p = 0x1000      # (never dereferenced: every call below is refused, or returns, before any HIP call)
    n0 = L.nfp_launch_count()

    def fwd(B=2, N=8, P=25, dtype=0, maps=p, w=p, b=p, pooled=p, att=p):
        return L.nfp_attpool_forward(B, N, P, dtype, maps, w, b, pooled, att, None)

    def bwd(B=2, N=8, P=25, dtype=0, maps=p, w=p, att=p, gp=p, gm=p, gw=p, gb=p, scratch=p, ns=18):
        return L.nfp_attpool_backward(B, N, P, dtype, maps, w, att, gp, gm, gw, gb, scratch, ns, None)

    for kw in (dict(maps=None), dict(w=None), dict(b=None), dict(pooled=None), dict(B=-1), dict(N=0), dict(P=0), dict(dtype=2),
               dict(dtype=-1)):
        assert fwd(**kw) == -1, kw
        assert L.nfp_last_error()
    for kw in (dict(maps=None), dict(w=None), dict(att=None), dict(gp=None), dict(B=-1), dict(N=0), dict(P=0), dict(dtype=7),
               dict(ns=17), dict(scratch=None), dict(gw=None, ns=17), dict(gb=None, ns=0)):
        assert bwd(**kw) == -1, kw
    assert b"scratch" in L.nfp_last_error()
    assert fwd(N=2, P=1 << 30) == -2 and bwd(N=2, P=1 << 30) == -2      # N * P >= 2^31
    assert fwd(B=0, maps=None, pooled=None, att=None) == 0               # an empty batch: OK, no launch
    assert bwd(B=0, maps=None, att=None, gp=None, gm=None, ns=1) == 0
    assert L.nfp_launch_count() == n0
