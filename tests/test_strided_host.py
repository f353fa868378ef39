"""The strided-map family (include/nfp.h: nfp_strided_*, csrc/nfp_strided.hip) on the host: the declarations, the host-only
dry run over the served and the refused descriptors, the argument checks (which run before any HIP call), the dispatcher's
unchanged route, functional.nfp_strided on CPU tensors, NFPInsert / NFPInsertNet with strided_layer on and off, and the
oracle against the reference's strided fixtures.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cases_strided as KS
from conftest import ROOT, load_golden, rel_err
from neighbour_feature_pooling_amd import NFPInsert, NFPPooling, _abi, nfp_op, nfp_strided
from neighbour_feature_pooling_amd.models import NFPInsertNet
from test_bottleneck_host import _desc as _cos_desc

NEW_EXPORTS = {"nfp_strided_supported", "nfp_strided_saved_floats", "nfp_strided_forward", "nfp_strided_backward"}
TOL = 1e-5


def _desc(shape=(2, 8, 9, 10), layout="nchw", dtype=torch.float32, **kw):
    """test_bottleneck_host._desc (cosine, R = 1, padding 0) at stride 2 where none is given."""
    kw.setdefault("stride", 2)
    return _cos_desc(shape, layout, dtype, **kw)


@pytest.fixture(scope="module")
def lib():
    from neighbour_feature_pooling_amd.build import build_hip
    build_hip()
    return _abi.load()


def test_new_exports_are_declared_and_loadable(lib):
    src = open(os.path.join(ROOT, "include", "nfp.h")).read()
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(nfp_[a-z_]+)\s*\(", body))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(_abi.EXPORTS)
    assert int(re.search(r"#define NFP_ABI_VERSION (\d+)", src).group(1)) == _abi.ABI_VERSION == 7
    for n in NEW_EXPORTS:
        assert hasattr(lib, n)
    assert lib.nfp_abi_version() == 7


def _served():
    return [
        _desc(), _desc(measure="dot"), _desc(measure="gfc"), _desc(measure="norm", p=2), _desc(measure="rmse"),      # the measures
        _desc(similarity=False), _desc(measure="norm", p=2, similarity=False),
        _desc(R=2), _desc(stride=3), _desc(stride=4), _desc(R=2, stride=4),
        _desc(padding=1, padding_mode="zeros"), _desc(padding=1, padding_mode="reflect"), _desc(padding=1, padding_mode="replicate"),
        _desc(R=2, padding=2, padding_mode="reflect"),
        _desc(shape=(2, 8, 3, 3)), _desc(shape=(2, 8, 2, 2), padding=1),                                               # H + 2P = 2R + 1
        _desc(shape=(1, 8, 9, 128)), _desc(shape=(1, 8, 9, 126), padding=1), _desc(shape=(1, 8, 9, 128), R=2),        # the widest rows
        _desc(shape=(1, 8, 12, 60), R=2, padding=2),                                                                   # R = 2 with a ring: W + 2P = 64
        _desc(dtype=torch.bfloat16), _desc(layout="nhwc"), _desc(layout="nhwc", dtype=torch.bfloat16),
        _desc(shape=(2, 3, 9, 10)), _desc(shape=(2, 4, 9, 10), layout="nhwc"),
        _desc(shape=(0, 8, 9, 10)), _desc(shape=(65535, 1, 3, 3)),
    ]


def _refused():
    mixed = _desc(dtype=torch.bfloat16)
    mixed.map_f32 = 1
    return [
        _desc(stride=1), _desc(stride=5), _desc(dilation=2, shape=(2, 8, 11, 11)),
        _desc(R=2, padding=1), _desc(padding=2, shape=(2, 8, 11, 11)),                      # a padding that is neither 0 nor R
        _desc(padding=1, padding_mode="circular"),
        _desc(R=3, shape=(2, 8, 11, 11)),
        _desc(measure="canberra"), _desc(measure="norm", p=1), _desc(measure="emd"), _desc(measure="norm", p=3), _desc(measure="Norm"),
        _desc(shape=(1, 8, 9, 129)), _desc(shape=(1, 8, 9, 127), padding=1), _desc(shape=(1, 8, 9, 300)),          # W + 2P over the bound
        _desc(shape=(2, 6, 9, 10), layout="nhwc"), _desc(shape=(2, 4, 9, 10), layout="nhwc", dtype=torch.bfloat16),
        mixed,
    ]


def test_supported_is_a_host_only_dry_run(lib):
    n0, v0, e0 = lib.nfp_launch_count(), lib.nfp_last_variant(), lib.nfp_last_error()
    for d in _served():
        assert lib.nfp_strided_supported(ctypes.byref(d)) == 1, (d.B, d.C, d.H, d.W, d.R, d.pad, d.stride, d.measure, d.dtype)
    for d in _refused():
        assert lib.nfp_strided_supported(ctypes.byref(d)) == 0, (d.B, d.C, d.H, d.W, d.R, d.pad, d.stride, d.measure, d.p)
    assert (lib.nfp_launch_count(), lib.nfp_last_variant(), lib.nfp_last_error()) == (n0, v0, e0)


def test_saved_floats(lib):
    assert lib.nfp_strided_saved_floats(ctypes.byref(_desc())) == 2 * 9 * 10
    assert lib.nfp_strided_saved_floats(ctypes.byref(_desc(measure="gfc", padding=1))) == 2 * 9 * 10
    for m in (dict(measure="dot"), dict(measure="norm", p=2), dict(measure="rmse"), dict(stride=1)):
        assert lib.nfp_strided_saved_floats(ctypes.byref(_desc(**m))) == 0, m


def test_refusals_launch_nothing_and_say_why(lib):
    p = 0x1000      # (never dereferenced: every call below is refused, or returns, before any HIP call)
    d = _desc()
    need = lib.nfp_strided_saved_floats(ctypes.byref(d))
    n0 = lib.nfp_launch_count()

    def fwd(d=d, x=p, out=p, saved=p, ns=need):
        return lib.nfp_strided_forward(ctypes.byref(d), x, out, saved, ns, None)

    def bwd(d=d, x=p, go=p, out=p, saved=p, ns=need, gx=p):
        return lib.nfp_strided_backward(ctypes.byref(d), x, go, out, saved, ns, gx, None)

    for kw in (dict(x=None), dict(out=None)):
        assert fwd(**kw) == -1 and b"null" in lib.nfp_last_error(), kw
    for kw in (dict(x=None), dict(go=None), dict(out=None), dict(gx=None)):
        assert bwd(**kw) == -1 and b"null" in lib.nfp_last_error(), kw
    assert fwd(ns=need - 1) == -1 and b"saved holds" in lib.nfp_last_error()
    assert bwd(ns=need - 1) == -1 and b"saved holds" in lib.nfp_last_error()
    assert bwd(saved=None) == -1 and b"saved holds 0" in lib.nfp_last_error()
    for bad, why in [(_desc(stride=1), b"stride 2 to 4"), (_desc(dilation=2, shape=(2, 8, 11, 11)), b"dilation 1"),
                     (_desc(padding=1, padding_mode="circular"), b"zeros / reflect / replicate"),
                     (_desc(R=3, shape=(2, 8, 11, 11)), b"R = 1 or 2"), (_desc(measure="canberra"), b"cosine / dot / gfc"),
                     (_desc(shape=(1, 8, 9, 127), padding=1), b"128 positions")]:
        assert fwd(bad) == -2 and why in lib.nfp_last_error(), (why, lib.nfp_last_error())
        assert bwd(bad) == -2 and why in lib.nfp_last_error(), (why, lib.nfp_last_error())
    empty = _desc(shape=(0, 8, 9, 10))
    assert fwd(empty, x=None, out=None, saved=None, ns=0) == 0        # an empty batch: OK, no launch
    assert bwd(empty, x=None, go=None, out=None, saved=None, ns=0, gx=None) == 0
    assert lib.nfp_launch_count() == n0


def test_the_dispatcher_keeps_strided_descriptors_on_the_any_geometry_kernels(lib):
    from test_dispatch_plan import desc, plan
    for kw in (dict(shape=(64, 512, 7, 7), stride=2), dict(shape=(64, 64, 56, 56), stride=2, pad=0),
               dict(shape=(4, 16, 28, 28), stride=3, R=2, measure="norm")):
        for backward, name in ((False, "fwd_pairs"), (True, "bwd_gather")):
            rc, text = plan(lib, desc(**kw), backward)
            assert rc == 0 and text.startswith(name), (kw, text)


@pytest.mark.parametrize("ctor", [dict(R=1, measure="cosine", stride=2, padding=0), dict(R=2, measure="norm", p=2, stride=3, padding=2),
                                  dict(R=1, measure="norm", stride=2), dict(R=1, measure="gfc", stride=4, padding=1, padding_mode="zeros")])
def test_nfp_strided_on_cpu_tensors_is_nfp(ctor):
    torch.manual_seed(3)
    cfg = NFPPooling(6, **ctor).config
    x = torch.randn(2, 6, 9, 8, requires_grad=True)
    a, b = nfp_strided(x, cfg), nfp_op(x, cfg)
    assert torch.equal(a, b)
    go = torch.randn_like(a)
    assert torch.equal(torch.autograd.grad(a, x, go)[0], torch.autograd.grad(b, x, go)[0])


def test_nfp_strided_refuses_stride_1_and_dilation_2():
    x = torch.randn(1, 4, 9, 9)
    for kw in (dict(stride=1), dict(stride=2, dilation=2)):
        with pytest.raises(ValueError, match="nfp_valid"):
            nfp_strided(x, NFPPooling(4, measure="cosine", **kw).config)


def _pair(C, seed, **kw):
    torch.manual_seed(seed)
    off = NFPInsert(C, **kw)
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    on = NFPInsert(C, strided_layer=True, **kw)
    assert torch.equal(state, torch.get_rng_state())        # the same draws in the same order
    return off, on


@pytest.mark.parametrize("kw", [dict(stride=2), dict(measure="cosine", R=2, padding=2, stride=2), dict(measure="cosine", stride=1),
                                dict(measure="cosine", stride=2, bias=True)], ids=["default_s2", "cos_r2_s2", "stride1", "biased"])
def test_insert_strided_layer_on_cpu_is_the_same_block(kw):
    off, on = _pair(12, 11, **kw)
    assert on.strided_layer is True and off.strided_layer is False
    sa, sb = off.state_dict(), on.state_dict()
    assert list(sa) == list(sb)
    assert [k for k, _ in off.named_parameters()] == [k for k, _ in on.named_parameters()]
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    torch.manual_seed(5)
    x0 = torch.randn(3, 12, 9, 8)
    res = []
    for m in (off, on):
        x = x0.clone().requires_grad_(True)
        out = m(x)
        out.backward(torch.linspace(-1, 1, out.numel()).reshape(out.shape))
        res.append((out.detach(), x.grad, {k: p.grad for k, p in m.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert sorted(res[0][2]) == sorted(res[1][2]) and res[0][2]
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k


def test_insert_strided_layer_is_keyword_only():
    with pytest.raises(TypeError):
        NFPInsert(6, 6, torch.contiguous_format, False, True)


def test_insert_net_with_the_strided_layer_runs_on_cpu():
    kw = dict(measure="cosine", stride=2, padding=1)
    torch.manual_seed(0)
    off = NFPInsertNet(num_classes=4, nfp_insert_idx=1, nfp_kwargs=kw)
    torch.manual_seed(0)
    on = NFPInsertNet(num_classes=4, nfp_insert_idx=1, nfp_kwargs=kw, strided_layer=True)
    assert on.insert.strided_layer and not off.insert.strided_layer
    assert list(off.state_dict()) == list(on.state_dict())
    for k, v in off.state_dict().items():
        assert torch.equal(v, on.state_dict()[k]), k
    x = torch.randn(2, 3, 32, 32)
    a, b = off(x), on(x)
    assert a.shape == (2, 4) and torch.equal(a, b)
    b.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in on.parameters())


@pytest.mark.parametrize("name", [c["name"] for c in KS.STRIDED_CASES] + KS.EXISTING)
def test_the_oracle_matches_the_reference_fixture(name):
    """The float64 oracle, which the GPU tests measure the kernels against, held to what the reference itself computed."""
    import cases as K
    import oracle
    oracle.build()
    c = KS.STRIDED_BY_NAME.get(name) or K.BY_NAME[name]
    g = load_golden(name)
    x = K.make_input(c)
    out = oracle.forward(x, **c["ctor"])
    gx = oracle.backward(x, K.make_grad_out(c, out.shape), **c["ctor"])
    eo, eg = rel_err(out, g["out"]), rel_err(gx, g["gx"])
    print(name, eo, eg)
    assert out.shape == g["out"].shape and eo <= TOL and eg <= TOL
    assert not np.isnan(g["gx"]).any()
