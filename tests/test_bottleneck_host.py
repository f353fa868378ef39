"""NFPBottleneck and functional.nfp_valid on the host: the module against the reference's fixtures (tests/golden/bneck_*.npz,
make_golden_bottleneck.py), reference-identical initialisation and state dict, nfp_valid's routing and argument checks,
and the nfp_valid_* declarations with their argument checks (which run before any HIP call).  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cases_bottleneck as KB
from conftest import ROOT, load_golden, rel_err
from neighbour_feature_pooling_amd import NFPBottleneck, NFPPooling, _abi, nfp_op, nfp_valid
from neighbour_feature_pooling_amd.functional import build_desc

TOL = 1e-5
NEW_EXPORTS = {"nfp_valid_supported", "nfp_valid_saved_floats", "nfp_valid_forward", "nfp_valid_backward"}
SD_KEYS = {"conv1.weight", "conv2.weight", "nfp.center_value.weight", "nfp.comp_neighbors.weight",
           "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var", "bn1.num_batches_tracked",
           "bn2.weight", "bn2.bias", "bn2.running_mean", "bn2.running_var", "bn2.num_batches_tracked"}


def bneck_module(c, g=None):
    """The case's module with the fixture's parameters and BatchNorm buffers (strict load), in the case's mode."""
    g = load_golden(c["name"]) if g is None else g
    m = NFPBottleneck(c["cin"], c["cout"], c["stride"])
    sd = {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p:")}
    m.load_state_dict(sd, strict=True)
    m.train(c["train"])
    return m, g


def run_bneck(m, c, dev="cpu", dtype=torch.float32, channels_last=False):
    """out, grad_x, {parameter gradients}, {BatchNorm buffers after the step} (numpy float32) of the case's seeded step."""
    x = torch.from_numpy(KB.make_input(c)).to(dev).to(dtype)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    m.zero_grad(set_to_none=True)
    out = m(x)
    out.backward(torch.from_numpy(KB.make_grad_out(c, out.shape)).to(dev).to(out.dtype))
    grads = {k: p.grad.detach().float().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    after = {k: v.detach().float().cpu().numpy() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    return out.detach().float().cpu().numpy(), x.grad.detach().float().cpu().numpy(), grads, after


def fixture_errors(got, g):
    """{tensor name: error relative to the fixture tensor's max magnitude} for out, grad_x, every parameter gradient and
    every BatchNorm buffer after the step."""
    out, gx, grads, after = got
    errs = {"out": rel_err(out, g["out"]), "grad_x": rel_err(gx, g["grad_x"])}
    gkeys = [k[2:] for k in g if k.startswith("g:")]
    assert sorted(grads) == sorted(gkeys)
    for k in gkeys:
        errs["g:" + k] = rel_err(grads[k], g["g:" + k])
    akeys = [k[6:] for k in g if k.startswith("after:")]
    assert sorted(after) == sorted(akeys) and akeys
    for k in akeys:
        errs["after:" + k] = rel_err(after[k], g["after:" + k])
    return errs


@pytest.mark.parametrize("name", [c["name"] for c in KB.BNECK_CASES])
def test_cpu_matches_reference_fixture(name):
    c = KB.BNECK_BY_NAME[name]
    m, g = bneck_module(c)
    got = run_bneck(m, c)
    assert got[0].shape == g["out"].shape
    errs = fixture_errors(got, g)
    print(errs)
    assert {"g:conv1.weight", "g:conv2.weight", "g:bn1.weight", "g:bn1.bias", "g:bn2.weight", "g:bn2.bias"} <= set(errs)
    if c["cin"] != c["cout"]:
        assert {"g:downsample.0.weight", "g:downsample.1.weight", "g:downsample.1.bias"} <= set(errs)
    for k, e in errs.items():
        assert e <= TOL, (k, e)


def test_eval_mode_leaves_the_running_statistics_alone():
    c = KB.BNECK_BY_NAME["bneck_eval_4x16x9x9"]
    g = load_golden(c["name"])
    for k in g:
        if k.startswith("after:"):
            assert np.array_equal(g[k], g["p:" + k[6:]])


@pytest.mark.parametrize("name,cin,cout,stride,seed", KB.BNECK_INIT_CASES, ids=[c[0] for c in KB.BNECK_INIT_CASES])
def test_init_matches_the_reference_bitwise(name, cin, cout, stride, seed):
    g = load_golden(name)
    torch.manual_seed(seed)
    m = NFPBottleneck(cin, cout, stride)
    sd = m.state_dict()
    stored = [k[2:] for k in g if k.startswith("p:")]
    assert stored and sorted(sd) == [str(k) for k in g["sd_keys"]]
    for k in stored:
        assert np.array_equal(sd[k].numpy(), g["p:" + k]), k
    assert m.expansion == 1 and NFPBottleneck.expansion == 1
    assert m.conv1.stride == (stride, stride) and m.conv2.in_channels == 8 and m.nfp.in_channels == cout // 4
    assert isinstance(m.downsample, torch.nn.Identity) == (cin == cout)


@pytest.mark.parametrize("name", ["bneck_s1_down_4x16x9x9", "bneck_s1_ident_2x32x7x7"])
def test_state_dict_keys_and_strict_load(name):
    c = KB.BNECK_BY_NAME[name]
    m, g = bneck_module(c)       # (load_state_dict(strict=True) of the fixture's parameters)
    sd = m.state_dict()
    assert sorted(sd) == [str(k) for k in g["sd_keys"]]
    want = set(SD_KEYS)
    if c["cin"] != c["cout"]:
        want |= {"downsample.0.weight"} | {"downsample.1." + s for s in ("weight", "bias", "running_mean", "running_var",
                                                                         "num_batches_tracked")}
    assert set(sd) == want
    assert torch.equal(m.conv1.weight.detach(), torch.from_numpy(g["p:conv1.weight"]))
    # a reference state dict carries the layer's two frozen conv weights as well: accepted under strict=True
    fresh = NFPBottleneck(c["cin"], c["cout"], c["stride"])
    fresh.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    assert torch.equal(fresh.conv2.weight, m.conv2.weight)


def test_match_is_sized_from_the_last_dimension_alone():
    m = NFPBottleneck(16, 32, stride=2)
    with pytest.raises(RuntimeError):       # a non-square map behind stride 2 fails, as in the reference
        m(torch.randn(2, 16, 12, 16))


@pytest.mark.parametrize("ctor", [dict(R=1, measure="cosine"), dict(R=2, measure="norm", p=2), dict(R=1, measure="rmse"),
                                  dict(R=1, measure="norm"), dict(R=1, measure="pearson")])
def test_nfp_valid_on_cpu_tensors_is_nfp(ctor):
    torch.manual_seed(3)
    cfg = NFPPooling(6, padding=0, **ctor).config
    x = torch.randn(2, 6, 7, 8, requires_grad=True)
    a, b = nfp_valid(x, cfg), nfp_op(x, cfg)
    assert torch.equal(a, b) and a.shape == (2, (2 * ctor["R"] + 1) ** 2 - 1, 7 - 2 * ctor["R"], 8 - 2 * ctor["R"])
    go = torch.randn_like(a)
    assert torch.equal(torch.autograd.grad(a, x, go)[0], torch.autograd.grad(b, x, go)[0])


@pytest.mark.parametrize("kw", [dict(padding=1), dict(padding=0, stride=2), dict(padding=0, dilation=2)])
def test_nfp_valid_refuses_other_geometries(kw):
    cfg = NFPPooling(4, R=1, measure="cosine", **kw).config
    with pytest.raises(ValueError):
        nfp_valid(torch.randn(1, 4, 9, 9), cfg)


def test_new_exports_are_declared_and_loadable():
    src = open(os.path.join(ROOT, "include", "nfp.h")).read()
    assert "nfp_heads.py:234-278" in src
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(nfp_[a-z_]+)\s*\(", body))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(_abi.EXPORTS)
    assert int(re.search(r"#define NFP_ABI_VERSION (\d+)", src).group(1)) == _abi.ABI_VERSION == 7
    from neighbour_feature_pooling_amd import build
    assert "nfp_valid.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "nfp_valid.hip"))
    build.build_hip()
    L = _abi.load()
    for n in NEW_EXPORTS:
        assert hasattr(L, n)
    assert L.nfp_abi_version() == 7


def _desc(shape=(2, 8, 6, 7), layout="nchw", dtype=torch.float32, **kw):
    from neighbour_feature_pooling_amd.functional import _canon
    ctor = dict(R=1, measure="cosine", padding=0)
    ctor.update(kw)
    cfg = NFPPooling(shape[1], **ctor).config
    return build_desc(shape, _canon(shape, layout), dtype, cfg)


def test_invalid_arguments_launch_nothing():
    """NFP_E_INVALID for a null pointer, a short `saved` and map_f32 = 1 on float32 storage; pad = 1 is a descriptor the
    reference accepts and these kernels do not serve — NFP_E_UNSUPPORTED, as include/nfp.h states.  No launch in either."""
    from neighbour_feature_pooling_amd.build import build_hip
    build_hip()
    L = _abi.load()
    p = 0x1000      # (never dereferenced: every call below is refused, or returns, before any HIP call)
    d = _desc()
    need = L.nfp_valid_saved_floats(ctypes.byref(d))
    assert need == 2 * 6 * 7 and L.nfp_valid_supported(ctypes.byref(d)) == 1
    n0 = L.nfp_launch_count()

    def fwd(d=d, x=p, out=p, saved=p, ns=need):
        return L.nfp_valid_forward(ctypes.byref(d), x, out, saved, ns, None)

    def bwd(d=d, x=p, go=p, out=p, saved=p, ns=need, gx=p):
        return L.nfp_valid_backward(ctypes.byref(d), x, go, out, saved, ns, gx, None)

    for kw in (dict(x=None), dict(out=None), dict(ns=need - 1)):
        assert fwd(**kw) == -1, kw
        assert L.nfp_last_error()
    for kw in (dict(x=None), dict(go=None), dict(out=None), dict(gx=None), dict(saved=None), dict(ns=need - 1)):
        assert bwd(**kw) == -1, kw
    assert b"saved" in L.nfp_last_error()
    mixed = _desc()
    mixed.map_f32 = 1                       # (float32 storage: a malformed descriptor)
    assert fwd(d=mixed) == -1 and bwd(d=mixed) == -1 and L.nfp_valid_supported(ctypes.byref(mixed)) == 0
    for bad in (_desc(padding=1), _desc(dtype=torch.bfloat16), _desc(shape=(2, 8, 6, 300)), _desc(measure="pearson"),
                _desc(measure="norm"), _desc(shape=(2, 6, 6, 7), layout="nhwc")):
        if bad.dtype == _abi.BF16 and bad.pad == 0 and bad.W == 7:
            bad.map_f32 = 1                 # (bf16 storage with float32 maps: valid for nfp_forward, refused here)
        assert fwd(d=bad) == -2 and bwd(d=bad) == -2, (bad.pad, bad.W, bad.measure)
        assert L.nfp_valid_supported(ctypes.byref(bad)) == 0
    empty = _desc(shape=(0, 8, 6, 7))
    assert fwd(d=empty, x=None, out=None, saved=None, ns=0) == 0        # an empty batch: OK, no launch
    assert bwd(d=empty, x=None, go=None, out=None, saved=None, ns=0, gx=None) == 0
    assert L.nfp_launch_count() == n0


def test_supported_is_a_host_only_dry_run():
    from neighbour_feature_pooling_amd.build import build_hip
    build_hip()
    L = _abi.load()
    n0, v0, e0 = L.nfp_launch_count(), L.nfp_last_variant(), L.nfp_last_error()
    served = [_desc(), _desc(R=2, measure="norm", p=2), _desc(shape=(3, 16, 9, 128), layout="nhwc", dtype=torch.bfloat16),
              _desc(shape=(65535, 1, 3, 3)), _desc(shape=(1, 5, 32767, 5), measure="rmse"), _desc(shape=(0, 8, 6, 7)),
              _desc(measure="gfc", similarity=False), _desc(measure="dot")]
    for d in served:
        assert L.nfp_valid_supported(ctypes.byref(d)) == 1, (d.B, d.C, d.H, d.W, d.measure)
    for d in (_desc(shape=(1, 8, 6, 129)), _desc(padding=1), _desc(measure="canberra"), _desc(measure="Norm", p=2)):
        assert L.nfp_valid_supported(ctypes.byref(d)) == 0
    assert L.nfp_valid_saved_floats(ctypes.byref(_desc(measure="dot"))) == 0
    assert L.nfp_valid_saved_floats(ctypes.byref(_desc(R=2, measure="norm", p=2))) == 0
    assert (L.nfp_launch_count(), L.nfp_last_variant(), L.nfp_last_error()) == (n0, v0, e0)
