"""The L1 family of the valid-map kernels on the host: the nfp_valid_abs_* declarations, their host-only dry runs and
argument checks (which run before any HIP call), functional.nfp_valid's CPU behaviour for Norm p = 1 / EMD, and
NFPInsert / NFPInsertNet with valid_layer=True against valid_layer=False and the reference's fixtures.  No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

import cases_insert as KI
from conftest import ROOT, load_golden
from neighbour_feature_pooling_amd import NFPInsert, NFPPooling, _abi, nfp_op, nfp_valid
from neighbour_feature_pooling_amd.models import NFPInsertNet
from test_bottleneck_host import _desc as _cos_desc
from test_insert_host import fixture_errors, run_insert

TOL = 1e-5
NEW_EXPORTS = {"nfp_valid_abs_supported", "nfp_valid_abs_forward", "nfp_valid_abs_backward"}
L1_FIXTURES = ["insert_default_2x12x9x9", "insert_r2_2x8x9x11"]


def _desc(shape=(2, 8, 6, 7), layout="nchw", dtype=torch.float32, **kw):
    """test_bottleneck_host._desc with the class default measure (Norm p = 1) where none is given."""
    kw.setdefault("measure", "norm")
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
    return [_desc(), _desc(measure="emd"), _desc(R=2), _desc(shape=(3, 16, 9, 128), layout="nhwc", dtype=torch.bfloat16),
            _desc(shape=(65535, 1, 3, 3)), _desc(shape=(1, 5, 32767, 5)), _desc(shape=(0, 8, 6, 7)),
            _desc(similarity=False), _desc(measure="emd", similarity=False, R=2)]


def _refused():
    mixed = _desc(dtype=torch.bfloat16)
    mixed.map_f32 = 1           # (bf16 storage with float32 maps: valid for nfp_forward, refused here)
    return [_desc(measure="cosine"), _desc(p=2), _desc(p=3), _desc(measure="Norm"), _desc(padding=1),
            _desc(shape=(1, 8, 6, 129)), _desc(shape=(2, 8, 6, 300)), _desc(shape=(2, 6, 6, 7), layout="nhwc"), mixed]


def test_supported_is_a_host_only_dry_run(lib):
    n0, v0, e0 = lib.nfp_launch_count(), lib.nfp_last_variant(), lib.nfp_last_error()
    for d in _served():
        assert lib.nfp_valid_abs_supported(ctypes.byref(d)) == 1, (d.B, d.C, d.H, d.W, d.R, d.measure, d.dtype)
    for d in _refused():
        assert lib.nfp_valid_abs_supported(ctypes.byref(d)) == 0, (d.B, d.C, d.H, d.W, d.pad, d.measure, d.p, d.diff_weights)
    assert (lib.nfp_launch_count(), lib.nfp_last_variant(), lib.nfp_last_error()) == (n0, v0, e0)
    # the existing calls keep refusing the L1 layer (tests/test_bottleneck_host.py pins that too)
    assert lib.nfp_valid_supported(ctypes.byref(_desc())) == 0
    assert lib.nfp_valid_supported(ctypes.byref(_desc(measure="emd"))) == 0


def test_emd_is_served_as_norm_p1_on_the_difference_weights(lib):
    """make_kp turns EMD into Norm p = 1 with diff = 1 whatever the descriptor's own p / diff_weights say."""
    d = _desc(measure="emd")
    d.p, d.diff_weights = 2.0, 0
    assert lib.nfp_valid_abs_supported(ctypes.byref(d)) == 1


def test_the_gpu_sweep_draws_inside_the_served_set(lib):
    """tests/test_gpu_valid_abs.py's 40 seeded geometries: every one is served, so none may fall back on the device."""
    from test_gpu_valid_abs import sweep_cases, sweep_descriptor
    cases = sweep_cases()
    assert len(cases) == 40 and {c[2] for c in cases} == {"norm", "emd"} and {c[4] for c in cases} == {"f32", "bf16"}
    assert {c[1] for c in cases} == {1, 2} and {c[5] for c in cases} == {"nchw", "nhwc"} and {c[3] for c in cases} == {True, False}
    for c in cases:
        assert lib.nfp_valid_abs_supported(ctypes.byref(sweep_descriptor(*c))) == 1, c


def test_invalid_arguments_launch_nothing(lib):
    p = 0x1000      # (never dereferenced: every call below is refused, or returns, before any HIP call)
    n0 = lib.nfp_launch_count()

    def fwd(d, x=p, out=p):
        return lib.nfp_valid_abs_forward(ctypes.byref(d), x, out, None)

    def bwd(d, x=p, go=p, gx=p):
        return lib.nfp_valid_abs_backward(ctypes.byref(d), x, go, gx, None)

    d = _desc()
    for kw in (dict(x=None), dict(out=None)):
        assert fwd(d, **kw) == -1, kw
        assert b"null" in lib.nfp_last_error()
    for kw in (dict(x=None), dict(go=None), dict(gx=None)):
        assert bwd(d, **kw) == -1, kw
        assert b"null" in lib.nfp_last_error()
    for bad in _refused():
        assert fwd(bad) == -2 and bwd(bad) == -2, (bad.pad, bad.W, bad.measure, bad.p)
        assert lib.nfp_last_error()
    broken = _desc()
    broken.map_f32 = 1          # (float32 storage: a malformed descriptor)
    assert fwd(broken) == -1 and bwd(broken) == -1 and lib.nfp_valid_abs_supported(ctypes.byref(broken)) == 0
    empty = _desc(shape=(0, 8, 6, 7))
    assert fwd(empty, x=None, out=None) == 0            # an empty batch: OK, no launch
    assert bwd(empty, x=None, go=None, gx=None) == 0
    assert lib.nfp_launch_count() == n0


@pytest.mark.parametrize("ctor", [dict(R=1, measure="norm"), dict(R=2, measure="norm"), dict(R=1, measure="emd"),
                                  dict(R=2, measure="emd", similarity=False)])
def test_nfp_valid_on_cpu_tensors_is_nfp(ctor):
    torch.manual_seed(3)
    cfg = NFPPooling(6, padding=0, **ctor).config
    x = torch.randn(2, 6, 7, 8, requires_grad=True)
    a, b = nfp_valid(x, cfg), nfp_op(x, cfg)
    assert torch.equal(a, b) and a.shape == (2, (2 * ctor["R"] + 1) ** 2 - 1, 7 - 2 * ctor["R"], 8 - 2 * ctor["R"])
    go = torch.randn_like(a)
    assert torch.equal(torch.autograd.grad(a, x, go)[0], torch.autograd.grad(b, x, go)[0])


def _pair(C, seed, **kw):
    torch.manual_seed(seed)
    off = NFPInsert(C, **kw)
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    on = NFPInsert(C, valid_layer=True, **kw)
    assert torch.equal(state, torch.get_rng_state())        # the same draws in the same order
    return off, on


@pytest.mark.parametrize("kw", [dict(), dict(R=2), dict(measure="cosine", R=1, padding=1), dict(bias=True)],
                         ids=["default", "r2", "padded", "biased"])
def test_insert_valid_layer_on_cpu_is_the_same_block(kw):
    off, on = _pair(12, 11, **kw)
    assert on.valid_layer is True and off.valid_layer is False
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


def test_insert_valid_layer_is_keyword_only_and_keeps_the_channel_check():
    with pytest.raises(TypeError):
        NFPInsert(6, 6, torch.contiguous_format, True)
    with pytest.raises(RuntimeError):
        NFPInsert(6, valid_layer=True)(torch.randn(1, 5, 7, 7))


@pytest.mark.parametrize("name", L1_FIXTURES)
def test_insert_valid_layer_matches_the_reference_fixture(name):
    c = KI.INSERT_BY_NAME[name]
    assert c["kw"].get("measure", "norm") == "norm" and c["kw"].get("padding", 0) == 0      # the L1 layer
    g = load_golden(name)
    m = NFPInsert(c["shape"][1], valid_layer=True, **c["kw"])
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p:")}, strict=True)
    m.train(c["train"])
    assert sorted(m.state_dict()) == [str(k) for k in g["sd_keys"]]
    errs = fixture_errors(run_insert(m, c), g)
    print(name, errs)
    for k, e in errs.items():
        assert e <= TOL, (k, e)


def test_insert_net_with_the_valid_layer_runs_on_cpu():
    torch.manual_seed(0)
    off = NFPInsertNet(num_classes=4, nfp_insert_idx=1)
    torch.manual_seed(0)
    on = NFPInsertNet(num_classes=4, nfp_insert_idx=1, valid_layer=True)
    assert on.insert.valid_layer and not off.insert.valid_layer
    assert list(off.state_dict()) == list(on.state_dict())
    x = torch.randn(2, 3, 32, 32)
    a, b = off(x), on(x)
    assert a.shape == (2, 4) and torch.equal(a, b)
    b.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in on.parameters())
