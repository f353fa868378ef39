"""memory_format on nfp_compress_map and on the modules built over it, on the host: the channels-last result of the torch
composition against the default call (values, gradients and statistics bit for bit), the refusals, the modules' unchanged
initialisation, state dict and fixtures, and the nfp_cproj_*_fmt declarations with their argument checks (which run
before any HIP call).  No GPU needed."""
import copy
import os
import re

import pytest
import torch

import cases_bottleneck as KB
import cases_insert as KI
import test_bottleneck_host as TB
import test_insert_host as TI
from conftest import ROOT, load_golden
from neighbour_feature_pooling_amd import NFPBottleneck, NFPInsert, _abi, functional, nfp_compress_map, nfp_compress_map_tensors
from neighbour_feature_pooling_amd.models import NFPInsertNet

TOL = 1e-5
CL = torch.channels_last
NEW_EXPORTS = {"nfp_cproj_forward_fmt", "nfp_cproj_backward_fmt"}


def _cl(t):
    return t.is_contiguous(memory_format=CL)


def _step(training, relu, **kw):
    """(out, the four gradients, running mean and variance after) of nfp_compress_map_tensors on TI._inputs under one
    NCHW grad_out."""
    maps, w, gamma, beta, rm, rv = TI._inputs()
    leaves = [t.clone().requires_grad_(True) for t in (maps, w, gamma, beta)]
    go = torch.randn(3, 6, 5, 4, generator=torch.Generator().manual_seed(9))
    out = nfp_compress_map_tensors(*leaves, rm, rv, training, 0.1, 1e-5, relu, **kw)
    return out, torch.autograd.grad(out, leaves, go), rm, rv


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("training", [True, False])
def test_channels_last_on_cpu_is_the_default_call_in_another_layout(training, relu):
    out, grads, rm, rv = _step(training, relu, memory_format=CL)
    ref, rgrads, rrm, rrv = _step(training, relu)
    assert out.shape == (3, 6, 5, 4) and _cl(out) and not out.is_contiguous()
    assert ref.is_contiguous() and torch.equal(out, ref)
    for a, b in zip(grads, rgrads):
        assert torch.equal(a, b)
    assert torch.equal(rm, rrm) and torch.equal(rv, rrv)
    same, *_ = _step(training, relu, memory_format=torch.contiguous_format)
    assert same.is_contiguous() and torch.equal(same, ref)


def test_the_module_form_takes_the_keyword_too():
    maps, w = TI._inputs()[:2]
    for kw in (dict(), dict(momentum=None)):
        a, b = torch.nn.BatchNorm2d(6, **kw), torch.nn.BatchNorm2d(6, **kw)
        got, want = nfp_compress_map(maps, w, a, memory_format=CL), nfp_compress_map(maps, w, b)
        assert _cl(got) and not got.is_contiguous() and torch.equal(got, want)
        for k, v in b.state_dict().items():
            assert torch.equal(a.state_dict()[k], v), k


def test_refusals():
    maps, w, gamma, beta, rm, rv = TI._inputs()
    bn = torch.nn.BatchNorm2d(6)
    with pytest.raises(ValueError, match="channels_last needs"):
        nfp_compress_map_tensors(maps.flatten(2), w, gamma, beta, rm, rv, True, memory_format=CL)
    with pytest.raises(ValueError, match="channels_last needs"):
        nfp_compress_map(maps.flatten(2), w, bn, memory_format=CL)
    for bad in (torch.preserve_format, torch.channels_last_3d, None):
        with pytest.raises(ValueError, match="memory_format"):
            nfp_compress_map_tensors(maps, w, gamma, beta, rm, rv, True, memory_format=bad)
        with pytest.raises(ValueError, match="memory_format"):
            nfp_compress_map(maps, w, bn, memory_format=bad)
    assert int(bn.num_batches_tracked) == 0                 # refused before the step counter moves
    with pytest.raises(TypeError):                          # keyword only
        nfp_compress_map_tensors(maps, w, gamma, beta, rm, rv, True, 0.1, 1e-5, True, CL)
    with pytest.raises(ValueError, match="fused_project"):
        NFPBottleneck(16, 32, memory_format=CL)
    with pytest.raises(ValueError, match="fused_project"):
        NFPBottleneck(16, 32, memory_format=torch.preserve_format)
    for bad in (torch.channels_last_3d, None):
        with pytest.raises(ValueError, match="memory_format"):
            NFPInsert(8, memory_format=bad)
        with pytest.raises(ValueError, match="memory_format"):
            NFPBottleneck(16, 32, fused_project=True, memory_format=bad)
    with pytest.raises(TypeError):                          # keyword only
        NFPInsert(8, None, CL)


def test_routing_keeps_unmeasured_channels_last_classes_with_the_composition(monkeypatch):
    class T:      # (what cproj_hip_serves looks at, without a device)
        def __init__(self, shape):
            self.shape, self.dtype, self.is_cuda = torch.Size(shape), torch.float32, True

        def is_contiguous(self):
            return True

        def numel(self):
            return self.shape.numel()

    g, w24 = torch.ones(24), torch.ones(24, 8, 1, 1)
    serves = functional.cproj_hip_serves
    monkeypatch.setenv("NFP_CPROJ_TORCH", "0")
    assert serves(T((4, 8, 7, 7)), w24, g, g, 0.1, channels_last=True)
    monkeypatch.setenv("NFP_CPROJ_TORCH", "1")
    assert not serves(T((64, 8, 54, 54)), w24, g, g, 0.1, channels_last=True)
    monkeypatch.delenv("NFP_CPROJ_TORCH")
    # the default, channels-last: what DESIGN 4g's three-arm table shows faster than the composition beyond the spread
    assert (functional.CPROJ_ROUTED_NHWC_EVAL_MAPS, functional.CPROJ_ROUTED_NHWC_TRAIN_PIXELS) == (24, 256 * 12 * 12)
    cl = dict(channels_last=True)
    assert serves(T((256, 8, 12, 12)), w24, g, g, 0.1, **cl) and serves(T((64, 8, 26, 26)), w24, g, g, 0.1, **cl)
    assert not serves(T((64, 8, 12, 12)), w24, g, g, 0.1, **cl) and not serves(T((64, 8, 5, 5)), w24, g, g, 0.1, **cl)
    w_24maps = torch.ones(24, 24, 1, 1)
    assert not serves(T((64, 24, 24, 24)), w_24maps, g, g, 0.1, **cl)                    # the 24-map step lost
    assert serves(T((64, 24, 24, 24)), w_24maps, g, g, 0.1, False, False, **cl)          # its eval forward won
    assert serves(T((4, 8, 7, 7)), w24, g, g, 0.1, False, False, **cl)
    assert not serves(T((4, 8, 7, 7)), w24, g, g, 0.1, False, True, **cl)                # a backward on running statistics
    assert not serves(T((4, 32, 7, 7)), torch.ones(24, 32, 1, 1), g, g, 0.1, False, False, **cl)     # 32 maps: not measured
    # ... and the NCHW routing stands as it was
    assert serves(T((64, 8, 54, 54)), w24, g, g, 0.1) and not serves(T((64, 8, 26, 26)), w24, g, g, 0.1)
    assert not serves(T((64, 24, 24, 24)), w_24maps, g, g, 0.1, False, False)


@pytest.mark.parametrize("fmt", [CL, torch.preserve_format])
def test_the_keyword_changes_no_parameter_and_no_state_dict_key(fmt):
    for build in (lambda **kw: NFPInsert(12, **kw), lambda **kw: NFPInsert(10, 6, R=2, measure="cosine", padding=2, **kw),
                  lambda **kw: NFPBottleneck(16, 32, fused_project=True, **kw),
                  lambda **kw: NFPInsertNet(num_classes=5, nfp_insert_idx=1, **kw)):
        torch.manual_seed(11)
        a = build()
        after_a = torch.rand(1)
        torch.manual_seed(11)
        b = build(memory_format=fmt)
        after_b = torch.rand(1)
        assert torch.equal(after_a, after_b)                # the RNG was consumed alike
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
        assert [k for k, _ in a.named_parameters()] == [k for k, _ in b.named_parameters()]
    assert NFPInsertNet(nfp_insert_idx=0, memory_format=CL).insert.memory_format == CL
    assert NFPInsert(8).memory_format == NFPBottleneck(16, 32).memory_format == torch.contiguous_format


@pytest.mark.parametrize("name", [c["name"] for c in KI.INSERT_CASES])
def test_insert_channels_last_matches_the_reference_fixture(name):
    c = KI.INSERT_BY_NAME[name]
    g = load_golden(name)
    m = NFPInsert(c["shape"][1], memory_format=CL, **c["kw"])
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p:")}, strict=True)
    m.train(c["train"])
    out = copy.deepcopy(m)(torch.from_numpy(KI.make_input(c)))      # (a copy: the step below is the fixture's one)
    assert _cl(out) and not out.is_contiguous()
    errs = TI.fixture_errors(TI.run_insert(m, c), g)
    print(errs)
    for k, e in errs.items():
        assert e <= TOL, (k, e)


@pytest.mark.parametrize("name", [c["name"] for c in KB.BNECK_CASES])
def test_bottleneck_channels_last_matches_the_reference_fixture(name):
    c = KB.BNECK_BY_NAME[name]
    g = load_golden(name)
    m = NFPBottleneck(c["cin"], c["cout"], c["stride"], fused_project=True, memory_format=CL)
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p:")}, strict=True)
    m.train(c["train"])
    got = TB.run_bneck(m, c)
    assert got[0].shape == g["out"].shape
    errs = TB.fixture_errors(got, g)
    print(errs)
    for k, e in errs.items():
        assert e <= TOL, (k, e)


def test_preserve_format_follows_the_input():
    torch.manual_seed(3)
    ins = NFPInsert(8, measure="cosine", padding=1, memory_format=torch.preserve_format)
    blk = NFPBottleneck(8, 16, fused_project=True, memory_format=torch.preserve_format)
    x = torch.randn(2, 8, 9, 9)
    for m in (ins, blk):
        m.eval()
        with torch.no_grad():
            a, b = m(x), m(x.contiguous(memory_format=CL))
        assert a.is_contiguous() and not _cl(a)
        assert _cl(b) and not b.is_contiguous()
        assert torch.allclose(a, b, rtol=0, atol=1e-5 * float(a.abs().max()))
    # an input dense in both layouts (one channel): NCHW
    one = NFPInsert(1, out_channels=4, measure="cosine", padding=1, memory_format=torch.preserve_format).eval()
    x1 = torch.randn(2, 1, 6, 6)
    assert x1.is_contiguous() and _cl(x1) and one(x1).is_contiguous()


def test_header_binding_and_library_declare_the_fmt_calls():
    header = open(os.path.join(ROOT, "include", "nfp.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(nfp_[a-z0-9_]+)\s*\(", body))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(_abi.EXPORTS)
    assert re.search(r"enum nfp_act_layout \{ NFP_ACT_NCHW = 0, NFP_ACT_NHWC = 1 \}", body)
    assert (_abi.ACT_NCHW, _abi.ACT_NHWC) == (0, 1)
    assert int(re.search(r"#define NFP_ABI_VERSION (\d+)", header).group(1)) == _abi.ABI_VERSION == 7
    from neighbour_feature_pooling_amd.build import build_hip
    build_hip()
    L = _abi.load()
    for n in NEW_EXPORTS:
        assert hasattr(L, n), n
    assert L.nfp_abi_version() == 7
    # the existing length query serves both layouts and returns what it did
    assert L.nfp_cproj_scratch_floats(4, 8, 49, 32, 0) == 4 * (2 * 8 + 64) == L.nfp_cpool_scratch_floats(4, 8, 49, 32, 0)
    assert L.nfp_cproj_scratch_floats(4, 8, 49, 32, 1) == 4 * 32 * 9 + 1 * (8 + 64)
    assert L.nfp_cproj_scratch_floats(2, 32, 1600, 16, 1) == 2 * 25 * 16 * 33 + 1 * (32 + 1024)
    assert L.nfp_cproj_scratch_floats(0, 8, 49, 32, 1) == 1 and L.nfp_cproj_scratch_floats(4, 33, 49, 32, 1) == 1


def test_fmt_calls_refuse_what_the_plain_calls_refuse_and_unknown_layouts():
    """Every call here is refused, or returns, before any HIP call: the pointer is never dereferenced and the launch counter
    stands still.  The rows are those test_gpu_cproj.py sends through nfp_cproj_forward / nfp_cproj_backward."""
    from neighbour_feature_pooling_amd.build import build_hip
    build_hip()
    L = _abi.load()
    INVALID, UNSUPPORTED = -1, -2
    MOM, EPS = 0.1, 1e-5
    B, N, P, D = 4, 8, 49, 32
    p = 0x1000      # (never dereferenced)
    ns = int(L.nfp_cpool_saved_floats(N, D))
    nf, nb = int(L.nfp_cproj_scratch_floats(B, N, P, D, 0)), int(L.nfp_cproj_scratch_floats(B, N, P, D, 1))

    def fwd(B=B, N=N, P=P, D=D, dtype=0, training=1, relu=1, maps=p, w=p, gamma=p, beta=p, rm=p, rv=p, mom=MOM, eps=EPS, out=p,
            saved=p, ns=ns, scratch=p, nscr=nf, layout=1):
        return L.nfp_cproj_forward_fmt(B, N, P, D, dtype, training, relu, maps, w, gamma, beta, rm, rv, mom, eps, out, saved, ns,
                                       scratch, nscr, None, layout)

    def bwd(B=B, N=N, P=P, D=D, dtype=0, training=1, relu=1, maps=p, w=p, gamma=p, beta=p, rm=None, rv=None, eps=EPS, saved=p,
            ns=ns, go=p, gm=p, gw=p, gg=p, gb=p, scratch=p, nscr=nb, layout=1):
        return L.nfp_cproj_backward_fmt(B, N, P, D, dtype, training, relu, maps, w, gamma, beta, rm, rv, eps, saved, ns, go, gm,
                                        gw, gg, gb, scratch, nscr, None, layout)

    n0 = L.nfp_launch_count()
    for layout in (-1, 2):
        assert fwd(layout=layout) == INVALID and b"nfp_cproj_forward_fmt" in L.nfp_last_error()
        assert b"layout" in L.nfp_last_error()
        assert bwd(layout=layout) == INVALID and b"nfp_cproj_backward_fmt" in L.nfp_last_error()
        assert fwd(layout=layout, training=0) == INVALID and bwd(layout=layout, gm=None, gw=None, gg=None, gb=None) == INVALID
    for layout in (0, 1):
        for kw in (dict(B=-1), dict(N=0), dict(P=0), dict(D=0), dict(dtype=2), dict(eps=-1.0), dict(mom=float("nan")),
                   dict(maps=None), dict(w=None), dict(gamma=None), dict(beta=None), dict(out=None), dict(rm=None),
                   dict(training=0, rm=None, rv=None), dict(saved=None), dict(ns=ns - 1), dict(scratch=None), dict(nscr=nf - 1)):
            assert fwd(layout=layout, **kw) == INVALID, kw
            assert b"nfp_cproj_forward_fmt" in L.nfp_last_error()
        for kw in (dict(B=-1), dict(N=0), dict(P=0), dict(D=0), dict(dtype=2), dict(eps=-1.0), dict(maps=None), dict(w=None),
                   dict(gamma=None), dict(beta=None), dict(go=None), dict(training=0), dict(saved=None), dict(ns=ns - 1),
                   dict(scratch=None), dict(nscr=nb - 1), dict(training=0, rm=p, rv=p, gm=None, scratch=None, nscr=0)):
            assert bwd(layout=layout, **kw) == INVALID, kw
            assert b"nfp_cproj_backward_fmt" in L.nfp_last_error()
        for kw in (dict(N=33), dict(P=2 ** 28), dict(N=1, P=2 ** 27), dict(D=2 ** 22 + 1), dict(B=1, P=1)):
            assert fwd(layout=layout, **kw) == UNSUPPORTED, kw
            assert bwd(layout=layout, **kw) == UNSUPPORTED, kw
        assert bwd(layout=layout, gm=None, gw=None, gg=None, gb=None) == 0      # nothing asked for: nothing to do
        assert fwd(layout=layout, B=0, maps=None, out=None, scratch=None, nscr=0) == 0      # an empty batch: OK, no launch
    assert L.nfp_launch_count() == n0
