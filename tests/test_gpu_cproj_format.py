"""nfp_compress_map with a channels-last result and a channels-last grad_out on the MI355X (csrc/nfp_cpool.hip: cproj_fwd_nhwc
and the NHWC forms of cproj_bwd_part / cproj_bwd_maps; include/nfp.h nfp_cproj_*_fmt).  The inputs, the float64 references,
the searched seeds and the bars are test_gpu_cproj.py's: every case's float64 reference keeps min|a| >= 1e-5 max|a|, which
is asserted before anything is compared, and no element is excluded.

What is compared:
  out                  bit for bit with the NCHW call's (the kernels form each element by the same chain), the running
                       statistics too (the same kernels write them)
  the four gradients   against float64 at that file's bars — 1e-5, grad_w 5e-5, offset maps 1e-4, bf16 1e-2 / 2e-2 — and bit
                       for bit with the NCHW call's: behind the staging of grad_out the sums are the NCHW kernels', in order
A grad_out that is NCHW-dense as well (H = W = 1: the one_pixel case) takes the NCHW backward — the same bytes — so there the
backward's variant name carries no `nhwc`; the forward's always does."""
import functools

import pytest
import torch

from conftest import rel_err
from test_gpu_cproj import (BF16_CASES, BF_GRAD, BF_OUT, CASES, EPS, F32, F32_GW, GUARD, MOM, OFFSET, MODES, RELU, _count, _lib,
                            _np, case_ref, errors, reference64, run_hip)

pytestmark = pytest.mark.gpu
CL = torch.channels_last
KEYS = ("gm", "gw", "gg", "gb")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from neighbour_feature_pooling_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _hip_wherever_it_can_serve(monkeypatch):
    """NFP_CPROJ_TORCH=0: the kernels are tested for everything they serve, whatever the default routing takes."""
    monkeypatch.setenv("NFP_CPROJ_TORCH", "0")


def _variant():
    return _lib().nfp_last_variant().decode()


def _name(which, dtype, training, relu, nhwc):
    return f"cproj_{which}<{dtype},{'train' if training else 'eval'},{'relu' if relu else 'lin'}{',nhwc' if nhwc else ''}>"


def run_fmt(ins, training, dev, relu=True, dtype=torch.float32, want=(True,) * 4, inplace=None, out_cl=True, go="cl"):
    """run_hip of test_gpu_cproj.py with the result asked for channels-last (out_cl) and grad_out handed over channels-last
    (go = "cl"), NCHW ("nchw") or as a slice of a wider tensor, dense in neither layout ("slice").  Adds fwd_variant /
    bwd_variant, and go_nchw: whether the grad_out handed over was NCHW-dense."""
    from neighbour_feature_pooling_amd import nfp_compress_map_tensors
    maps, w, gamma, beta, rm, rv, g = ins
    t = [x.to(dev) for x in (maps.to(dtype), w, gamma, beta)]
    t = [x.requires_grad_(r) for x, r in zip(t, want)]
    rm, rv = rm.clone().to(dev), rv.clone().to(dev)
    n0 = _count()
    out = nfp_compress_map_tensors(t[0], t[1], t[2], t[3], rm, rv, training, MOM, EPS, relu,
                                   memory_format=CL if out_cl else torch.contiguous_format)
    n1 = _count()
    fwd_variant = _variant()
    assert out.is_contiguous(memory_format=CL if out_cl else torch.contiguous_format)
    kept = out.detach().clone()
    if inplace == "relu":
        out.relu_()
    elif inplace == "add":
        out += 1
    g = g.to(dev).to(out.dtype)
    if go == "cl":
        g = g.contiguous(memory_format=CL)
    elif go == "slice":
        wide = torch.zeros(g.shape[:3] + (g.shape[3] + 3,), dtype=g.dtype, device=dev)
        wide[..., 1:1 + g.shape[3]] = g
        g = wide[..., 1:1 + g.shape[3]]
        assert not g.is_contiguous() and not g.is_contiguous(memory_format=CL)
    asked = [x for x in t if x.requires_grad]
    grads = iter(torch.autograd.grad(out, asked, g) if asked else ())
    torch.cuda.synchronize()
    n2 = _count()
    res = dict(zip(KEYS, (next(grads) if r else None for r in want)))
    res.update(out=kept, rm=rm, rv=rv, fwd=n1 - n0, bwd=n2 - n1, fwd_variant=fwd_variant, bwd_variant=_variant(),
               go_nchw=g.is_contiguous())
    return res


@functools.lru_cache(maxsize=None)
def nchw_run(name, training, relu=True, bf16=False):
    """The NCHW call on a case's inputs (test_gpu_cproj.py::run_hip) — run once, shared, never modified."""
    ins, _ = case_ref(name, training, relu, bf16)
    return run_hip(ins, training, torch.device("cuda:0"), relu, torch.bfloat16 if bf16 else torch.float32)


def same_as_nchw(got, plain):
    assert torch.equal(got["out"], plain["out"])
    assert torch.equal(got["rm"], plain["rm"]) and torch.equal(got["rv"], plain["rv"])
    for k in KEYS:
        if got[k] is not None:
            assert torch.equal(got[k], plain[k]), k


@pytest.mark.parametrize("relu", RELU)
@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_float32_channels_last_both_ways(name, training, relu, dev):
    ins, ref = case_ref(name, training, relu)
    assert not relu or ref["guard"] >= GUARD, ref["guard"]
    got = run_fmt(ins, training, dev, relu)
    e = errors(got, ref)
    print(name, "train" if training else "eval", "relu" if relu else "lin", e, got["fwd"], got["bwd"], got["bwd_variant"])
    B, D = ins[0].shape[0], ins[1].shape[0]
    assert got["out"].dtype == torch.float32 and got["out"].shape == (B, D) + ins[0].shape[2:]
    assert got["gm"].shape == ins[0].shape and got["gm"].is_contiguous() and got["gw"].shape == ins[1].shape
    bar = OFFSET if name == "offset" else F32
    for k in ("out", "gm", "gg", "gb"):
        assert e[k] <= bar, (k, e[k])
    assert e["gw"] <= (OFFSET if name == "offset" else F32_GW), e["gw"]
    same_as_nchw(got, nchw_run(name, training, relu))
    assert got["fwd"] == (3 if training else 1) and got["bwd"] == 3
    assert got["fwd_variant"] == _name("fwd", "f32", training, relu, True)
    assert got["go_nchw"] == (name == "one_pixel")
    assert got["bwd_variant"] == _name("bwd", "f32", training, relu, not got["go_nchw"])


@pytest.mark.parametrize("relu", RELU)
@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("name", BF16_CASES)
def test_bf16_channels_last_both_ways(name, training, relu, dev):
    ins, ref = case_ref(name, training, relu, True)
    assert not relu or ref["guard"] >= GUARD, ref["guard"]
    got = run_fmt(ins, training, dev, relu, torch.bfloat16)
    e = errors(got, ref)
    print(name, "train" if training else "eval", "relu" if relu else "lin", e)
    assert got["out"].dtype == torch.bfloat16 and got["gm"].dtype == torch.bfloat16 and got["gw"].dtype == torch.float32
    assert e["out"] <= BF_OUT
    for k in KEYS:
        assert e[k] <= BF_GRAD, (k, e[k])
    same_as_nchw(got, nchw_run(name, training, relu, True))
    assert got["fwd_variant"] == _name("fwd", "bf16", training, relu, True)
    assert got["bwd_variant"] == _name("bwd", "bf16", training, relu, True)


@pytest.mark.parametrize("training", MODES)
def test_bf16_odd_d_pairs_straddle_the_pixel_rows(training, dev):
    """D = 5 in bf16: the second image starts on an odd element, so the dword pairs of the forward's stores straddle two
    pixels' rows and the span's first and last element stand alone.  Without the ReLU no guard is needed."""
    ins, ref = case_ref("tiny_d", training, False, True)
    got = run_fmt(ins, training, dev, False, torch.bfloat16)
    e = errors(got, ref)
    print("tiny_d bf16", "train" if training else "eval", e)
    assert e["out"] <= BF_OUT
    for k in KEYS:
        assert e[k] <= BF_GRAD, (k, e[k])
    same_as_nchw(got, nchw_run("tiny_d", training, False, True))


@pytest.mark.parametrize("D", [70, 67, 1])
def test_bf16_forward_over_several_tiles_of_even_and_odd_d(D, dev):
    """The forward's other store paths in bf16: D = 70, two tiles of an even D (pairs inside every segment); D = 67, two tiles
    of an odd D (single elements); D = 1 (the pair of two neighbouring pixels).  Eval, no ReLU: against the float64
    composition at the bf16 bar, and bit for bit with the NCHW call."""
    from neighbour_feature_pooling_amd import nfp_compress_map_tensors
    g = torch.Generator().manual_seed(100 + D)
    maps = torch.randn(3, 8, 5, 7, generator=g)
    w, gamma, beta = torch.randn(D, 8, 1, 1, generator=g) * 0.5, torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    rm, rv = torch.randn(D, generator=g) * 0.3, torch.rand(D, generator=g) + 0.5
    ref = reference64((maps, w, gamma, beta, rm, rv, torch.zeros(3, D, 5, 7)), False, False, torch.bfloat16)["out"]
    d = [t.to(dev) for t in (maps.bfloat16(), w, gamma, beta, rm, rv)]
    with torch.no_grad():
        plain = nfp_compress_map_tensors(*d, False, MOM, EPS, False)
        n0 = _count()
        got = nfp_compress_map_tensors(*d, False, MOM, EPS, False, memory_format=CL)
    assert _count() - n0 == 1 and _variant() == "cproj_fwd<bf16,eval,lin,nhwc>"
    assert got.is_contiguous(memory_format=CL) and torch.equal(got, plain)
    assert rel_err(_np(got), _np(ref)) <= BF_OUT


@pytest.mark.parametrize("training", MODES)
def test_the_backward_follows_the_layout_of_grad_out(training, dev):
    ins, ref = case_ref("n32_nonsquare", training)
    assert ref["guard"] >= GUARD
    plain = nchw_run("n32_nonsquare", training)
    for out_cl, go, bwd_nhwc in ((False, "cl", True), (True, "nchw", False), (True, "slice", False), (False, "slice", False)):
        got = run_fmt(ins, training, dev, out_cl=out_cl, go=go)
        assert got["fwd_variant"] == _name("fwd", "f32", training, True, out_cl), (out_cl, go)
        assert got["bwd_variant"] == _name("bwd", "f32", training, True, bwd_nhwc), (out_cl, go)
        same_as_nchw(got, plain)
        e = errors(got, ref)
        for k in ("out", "gm", "gg", "gb"):
            assert e[k] <= F32, (out_cl, go, k, e[k])
        assert e["gw"] <= F32_GW, (out_cl, go, e["gw"])
        assert got["bwd"] == 3


def test_a_bf16_grad_out_for_float32_maps_keeps_its_layout(dev):
    """The dtype cast in front of the kernels keeps a dense layout: a channels-last grad_out of another dtype still takes the
    channels-last kernels (called as autograd would call it)."""
    from neighbour_feature_pooling_amd.functional import cproj_backward_call, cproj_forward_call
    ins, _ = case_ref("common", True)
    maps, w, gamma, beta, rm, rv, g = (t.to(dev) for t in ins)
    w2 = w.reshape(32, 8).contiguous()
    _, saved = cproj_forward_call(maps, w2, gamma, beta, rm.clone(), rv.clone(), True, MOM, EPS, True)
    g16 = g.bfloat16().contiguous(memory_format=CL)
    a = cproj_backward_call(maps, w2, gamma, beta, None, None, saved, True, EPS, True, g16, (True,) * 4)
    assert _variant() == "cproj_bwd<f32,train,relu,nhwc>"
    b = cproj_backward_call(maps, w2, gamma, beta, None, None, saved, True, EPS, True, g16.float().contiguous(), (True,) * 4)
    assert _variant() == "cproj_bwd<f32,train,relu>"
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("relu", RELU)
@pytest.mark.parametrize("training", MODES)
def test_each_gradient_switched_off_in_turn(training, relu, dev):
    ins, _ = case_ref("n32_nonsquare", training, relu)
    full = run_fmt(ins, training, dev, relu)
    for off in range(4):
        want = tuple(i != off for i in range(4))
        got = run_fmt(ins, training, dev, relu, want=want)
        assert got[KEYS[off]] is None
        for i, k in enumerate(KEYS):
            if i != off:
                assert torch.equal(got[k], full[k]), (KEYS[off], k)
        assert got["bwd"] == (2 if off == 0 else 3)       # without grad_maps its kernel is skipped
        assert got["bwd_variant"] == _name("bwd", "f32", training, relu, True)
    got = run_fmt(ins, training, dev, relu, want=(True, False, False, False))
    assert torch.equal(got["gm"], full["gm"]) and got["bwd"] == (3 if training else 1)
    got = run_fmt(ins, training, dev, relu, want=(False,) * 4)
    assert torch.equal(got["out"], full["out"]) and got["bwd"] == 0
    assert got["fwd_variant"] == _name("fwd", "f32", training, relu, True)


@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("relu,inplace", [(True, "relu"), (True, "add"), (False, "add")])
def test_the_backward_does_not_read_the_output(relu, inplace, training, dev):
    ins, ref = case_ref("common", training, relu)
    plain = run_fmt(ins, training, dev, relu)
    got = run_fmt(ins, training, dev, relu, inplace=inplace)
    assert torch.equal(got["out"], plain["out"])
    for k in KEYS:
        assert torch.equal(got[k], plain[k]), k
    e = errors(got, ref)
    for k in ("gm", "gg", "gb"):
        assert e[k] <= F32, (k, e[k])
    assert e["gw"] <= F32_GW


@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("name", ["common", "chunked", "d_tiles"])
def test_two_runs_agree_bitwise(name, training, dev):
    ins, _ = case_ref(name, training)
    a, b = run_fmt(ins, training, dev), run_fmt(ins, training, dev)
    for k in ("out",) + KEYS + ("rm", "rv"):
        assert torch.equal(a[k], b[k]), k


def test_eval_rows_do_not_depend_on_the_batch(dev):
    shape, D, _, _ = CASES["common"]
    assert shape[0] == 4
    ins, _ = case_ref("common", False)
    full = run_fmt(ins, False, dev)
    part = run_fmt(tuple(t[:1] if i in (0, 6) else t for i, t in enumerate(ins)), False, dev)
    assert part["out"].shape[0] == 1
    assert torch.equal(part["out"][0], full["out"][0]) and torch.equal(part["gm"][0], full["gm"][0])


def test_the_switch_and_the_default_routing_for_channels_last(dev, monkeypatch):
    from neighbour_feature_pooling_amd import functional, nfp_compress_map_tensors
    ins, _ = case_ref("common", True)
    d = [t.to(dev) for t in ins]

    def call(maps, training=True):
        n0 = _count()
        out = nfp_compress_map_tensors(maps, d[1], d[2], d[3], d[4].clone(), d[5].clone(), training, MOM, EPS, memory_format=CL)
        assert out.is_contiguous(memory_format=CL) and not out.is_contiguous()
        return out, _count() - n0

    hip, k = call(d[0])
    assert k == 3 and _variant() == "cproj_fwd<f32,train,relu,nhwc>"
    monkeypatch.setenv("NFP_CPROJ_TORCH", "1")          # the composition, converted
    host, k = call(d[0])
    assert k == 0 and rel_err(_np(hip), _np(host)) <= 1e-4
    monkeypatch.delenv("NFP_CPROJ_TORCH")               # the default: what DESIGN 4g's channels-last table shows faster
    assert d[0].shape[0] * 49 < functional.CPROJ_ROUTED_NHWC_TRAIN_PIXELS
    assert call(d[0])[1] == 0                           # a small train-mode step: the composition
    with torch.no_grad():                               # the forward on running statistics, no backward: the kernel
        assert call(d[0], False)[1] == 1 and _variant() == "cproj_fwd<f32,eval,relu,nhwc>"
    big = torch.randn(256, 8, 12, 12, device=dev)       # the smallest train-mode class that measured faster
    assert call(big)[1] == 3 and _variant() == "cproj_fwd<f32,train,relu,nhwc>"


def test_insert_with_preserve_format_follows_a_channels_last_input(dev):
    from neighbour_feature_pooling_amd import NFPInsert
    torch.manual_seed(0)
    a = NFPInsert(16).to(dev)
    torch.manual_seed(0)
    b = NFPInsert(16, memory_format=torch.preserve_format).to(dev)
    x = torch.randn(4, 16, 9, 9, device=dev).contiguous(memory_format=CL)
    want = a(x)
    assert _variant() == "cproj_fwd<f32,train,relu>"
    xb = x.clone().requires_grad_(True)
    got = b(xb)
    assert _variant() == "cproj_fwd<f32,train,relu,nhwc>"
    assert got.shape == (4, 16, 7, 7) and got.is_contiguous(memory_format=CL) and not got.is_contiguous()
    assert rel_err(_np(got), _np(want)) <= F32
    got.backward(torch.randn(4, 16, 7, 7, device=dev).contiguous(memory_format=CL))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xb.grad).all()) and float(b.nfp_proj[0].weight.grad.abs().max()) > 0
    assert b(x.contiguous()).is_contiguous()                 # an NCHW input: an NCHW map
    assert _variant() == "cproj_fwd<f32,train,relu>"


def test_bottleneck_in_channels_last(dev):
    from neighbour_feature_pooling_amd import NFPBottleneck
    torch.manual_seed(0)
    a = NFPBottleneck(16, 32).to(dev)
    torch.manual_seed(0)
    b = NFPBottleneck(16, 32, fused_project=True, memory_format=CL).to(dev)
    x = torch.randn(4, 16, 9, 9, device=dev).contiguous(memory_format=CL)
    want = a(x)
    xb = x.clone().requires_grad_(True)
    seen = []
    hook = b.relu.register_forward_hook(lambda m, i, o: seen.append(_variant()))
    got = b(xb)
    hook.remove()
    assert seen[-1] == "cproj_fwd<f32,train,lin,nhwc>"
    assert got.shape == (4, 32, 7, 7) and got.is_contiguous(memory_format=CL) and not got.is_contiguous()
    assert rel_err(_np(got), _np(want)) <= F32
    got.backward(torch.randn(4, 32, 7, 7, device=dev).contiguous(memory_format=CL))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xb.grad).all()) and float(b.conv2.weight.grad.abs().max()) > 0
