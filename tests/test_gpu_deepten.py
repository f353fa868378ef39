"""DeepTENEncoding on the MI355X: the kernels of csrc/nfp_deepten.hip (include/nfp.h nfp_deepten_*) against the reference's
fixtures (tests/golden/deepten_*.npz) and the float64 torch formulation on the GPU — spread and saturated assignments, K = 1,
NaN, determinism, nullable gradients, poisoned buffers and LDS, the calls that take the torch formulation instead, CUDA-graph
replay and the nets.

The bar (test_deepten_host.py): err = max|got - ref64| / max|ref64| <= max(4 * err32, 2e-6), err32 from `_host.deepten_host`
in float32 (or the fixture's float32 arrays).  bf16 x: out and grad_x are one rounding of a float32 value —
one_rounding_excess(got, ref64 of the bf16-rounded inputs, slack = that float32 bar) <= 1; the parameter gradients, float32
sums over exactly representable inputs, keep the float32 bar."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases_deepten as KD
import poison as P
from conftest import rel_err, same_nan_pattern
from one_rounding import one_rounding_excess
from test_deepten_host import NAMES, bar, check_under_the_bar, deepten_module, run_module

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAYOUTS = ("nchw", "nhwc", "tok")


@pytest.fixture(scope="module", autouse=True)
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from neighbour_feature_pooling_amd import _abi
    _abi.load()
    return torch.device(DEV)


def _lib():
    from neighbour_feature_pooling_amd import _abi
    return _abi.load()


def _count():
    return _lib().nfp_launch_count()


def _variant():
    return _lib().nfp_last_variant().decode()


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


def _lay(x, layout):
    """A dense NCHW x in the layout asked for: "nhwc" channels-last; "tok" the patch tokens of a [B,1+N,D] buffer behind a
    class token, viewed as [B,D,H,W] (models.NFPNet): channels-last images a batch stride of (1+N)*D apart."""
    B, D, H, W = x.shape
    if layout == "nchw":
        return x.contiguous()
    if layout == "nhwc":
        return x.contiguous(memory_format=torch.channels_last)
    buf = torch.full((B, 1 + H * W, D), 7.0, dtype=x.dtype, device=x.device)
    buf[:, 1:] = x.flatten(2).transpose(1, 2)
    v = buf[:, 1:].transpose(1, 2).unflatten(2, (H, W))
    assert B == 1 or v.stride(0) == (1 + H * W) * D
    return v


def _op(x, cw, sc, go, want=(True, True, True)):
    """(out, grad_x, grad_codewords, grad_scale) of nfp_deepten_encode, None where no gradient was asked for."""
    from neighbour_feature_pooling_amd import nfp_deepten_encode
    ins = [t.detach().requires_grad_(r) for t, r in zip((x, cw.clone(), sc.clone()), want)]
    out = nfp_deepten_encode(*ins)
    asked = [t for t in ins if t.requires_grad]
    grads = iter(torch.autograd.grad(out, asked, go.to(out.dtype)) if asked else ())
    return (out.detach(),) + tuple(next(grads) if r else None for r in want)


def _host(x, cw, sc, go, dtype):
    """The same four from `_host.deepten_host` in `dtype` on the device."""
    from neighbour_feature_pooling_amd._host import deepten_host
    ins = [t.detach().to(dtype).requires_grad_(True) for t in (x, cw, sc)]
    out = deepten_host(*ins)
    return (out.detach(),) + torch.autograd.grad(out, ins, go.to(dtype))


def _inputs(shape, K, kind, bf, seed):
    """x (rounded to bf16 where asked, kept float32), codewords 0.5 N(0,1), scale -U(0,1) 16/D, grad_out (rounded likewise)."""
    B, D, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    x = torch.relu(x) if kind == "relu" else x
    cw = 0.5 * torch.randn(K, D, generator=g)
    sc = -torch.rand(K, generator=g) * 16.0 / D
    go = torch.randn(B, K * D, generator=g)
    if bf:
        x, go = x.bfloat16().float(), go.bfloat16().float()
    return tuple(t.to(DEV) for t in (x, cw, sc, go))


def _check(got, ref64, ref32, bf, label, names=NAMES):
    """The file comment's bars; got / ref64 / ref32 in NAMES order (device tensors or numpy)."""
    got, ref64, ref32 = ([_np(t) if isinstance(t, torch.Tensor) else t for t in r] for r in (got, ref64, ref32))
    if not bf:
        check_under_the_bar(got, ref64, ref32, label, names)
        return
    for i, n in enumerate(NAMES):
        if n not in names:
            continue
        e32 = rel_err(ref32[i].reshape(-1), ref64[i].reshape(-1))
        if n in ("out", "grad_x"):
            ex = one_rounding_excess(got[i].reshape(-1), ref64[i].reshape(-1), slack=bar(e32))
            print(f"{label} {n}: one-rounding excess {ex:.3f} (float32 bar {bar(e32):.3e})")
            assert ex <= 1.0, (label, n, ex)
        else:
            err = rel_err(got[i].reshape(-1), ref64[i].reshape(-1))
            print(f"{label} {n}: err {err:.3e} err32 {e32:.3e} bar {bar(e32):.3e}")
            assert err <= bar(e32), (label, n, err, e32)


# ---- (a) the reference's fixtures through the module ------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", [c["name"] for c in KD.DEEPTEN_CASES])
def test_fixture_through_the_module(name, layout):
    c = KD.DEEPTEN_BY_NAME[name]
    m, g = deepten_module(c)
    m = m.to(DEV)
    x = _lay(torch.from_numpy(KD.make_x(c)).to(DEV), layout)
    n0 = _count()
    got = run_module(m, x, torch.from_numpy(KD.make_grad_out(c)).to(DEV))
    torch.cuda.synchronize()
    assert _count() - n0 == 5                       # two launches forward, three backward
    assert _variant().startswith("dten_bwd<f32,"), _variant()
    check_under_the_bar(got, g, g, f"{name} {layout}")


# ---- (b) spread assignments against the float64 formulation on the GPU -------------------------------------------------------
SPREAD = [((3, 20, 3, 3), 5), ((2, 37, 5, 3), 7), ((2, 192, 14, 14), 32), ((2, 512, 7, 7), 32), ((2, 520, 5, 5), 33),
          ((2, 64, 4, 4), 64), ((2, 1030, 2, 3), 32), ((2, 960, 7, 7), 32)]
SPREAD_IDS = ["x".join(map(str, s)) + f"k{k}" for s, k in SPREAD]


@functools.lru_cache(maxsize=None)
def _spread_case(i, bf):
    """Inputs and both references of SPREAD[i], computed once and shared by the layouts (never written to)."""
    shape, K = SPREAD[i]
    # x ~ N(0,1) or relu of it, turn about — but relu for both small maps, whose few channels (16 / D large) saturate under N(0,1)
    ins = _inputs(shape, K, "relu" if i % 2 or i < 2 else "normal", bf, 510 + i)
    ref64, ref32 = _host(*ins, torch.float64), _host(*ins, torch.float32)
    x, cw, sc, _ = (t.double() for t in ins)
    dist = ((x.flatten(2).transpose(1, 2).unsqueeze(2) - cw) ** 2).sum(3)
    spread = float(torch.softmax(-sc * dist, dim=2).max(dim=2).values.mean())
    return ins, tuple(_np(t) for t in ref64), tuple(_np(t) for t in ref32), spread


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(SPREAD)), ids=SPREAD_IDS)
def test_spread_assignments_match_float64(i, dt, layout):
    bf = dt == "bf16"
    (x, cw, sc, go), ref64, ref32, spread = _spread_case(i, bf)
    print(SPREAD_IDS[i], dt, "mean max_k A", spread)
    assert spread < 0.95                            # (not saturated: every codeword's terms are exercised)
    xin = _lay(x.bfloat16() if bf else x, layout)
    n0 = _count()
    got = _op(xin, cw, sc, go)
    torch.cuda.synchronize()
    assert _count() - n0 == 5
    assert _variant() == f"dten_bwd<{dt},{'nchw' if layout == 'nchw' else 'nhwc'}>", _variant()
    assert got[0].dtype == xin.dtype and got[1].dtype == xin.dtype and got[1].shape == xin.shape
    assert got[2].dtype == got[3].dtype == torch.float32
    _check(got, ref64, ref32, bf, f"{SPREAD_IDS[i]} {dt} {layout}")


# ---- (c) saturated logits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,K,kind,mul", [((2, 64, 4, 4), 8, "normal", 4.0), ((2, 512, 7, 7), 32, "relu", 1.0)],
                         ids=["2x64x4x4k8_x4", "2x512x7x7k32_relu"])
def test_saturated_logits(shape, K, kind, mul):
    from neighbour_feature_pooling_amd import DeepTENEncoding
    B, D, H, W = shape
    torch.manual_seed(31)
    m = DeepTENEncoding(D, K)                        # fresh init: |scale| up to 1, no 16 / D
    x, _, _, go = _inputs(shape, K, kind, False, 600)
    x = x * mul
    cw, sc = m.codewords.detach().to(DEV), m.scale.detach().to(DEV)
    got = _op(x, cw, sc, go)
    for t in got:
        assert torch.isfinite(t).all()
    ref64, ref32 = _host(x, cw, sc, go, torch.float64), _host(x, cw, sc, go, torch.float32)
    _check(got, ref64, ref32, False, "saturated", names=NAMES[:3])
    # grad_scale: in float32 the value itself is cancellation noise here (the reference's too): its error is measured against
    # the size of the terms it is summed from, sum_{b,n} A (|dA| + sum_k A |dA|) dist in float64
    xd, cd, sd = x.double(), cw.double(), sc.double()
    r = xd.flatten(2).transpose(1, 2).unsqueeze(2) - cd                                   # [B,N,K,D]
    dist = (r ** 2).sum(3)
    A = torch.softmax(-sd * dist, dim=2)
    dA = (go.double().view(B, 1, K, D) * r).sum(3)
    size = float((A * (dA.abs() + (A * dA.abs()).sum(2, keepdim=True)) * dist).sum((0, 1)).max())
    err = float((got[3].double() - ref64[3]).abs().max()) / size
    e32 = float((ref32[3].double() - ref64[3]).abs().max()) / size
    print(f"saturated grad_scale: err {err:.3e} err32 {e32:.3e} bar {bar(e32):.3e} (mean max_k A "
          f"{float(A.max(2).values.mean()):.4f})")
    assert err <= bar(e32)


# ---- (d) one codeword --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_one_codeword_has_no_scale_gradient(layout):
    x, cw, sc, go = _inputs((3, 20, 3, 3), 1, "normal", False, 700)
    got = _op(_lay(x, layout), cw, sc, go)
    assert torch.equal(got[3], torch.zeros_like(got[3]))
    _check(got, _host(x, cw, sc, go, torch.float64), _host(x, cw, sc, go, torch.float32), False, "K=1", names=NAMES[:3])


# ---- (e) NaN -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "tok"])
def test_nan_stays_in_its_image(layout):
    """A NaN in one element of image 1: that image's out is NaN throughout and its grad_x NaN where the reference's is (the
    pixel of the NaN — the pixels of an image meet only in the sums over n); images 0 and 2 keep their bits; the parameter
    gradients, sums over the batch, are NaN as the reference's are."""
    x, cw, sc, go = _inputs((3, 37, 5, 3), 7, "normal", False, 800)
    clean = _op(_lay(x, layout), cw, sc, go)
    x[1, 3, 2, 1] = float("nan")
    got = _op(_lay(x, layout), cw, sc, go)
    ref = _host(x, cw, sc, go, torch.float64)
    assert torch.isnan(got[0][1]).all() and torch.isnan(got[1][1]).any() and torch.isnan(got[1][1, :, 2, 1]).all()
    for a, r in zip(got, ref):
        assert same_nan_pattern(_np(a), _np(r))
    assert torch.isnan(got[2]).all() and torch.isnan(got[3]).all()
    for b in (0, 2):
        assert torch.equal(got[0][b], clean[0][b]) and torch.equal(got[1][b], clean[1][b])


# ---- (f) determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "tok"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,K", [((5, 192, 14, 14), 32), ((5, 37, 5, 3), 7)], ids=["5x192x14x14k32", "5x37x5x3k7"])
def test_bitwise_reproducible_and_independent_of_the_batch(shape, K, dt, layout):
    x, cw, sc, go = _inputs(shape, K, "normal", dt == torch.bfloat16, 900)
    x = x.to(dt)
    one, two = _op(_lay(x, layout), cw, sc, go), _op(_lay(x, layout), cw, sc, go)
    for a, c in zip(one, two):
        assert torch.equal(a, c)
    for i in (0, 3, 4):
        alone = _op(_lay(x[i:i + 1], layout), cw, sc, go[i:i + 1])
        assert torch.equal(alone[0][0], one[0][i])
        assert torch.equal(alone[1][0], one[1][i])


# ---- (g) unused gradients ----------------------------------------------------------------------------------------------------
class _Spy:
    """`torch` with `empty` recorded (the seam tests/poison.py uses)."""

    def __init__(self):
        self.shapes = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, **kwargs):
        t = torch.empty(*args, **kwargs)
        self.shapes.append(tuple(t.shape))
        return t


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_unused_gradients_are_neither_allocated_nor_computed(dt, monkeypatch):
    from neighbour_feature_pooling_amd import functional, nfp_deepten_encode
    shape, K = (4, 37, 5, 3), 7
    B, D, N = shape[0], shape[1], shape[2] * shape[3]
    x, cw, sc, go = _inputs(shape, K, "normal", dt == torch.bfloat16, 1000)
    x = x.to(dt)
    full = _op(x, cw, sc, go)
    L = _lib()
    w_only, w_and_partials = L.nfp_deepten_scratch_floats(B, N, K, D, 0), L.nfp_deepten_scratch_floats(B, N, K, D, 1)
    assert w_only == B * N * K < w_and_partials

    def spied(want):
        spy = _Spy()
        monkeypatch.setattr(functional, "torch", spy)
        n0 = _count()
        got = _op(x, cw, sc, go, want)
        torch.cuda.synchronize()
        monkeypatch.setattr(functional, "torch", torch)
        return got, _count() - n0, spy.shapes

    got, launches, shapes = spied((True, False, False))              # frozen parameters: no partials, no reduce
    assert launches == 2 + 2
    assert (K, D) not in shapes and (K,) not in shapes and (w_and_partials,) not in shapes and (w_only,) in shapes
    assert got[2] is None and got[3] is None and torch.equal(got[1], full[1]) and torch.equal(got[0], full[0])
    got, launches, shapes = spied((False, True, True))               # x takes no gradient
    assert launches == 2 + 3
    assert tuple(x.shape) not in shapes and (K, D) in shapes and (K,) in shapes and (w_and_partials,) in shapes
    assert got[1] is None and torch.equal(got[2], full[2]) and torch.equal(got[3], full[3])
    got, launches, shapes = spied((False, False, True))              # the scale alone: no pass over x's channel chunks
    assert launches == 2 + 2
    assert tuple(x.shape) not in shapes and (K, D) not in shapes
    assert torch.equal(got[3], full[3])
    got, launches, shapes = spied((True, True, False))
    assert launches == 2 + 3 and (K,) not in shapes
    assert torch.equal(got[1], full[1]) and torch.equal(got[2], full[2])
    n0 = _count()
    with torch.no_grad():
        out = nfp_deepten_encode(x.requires_grad_(True), cw, sc)
    assert _count() - n0 == 2 and torch.equal(out, full[0])
    assert _variant() == f"dten_fwd<{'bf16' if dt == torch.bfloat16 else 'f32'},nchw>"


# ---- (h) poisoned buffers, fenced inputs, poisoned LDS -------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape,K", [((3, 20, 3, 3), 5), ((2, 520, 5, 5), 33), ((2, 192, 14, 14), 32)],
                         ids=["3x20x3x3k5", "2x520x5x5k33", "2x192x14x14k32"])
def test_poisoned_buffers_and_fenced_inputs(shape, K, dt, layout):
    from neighbour_feature_pooling_amd import nfp_deepten_encode
    bf = dt == "bf16"
    x0, cw0, sc0, go0 = _inputs(shape, K, "normal", bf, 1100)
    x0 = _lay(x0.bfloat16() if bf else x0, layout)

    def case(poison):
        x, cw, sc = poison.fenced(x0).requires_grad_(True), poison.fenced(cw0).requires_grad_(True), \
            poison.fenced(sc0).requires_grad_(True)
        assert x.stride() == x0.stride()
        out = nfp_deepten_encode(x, cw, sc)
        fv = _variant()
        gx, gc, gs = torch.autograd.grad(out, (x, cw, sc), poison.fenced(go0.to(out.dtype)))
        return dict(out=out.detach(), gx=gx, gc=gc, gs=gs, fv=fv, bv=_variant())

    zero = P.run_fills(case, f"deepten {shape} K{K} {dt} {layout}")
    assert zero["fv"].startswith(f"dten_fwd<{dt},") and zero["bv"].startswith(f"dten_bwd<{dt},")
    xf = x0.float()
    _check((zero["out"], zero["gx"], zero["gc"], zero["gs"]), _host(xf, cw0, sc0, go0, torch.float64),
           _host(xf, cw0, sc0, go0, torch.float32), bf, f"poison {shape} {dt} {layout}")


def test_smallest_spread_cases_with_poisoned_lds():
    """(b)'s three smallest shapes once more on the -DNFP_LDS_POISON build (libnfp_hip_poison.so), in a fresh process: every
    word of a workgroup's LDS is a signalling NaN before the kernel proper starts."""
    if os.environ.get("NFP_TEST_LIB"):
        pytest.skip("this IS the run on the test build")
    env = dict(os.environ, NFP_TEST_LIB="libnfp_hip_poison.so")
    sel = "spread_assignments and (3x20x3x3k5 or 2x37x5x3k7 or 2x64x4x4k64)"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", sel,
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and "18 passed" in r.stdout, tail


# ---- (i) the calls that take the torch formulation ----------------------------------------------------------------------------
def test_fallbacks_take_the_composition(monkeypatch):
    from neighbour_feature_pooling_amd import nfp_deepten_encode
    x, cw, sc, go = _inputs((2, 37, 5, 3), 7, "relu", False, 511)         # ((b)'s inputs of this shape: spread assignments)
    ref64 = _host(x, cw, sc, go, torch.float64)
    hip = _op(x, cw, sc, go)
    n0 = _count()
    for xi, tol in ((x.cpu(), 1e-5), (x.half(), 2e-2), (x.double(), 1e-12), (x[..., ::2], None)):
        pdt = torch.float64 if xi.dtype == torch.float64 else torch.float32
        ci, si = cw.to(xi.device, pdt).requires_grad_(True), sc.to(xi.device, pdt).requires_grad_(True)
        out = nfp_deepten_encode(xi.requires_grad_(True), ci, si)
        assert out.dtype == xi.dtype and out.device == xi.device
        torch.autograd.grad(out, (xi, ci, si), torch.ones_like(out))
        if tol is not None:
            assert rel_err(_np(out), _np(ref64[0])) <= tol
    x65, cw65, sc65, go65 = _inputs((2, 20, 3, 3), 65, "normal", False, 1201)          # K = 65
    for a, b in zip(_op(x65, cw65, sc65, go65), _host(x65, cw65, sc65, go65, torch.float32)):
        assert torch.equal(a, b)
    monkeypatch.setenv("NFP_DEEPTEN_TORCH", "1")                                       # read at call time
    env = _op(x, cw, sc, go)
    monkeypatch.delenv("NFP_DEEPTEN_TORCH")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ac = nfp_deepten_encode(x, cw, sc)
    assert _count() == n0                                                              # no NFP kernel ran
    assert ac.dtype == torch.float32                 # (the reference's output type there: softmax and sum are float32 ops)
    host32 = _host(x, cw, sc, go, torch.float32)
    for a, b in zip(env, host32):
        assert torch.equal(a, b)
    _check(env, ref64, host32, False, "NFP_DEEPTEN_TORCH=1")
    _check(hip, ref64, host32, False, "hip")
    assert _count() - n0 == 0
    _op(x, cw, sc, go)
    assert _count() - n0 == 5


def test_torch_compile_fullgraph_matches_eager():
    c = KD.DEEPTEN_BY_NAME["deepten_2x37x5x3_k7"]
    m, g = deepten_module(c)
    m = m.to(DEV)
    x, go = torch.from_numpy(KD.make_x(c)).to(DEV), torch.from_numpy(KD.make_grad_out(c)).to(DEV)
    eager = run_module(m, x, go)
    torch._dynamo.reset()
    n0 = _count()
    compiled = run_module(torch.compile(m, fullgraph=True), x, go)
    assert _count() == n0                           # (traced as ATen ops: no NFP kernel)
    # two float32 evaluations of the same formulas, each allowed the bar from the float64 result: apart by at most two bars
    for u, v, n in zip(eager, compiled, NAMES):
        tol = 2 * bar(rel_err(g[n].reshape(-1), g[n + "_64"].reshape(-1)))
        err = rel_err(v.reshape(-1), u.reshape(-1))
        print(f"compiled against eager {n}: {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol, n


# ---- (j) an empty batch -------------------------------------------------------------------------------------------------------
def test_empty_batch():
    from neighbour_feature_pooling_amd import nfp_deepten_encode
    x, cw, sc, _ = _inputs((2, 20, 3, 3), 5, "normal", False, 1300)
    n0 = _count()
    xe, ce, se = x[:0].requires_grad_(True), cw.requires_grad_(True), sc.requires_grad_(True)
    out = nfp_deepten_encode(xe, ce, se)
    assert out.shape == (0, 100) and out.dtype == torch.float32 and out.is_cuda
    out.sum().backward()
    assert torch.equal(ce.grad, torch.zeros_like(ce)) and torch.equal(se.grad, torch.zeros_like(se))
    assert xe.grad.shape == xe.shape and _count() == n0


# ---- (k) CUDA-graph replay ----------------------------------------------------------------------------------------------------
def test_cuda_graph_replay_of_a_no_grad_forward_matches_eager():
    c = KD.DEEPTEN_BY_NAME["deepten_2x64x5x5_k32"]
    m, _ = deepten_module(c)
    m = m.to(DEV)
    x = torch.from_numpy(KD.make_x(c)).to(DEV)
    with torch.no_grad():
        ref = m(x).clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):            # eager warm-up on the capture stream
                m(x)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(x)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, ref)


# ---- (l) the nets -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone,image,layout", [("resnet18", 64, "nchw"), ("vit_tiny_patch16_224", 64, "nhwc")])
def test_deepten_net_train_step(backbone, image, layout):
    from neighbour_feature_pooling_amd import train
    torch.manual_seed(0)
    net = train.build(backbone, num_classes=5, image=image, device=DEV, pooling="deepten", num_codes=8)
    step, _ = train.make_step(net)
    x, y = train.synthetic_batch(4, 3, image, 5, DEV, torch.float32, seed=1)
    before = net.encoding.codewords.detach().clone()
    n0 = _count()
    loss = float(step(x, y))
    torch.cuda.synchronize()
    assert _count() - n0 == 5 and _variant() == f"dten_bwd<f32,{layout}>", (_count() - n0, _variant())
    assert np.isfinite(loss) and np.isfinite(float(step(x, y)))
    assert not torch.equal(before, net.encoding.codewords.detach())
