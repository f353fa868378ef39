"""SimilarityAwarePooling on the MI355X: the softmax-pool tail kernels (csrc/nfp_attpool.hip, include/nfp.h nfp_attpool_*)
against the reference's fixtures (tests/golden/sap_*.npz) and the float64 torch formulation on the same maps, peaked
logits, NaN, determinism, nullable gradients, the module end to end and the calls that take the torch tail instead.
Bars: 1e-5 of each tensor's max magnitude for float32; 1e-2 (pooled) / 2e-2 (gradients) for bf16 on the same bf16-rounded
inputs; |grad_b| <= bar * max|grad_w| (grad_b is zero in exact arithmetic)."""
import numpy as np
import pytest
import torch

import cases as K
import cases_sap as KS
from conftest import rel_err, same_nan_pattern
from test_sap_host import check_against_fixture, run_sap, sap_module

pytestmark = pytest.mark.gpu

F32, BF_OUT, BF_GRAD = 1e-5, 1e-2, 2e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from neighbour_feature_pooling_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


def _lib():
    from neighbour_feature_pooling_amd import _abi
    return _abi.load()


def _count():
    return _lib().nfp_launch_count()


def _variant():
    return _lib().nfp_last_variant().decode()


def _inputs(B, N, P, dtype, seed=0, dev="cuda:0"):
    """maps [B,N,P] (rounded to dtype), w [N], b [1], grad_pooled [B,N] — seeded, on the device."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 3 * N + P)
    maps = torch.randn(B, N, P, generator=g).to(dtype).to(dev)
    w = (torch.randn(N, generator=g) * 0.5).to(dev)
    b = torch.randn(1, generator=g).to(dev)
    gp = torch.randn(B, N, generator=g).to(dev)
    return maps, w, b, gp


def _hip(maps, w, b, gp, want=(True, True, True)):
    """(pooled, grad_maps, grad_w, grad_b) of the op, None where no gradient was asked for; all on the device."""
    from neighbour_feature_pooling_amd import nfp_attention_pool
    ins = [t.detach().clone().requires_grad_(r) for t, r in zip((maps, w, b), want)]
    pooled = nfp_attention_pool(*ins)
    asked = [t for t in ins if t.requires_grad]
    grads = iter(torch.autograd.grad(pooled, asked, gp.to(pooled.dtype)))
    return (pooled.detach(),) + tuple(next(grads) if r else None for r in want)


def _ref64(maps, w, b, gp):
    """The same four from the float64 torch formulation on the CPU, on the maps as they are (already rounded)."""
    from neighbour_feature_pooling_amd._host import attention_pool_host
    ins = [t.detach().double().cpu().requires_grad_(True) for t in (maps, w, b)]
    pooled = attention_pool_host(*ins)
    return (pooled.detach(),) + torch.autograd.grad(pooled, ins, gp.double().cpu())


def _np(t):
    return t.detach().double().cpu().numpy()


def _check(got, ref, bf, label=""):
    tol_out, tol_g = (BF_OUT, BF_GRAD) if bf else (F32, F32)
    errs = dict(pooled=rel_err(_np(got[0]), _np(ref[0])), grad_maps=rel_err(_np(got[1]), _np(ref[1])),
                grad_w=rel_err(_np(got[2]), _np(ref[2])), grad_b=float(np.abs(_np(got[3])).max()),
                grad_b_bar=tol_g * float(np.abs(_np(ref[2])).max()))
    print(label, errs)
    assert errs["pooled"] <= tol_out
    assert errs["grad_maps"] <= tol_g
    assert errs["grad_w"] <= tol_g
    assert errs["grad_b"] <= errs["grad_b_bar"]
    return errs


# ---- 1. the reference's fixtures through the module ------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in KS.SAP_CASES])
def test_fixture_through_the_module(name, dev):
    c = KS.SAP_BY_NAME[name]
    m, g = sap_module(c)
    m = m.to(dev)
    x = torch.from_numpy(K.make_input(c)).to(dev).requires_grad_(True)
    # launches of the layer alone, each way
    n0 = _count()
    maps = m.nfp(x)
    k_fwd = _count() - n0
    go = torch.ones_like(maps)
    n0 = _count()
    torch.autograd.grad(maps, x, go)
    k_bwd = _count() - n0
    # the module: the layer's launches plus 1 forward, plus 2 backward (the tail's backward and the batch reduce)
    m.zero_grad(set_to_none=True)
    n0 = _count()
    pooled = m(x)
    assert _count() - n0 == k_fwd + 1
    assert _variant() == "attpool_fwd<f32>", _variant()
    gp = torch.from_numpy(KS.make_grad_pooled(c, pooled.shape[1])).to(dev)
    n0 = _count()
    pooled.backward(gp)
    torch.cuda.synchronize()
    assert _count() - n0 == k_bwd + 2
    got = tuple(t.detach().float().cpu().numpy() for t in (pooled, x.grad, m.att_proj.weight.grad, m.att_proj.bias.grad))
    check_against_fixture(got, g, F32)
    # att_proj frozen: the tail's backward alone
    m.att_proj.requires_grad_(False)
    x.grad = None
    pooled = m(x)
    n0 = _count()
    pooled.backward(gp)
    torch.cuda.synchronize()
    assert _count() - n0 == k_bwd + 1
    assert m.att_proj.weight.grad is None or torch.equal(m.att_proj.weight.grad.cpu(), torch.from_numpy(got[2]))
    assert np.array_equal(x.grad.cpu().numpy(), got[1])


def test_fixtures_once_more_via_run_sap(dev):
    """(the same entry the CPU test uses, on the device: bias=True layer, channels-last x)"""
    c = KS.SAP_BY_NAME["sap_cos_bias_2x8x7x6"]
    m, g = sap_module(c)
    check_against_fixture(run_sap(m.to(dev), c, dev=dev, channels_last=True), g, F32)


# ---- 2. the op against the float64 formulation on the same maps ------------------------------------------------------------
SHAPES = [(1, 8, 1), (2, 8, 25), (3, 24, 30), (2, 8, 63), (2, 8, 64), (2, 8, 65), (2, 32, 196), (2, 48, 1), (3, 8, 1122),
          (2, 8, 12100), (65, 24, 100), (300, 8, 25)]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B,N,P", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_op_matches_float64_formulation(B, N, P, dt, dev):
    bf = dt == "bf16"
    maps, w, b, gp = _inputs(B, N, P, torch.bfloat16 if bf else torch.float32)
    n0 = _count()
    got = _hip(maps, w, b, gp)
    torch.cuda.synchronize()
    assert _count() - n0 == 3                                   # forward, backward, batch reduce
    assert _variant() == f"attpool_bwd<{dt}>", _variant()
    assert got[0].dtype == maps.dtype and got[1].dtype == maps.dtype and got[2].dtype == torch.float32
    _check(got, _ref64(maps, w, b, gp), bf, f"({B},{N},{P}) {dt}")


# ---- 3. peaked logits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,P", [(2, 8, 25), (3, 8, 1122), (2, 8, 12100)])
def test_peaked_logits(B, N, P, dev):
    maps, w, b, gp = _inputs(B, N, P, torch.float32, seed=1)
    logits = (maps.double() * w.double().reshape(1, N, 1)).sum(1)
    w = (w.double() * (80.0 / logits.abs().max())).float()       # l spans +-80
    b = torch.zeros_like(b)
    got = _hip(maps, w, b, gp)
    for t in got:
        assert torch.isfinite(t).all()
    _check(got, _ref64(maps, w, b, gp), False, f"peaked ({B},{N},{P})")


# ---- 4. NaN ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [30, 12100])
def test_nan_stays_in_its_image(P, dev):
    maps, w, b, gp = _inputs(3, 8, P, torch.float32, seed=2)
    maps[1, 3, 7] = float("nan")
    got = _hip(maps, w, b, gp)
    ref = _ref64(maps, w, b, gp)
    pooled = _np(got[0])
    assert np.isnan(pooled[1]).all() and np.isfinite(pooled[[0, 2]]).all()
    for a, r in zip(got, ref):
        assert same_nan_pattern(_np(a), _np(r))
    assert rel_err(pooled[[0, 2]], _np(ref[0])[[0, 2]]) <= F32
    assert rel_err(_np(got[1])[[0, 2]], _np(ref[1])[[0, 2]]) <= F32


# ---- 5. determinism --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,P", [(24, 100), (8, 12100)])
def test_bitwise_reproducible_and_independent_of_the_batch(N, P, dt, dev):
    maps, w, b, gp = _inputs(5, N, P, dt, seed=3)
    one, two = _hip(maps, w, b, gp), _hip(maps, w, b, gp)
    for a, c in zip(one, two):
        assert torch.equal(a, c)
    for i in (0, 3, 4):
        alone = _hip(maps[i:i + 1].contiguous(), w, b, gp[i:i + 1].contiguous())
        assert torch.equal(alone[0][0], one[0][i])
        assert torch.equal(alone[1][0], one[1][i])


# ---- 6. nullable gradients -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_unused_gradients_are_not_computed(dt, dev):
    maps, w, b, gp = _inputs(4, 24, 100, dt, seed=4)
    full = _hip(maps, w, b, gp)
    n0 = _count()
    params = _hip(maps, w, b, gp, want=(False, True, True))       # the maps take no gradient
    assert _count() - n0 == 3
    assert params[1] is None and torch.equal(params[2], full[2]) and torch.equal(params[3], full[3])
    n0 = _count()
    frozen = _hip(maps, w, b, gp, want=(True, False, False))      # att_proj frozen: no partials, no reduce
    assert _count() - n0 == 2
    assert frozen[2] is None and frozen[3] is None and torch.equal(frozen[1], full[1])
    only_w = _hip(maps, w, b, gp, want=(True, True, False))
    assert torch.equal(only_w[2], full[2]) and torch.equal(only_w[1], full[1])
    from neighbour_feature_pooling_amd import nfp_attention_pool
    n0 = _count()
    with torch.no_grad():                                         # no backward will follow: att is not written
        out = nfp_attention_pool(maps.requires_grad_(True), w, b)
    assert _count() - n0 == 1 and torch.equal(out, full[0])


# ---- 7. the module end to end ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("ctor", [dict(R=1, measure="cosine"), dict(R=1, measure="norm", p=2)], ids=["cos", "l2"])
@pytest.mark.parametrize("shape", [(4, 64, 7, 7), (2, 8, 30, 30)], ids=["4x64x7x7", "2x8x30x30"])
def test_module_end_to_end(shape, ctor, cl, dt, dev):
    from neighbour_feature_pooling_amd import SimilarityAwarePooling
    bf = dt == "bf16"
    torch.manual_seed(11)
    m = SimilarityAwarePooling(shape[1], **ctor)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(shape, generator=g)
    if bf:
        x = x.bfloat16().float()
    gp = torch.randn(shape[0], m.nfp_channels, generator=g)
    # float64 host formulation, on the CPU
    m64 = SimilarityAwarePooling(shape[1], **ctor).double()
    m64.load_state_dict(m.state_dict())
    x64 = x.double().requires_grad_(True)
    p64 = m64(x64)
    p64.backward(gp.double())
    # the module on the device
    md = m.to(dev)
    xd = x.to(dev).to(torch.bfloat16 if bf else torch.float32)
    if cl:
        xd = xd.contiguous(memory_format=torch.channels_last)
    xd.requires_grad_(True)
    pd = md(xd)
    assert _variant() == f"attpool_fwd<{dt}>", _variant()
    pd.backward(gp.to(dev).to(pd.dtype))
    errs = dict(pooled=rel_err(_np(pd), _np(p64)), grad_x=rel_err(_np(xd.grad), _np(x64.grad)),
                grad_w=rel_err(_np(md.att_proj.weight.grad), _np(m64.att_proj.weight.grad)))
    print(shape, ctor, cl, dt, errs)
    assert errs["pooled"] <= (BF_OUT if bf else F32)
    assert errs["grad_x"] <= (BF_GRAD if bf else F32)
    # att_proj's gradient end to end is held to the float32 bar only.  The attention's adjoint sums to zero over the pixels, so
    # grad_w = sum_p dl_p m_np sees the maps' VARIATION over the pixels, while the bf16 maps the layer hands over carry a
    # rounding of 2^-9 of their MAGNITUDE: for L2 maps of 64 channels (values near 11, varying by about 1) that alone is
    # some 2 % of grad_w — a property of bf16 maps, not of the tail (printed above; on the same rounded maps grad_w is held
    # to the bf16 bar by test_op_matches_float64_formulation).
    if not bf:
        assert errs["grad_w"] <= F32


# ---- 8. the calls that take the torch tail ---------------------------------------------------------------------------------
def test_strided_fp16_and_float64_maps_take_the_torch_tail(dev):
    from neighbour_feature_pooling_amd import nfp_attention_pool
    maps, w, b, gp = _inputs(2, 8, 60, torch.float32, seed=5)
    ref = _ref64(maps, w, b, gp)
    n0 = _count()
    wide = torch.zeros(2, 8, 120, device=dev)
    wide[..., ::2] = maps
    strided = wide[..., ::2].requires_grad_(True)
    assert not strided.is_contiguous()
    for m_in, tol in ((strided, F32), (maps.double().requires_grad_(True), 1e-12), (maps.half().requires_grad_(True), BF_OUT)):
        pdt = torch.float64 if m_in.dtype == torch.float64 else torch.float32      # (float64 maps: float64 parameters too)
        wi, bi = w.to(pdt).requires_grad_(True), b.to(pdt).requires_grad_(True)
        pooled = nfp_attention_pool(m_in, wi, bi)
        assert pooled.dtype == m_in.dtype
        gm, gw, gb = torch.autograd.grad(pooled, (m_in, wi, bi), gp.to(pooled.dtype))
        r = ref if m_in.dtype != torch.float16 else _ref64(maps.half(), w, b, gp)
        assert rel_err(_np(pooled), _np(r[0])) <= tol
        assert rel_err(_np(gm), _np(r[1])) <= tol
        assert rel_err(_np(gw), _np(r[2])) <= tol
    assert _count() == n0                                           # no NFP kernel ran


def test_env_switch_selects_the_torch_tail(dev, monkeypatch):
    c = KS.SAP_BY_NAME["sap_l2_r2_3x8x9x8"]
    m, g = sap_module(c)
    m = m.to(dev)
    x = torch.from_numpy(K.make_input(c)).to(dev)
    with torch.no_grad():
        n0 = _count()
        m.nfp(x)
        k_fwd = _count() - n0
        n0 = _count()
        hip = m(x)
        assert _count() - n0 == k_fwd + 1
        monkeypatch.setenv("NFP_SAP_TORCH", "1")                   # read at call time
        n0 = _count()
        tail = m(x)
        assert _count() - n0 == k_fwd
        assert not _variant().startswith("attpool")
    assert rel_err(_np(tail), _np(hip)) <= F32
    check_against_fixture(run_sap(m, c, dev=dev), g, F32)            # the torch tail on the device, gradients included
    monkeypatch.delenv("NFP_SAP_TORCH")
    n0 = _count()
    with torch.no_grad():
        m(x)
    assert _count() - n0 == k_fwd + 1


def test_torch_compile_fullgraph_matches_eager(dev):
    c = KS.SAP_BY_NAME["sap_cos_r1_2x16x7x7"]
    m, g = sap_module(c)
    m = m.to(dev)
    eager = run_sap(m, c, dev=dev)
    torch._dynamo.reset()
    compiled = run_sap(torch.compile(m, fullgraph=True), c, dev=dev)
    for u, v in zip(eager[:3], compiled[:3]):
        assert rel_err(v, u) <= F32
    check_against_fixture(compiled, g, F32)


def test_autocast_takes_and_returns_float32(dev):
    from neighbour_feature_pooling_amd import nfp_attention_pool
    maps, w, b, gp = _inputs(2, 8, 25, torch.bfloat16, seed=6)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = nfp_attention_pool(maps, w, b)
    assert out.dtype == torch.float32 and _variant() == "attpool_fwd<f32>"
    assert rel_err(_np(out), _np(_ref64(maps, w, b, gp)[0])) <= F32


def test_cuda_graph_replay_of_a_no_grad_forward_matches_eager(dev):
    c = KS.SAP_BY_NAME["sap_cos_r1_2x16x7x7"]
    m, _ = sap_module(c)
    m = m.to(dev)
    x = torch.from_numpy(K.make_input(c)).to(dev)
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
