"""NFPPooling(bias=True) on the MI355X: the biased HIP kernels (csrc/nfp_bias.hip, include/nfp.h ABI 7) against the
reference's fixtures (tests/golden/bias_*.npz) and the float64 host formulation, their determinism, the ABI's buffer
checks, torch.compile / opcheck / graph capture, and the callers that used to bypass forward()."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases as K
import cases_bias as KB
from conftest import assert_matches_golden, golden_out_shape, load_golden, rel_err, same_nan_pattern

pytestmark = pytest.mark.gpu

MEASURES = [m for m in KB.MEASURES if m != "scs"]
# float32-vs-float32 conditioning of a few measures (eps-sized denominators, near-cancelling sums): not index errors
LOOSE = ("geman", "pearson", "hellinger", "squaredchord", "jeffrey", "smith", "canberra", "chisquared1", "chisquared2")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from neighbour_feature_pooling_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


def _lib():
    from neighbour_feature_pooling_amd import _abi
    return _abi.load()


def _variant():
    return _lib().nfp_last_variant().decode()


def _module(C, ctor, bc=None, nb=None, seed=0):
    from neighbour_feature_pooling_amd import NFPPooling
    torch.manual_seed(seed)
    m = NFPPooling(C, bias=True, **ctor)
    with torch.no_grad():
        if bc is not None:
            m.center_value.bias.copy_(torch.as_tensor(bc))
        if nb is not None:
            m.comp_neighbors.bias.copy_(torch.as_tensor(nb))
    return m


def _run(m, x, go):
    """out, grad_x, grad_centre_bias (None allowed), grad_neighbour_bias — numpy float32."""
    m.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    out = m(x)
    out.backward(go)
    gbc = m.center_value.bias.grad
    return (out.detach().float().cpu().numpy(), x.grad.float().cpu().numpy(),
            None if gbc is None else gbc.float().cpu().numpy(), m.comp_neighbors.bias.grad.float().cpu().numpy(), x.grad)


def _host64(m, x, go):
    """The float64 host formulation on the same (already rounded) input and biases."""
    from neighbour_feature_pooling_amd._host import nfp_host
    x64 = x.detach().double().cpu().requires_grad_(True)
    bc = m.center_value.bias.detach().double().cpu().requires_grad_(True)
    nb = m.comp_neighbors.bias.detach().double().cpu().requires_grad_(True)
    ref = nfp_host(x64, m.config, bc, nb)
    ref.backward(go.double().cpu())
    return (ref.detach().numpy(), x64.grad.numpy(), None if bc.grad is None else bc.grad.numpy(), nb.grad.numpy())


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", [c["name"] for c in KB.BIAS_CASES])
def test_fixture_float32(name, channels_last, dev):
    c = KB.BIAS_BY_NAME[name]
    g = load_golden(name)
    m = _module(c["shape"][1], c["ctor"], g["bc"], g["nb"]).to(dev)
    x = torch.from_numpy(K.make_input(c)).to(dev)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    go = torch.from_numpy(K.make_grad_out(c, golden_out_shape(g))).to(dev)
    n0 = _lib().nfp_launch_count()
    meas = c["ctor"].get("measure", "norm").lower()
    with pytest.warns(RuntimeWarning) if meas == "scs" else _nullctx():
        out, gx, gbc, gnb, gxt = _run(m, x, go)
    torch.cuda.synchronize()
    if meas != "scs":
        assert _lib().nfp_launch_count() >= n0 + 5, "the biased HIP kernels did not run"
        assert _variant().startswith("bias_bwd<"), _variant()
    if channels_last:
        assert gxt.is_contiguous(memory_format=torch.channels_last)
    tol = 5e-4 if meas in LOOSE else 1e-4
    assert_matches_golden(out, gx, g, tol)
    assert rel_err(gnb, g["gnb"]) <= tol
    if int(g["gbc_none"]):
        assert gbc is None
    else:
        assert rel_err(gbc, g["gbc"]) <= tol


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


# channels-last under the measure's own id (as before), NCHW as <measure>-nchw
BF16_CASES = ([pytest.param(m, True, id=m) for m in MEASURES + ["Norm"]] +
              [pytest.param(m, False, id=f"{m}-nchw") for m in MEASURES + ["Norm"]])


@pytest.mark.parametrize("measure,channels_last", BF16_CASES)
def test_every_measure_bf16(measure, channels_last, dev):
    """bf16 storage, f32 arithmetic, against the float64 formulation on the SAME bf16-rounded inputs, at the bf16 bounds
    of the existing bf16 tests: out within 1e-2 and gradients within 2e-2 of the tensor's largest magnitude."""
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(2, 12, 9, 7, generator=g) + 0.25).to(torch.bfloat16)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    m = _module(12, dict(R=1, measure=measure, padding=1), seed=4)
    go = torch.randn(2, 8, 9, 7, generator=g).to(torch.bfloat16)
    mg = m.to(dev)
    out, gx, gbc, gnb, _ = _run(mg, x.to(dev), go.to(dev))
    assert _variant().startswith("bias_bwd<"), _variant()
    assert ("nhwc" if channels_last else "nchw") in _variant(), _variant()
    r_out, r_gx, r_gbc, r_gnb = _host64(m.cpu(), x.float(), go.float())
    assert rel_err(out, r_out) <= 1e-2
    assert rel_err(gx, r_gx) <= 2e-2
    assert rel_err(gnb, r_gnb) <= 2e-2
    assert (gbc is None) == (r_gbc is None)
    if gbc is not None:
        assert rel_err(gbc, r_gbc) <= 2e-2


def test_random_geometries(dev):
    """Random (geometry, measure, layout) draws against the float64 formulation: the inverse index map of bias_gx and
    the zero-padded pairs of bias_part are what this nets."""
    import random
    rnd = random.Random(11)
    done = 0
    for it in range(300):
        if done >= 60:
            break
        H, W = rnd.randint(2, 13), rnd.randint(2, 13)
        R, stride, dil = rnd.choice([1, 1, 2]), rnd.choice([1, 1, 2, 3]), rnd.choice([1, 1, 2])
        pad = rnd.randint(0, R + 1)
        mode = rnd.choice(["reflect", "zeros", "replicate", "circular"])
        k = 2 * R + 1
        if H + 2 * pad < dil * (k - 1) + 1 or W + 2 * pad < dil * (k - 1) + 1:
            continue
        if (mode == "reflect" and (pad >= H or pad >= W)) or (mode == "circular" and (pad > H or pad > W)):
            continue
        meas = rnd.choice(MEASURES + ["Norm"])
        B, C = rnd.randint(1, 3), rnd.choice([3, 5, 6, 8, 13])
        ctor = dict(R=R, measure=meas, padding=pad, stride=stride, dilation=dil, padding_mode=mode,
                    similarity=rnd.random() < 0.7)
        if meas.lower() == "norm":
            ctor["p"] = rnd.choice([1, 2, 3])
        m = _module(C, ctor, seed=it)
        gen = torch.Generator().manual_seed(it)
        x = torch.rand(B, C, H, W, generator=gen) + 0.25
        mg = _module(C, ctor, seed=it).to(dev)
        xd = x.to(dev)
        if rnd.random() < 0.3:
            xd = xd.contiguous(memory_format=torch.channels_last)
        out_shape = mg(xd).shape
        go = torch.randn(out_shape, generator=gen)
        out, gx, gbc, gnb, _ = _run(mg, xd, go.to(dev))
        r_out, r_gx, r_gbc, r_gnb = _host64(m, x, go)
        what = (it, tuple(x.shape), ctor)
        tol = 5e-4 if meas.lower() in LOOSE else 1e-4
        assert same_nan_pattern(out, r_out), what
        assert rel_err(np.nan_to_num(out), np.nan_to_num(r_out)) <= tol, what
        assert rel_err(np.nan_to_num(gx), np.nan_to_num(r_gx)) <= tol, what
        assert rel_err(np.nan_to_num(gnb), np.nan_to_num(r_gnb)) <= tol, what
        assert (gbc is None) == (r_gbc is None), what
        if gbc is not None:
            assert rel_err(np.nan_to_num(gbc), np.nan_to_num(r_gbc)) <= tol, what
        done += 1
    assert done >= 60


def test_bias_gradients_are_bitwise_reproducible(dev):
    m = _module(64, dict(R=1, measure="cosine", padding=1), seed=1).to(dev)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(8, 64, 14, 14, generator=g).to(dev)
    go = torch.randn(8, 8, 14, 14, generator=g).to(dev)
    a = _run(m, x, go)
    b = _run(m, x, go)
    for u, v in zip(a[:4], b[:4]):
        assert np.array_equal(u, v)


def test_short_buffers_are_refused_before_any_launch(dev):
    from neighbour_feature_pooling_amd import _abi, functional
    from neighbour_feature_pooling_amd.functional import NfpConfig
    L = _lib()
    cfg = NfpConfig(R=1, measure="cosine", padding=1, diff_weights=False)
    x = torch.randn(2, 4, 6, 5, device=dev)
    plan = functional._plan(x, "nchw", cfg, tables=False)
    d, oshape, ns, nsc = plan.desc, plan.oshape, plan.ask("nfp_bias_saved_floats"), plan.ask("nfp_bias_scratch_floats")
    assert ns > 0 and nsc > 0
    bc, nb = torch.zeros(4, device=dev), torch.zeros(32, device=dev)
    out = torch.empty(oshape, device=dev)
    saved = torch.empty(ns, device=dev)
    scratch = torch.empty(nsc, device=dev)
    gx = torch.empty_like(x)
    gbc, gnb = torch.empty_like(bc), torch.empty_like(nb)
    stream = functional._raw_stream(x.device)
    torch.cuda.synchronize()
    n0 = L.nfp_launch_count()
    assert L.nfp_bias_forward(ctypes.byref(d), x.data_ptr(), bc.data_ptr(), nb.data_ptr(), out.data_ptr(),
                              saved.data_ptr(), ns - 1, stream) == -1
    assert b"saved" in L.nfp_last_error()
    assert L.nfp_bias_forward(ctypes.byref(d), x.data_ptr(), bc.data_ptr(), nb.data_ptr(), out.data_ptr(),
                              saved.data_ptr(), ns, stream) == 0
    n1 = L.nfp_launch_count()
    assert n1 > n0
    go = torch.ones_like(out)
    args = lambda s_n, sc_n: (ctypes.byref(d), x.data_ptr(), bc.data_ptr(), nb.data_ptr(), go.data_ptr(), out.data_ptr(),
                              saved.data_ptr(), s_n, gx.data_ptr(), gbc.data_ptr(), gnb.data_ptr(), scratch.data_ptr(),
                              sc_n, stream)
    assert L.nfp_bias_backward(*args(ns - 1, nsc)) == -1
    assert L.nfp_bias_backward(*args(ns, nsc - 1)) == -1
    assert b"scratch" in L.nfp_last_error()
    assert L.nfp_launch_count() == n1
    assert L.nfp_bias_backward(*args(ns, nsc)) == 0
    torch.cuda.synchronize()
    assert L.nfp_launch_count() > n1
    assert _abi.ABI_VERSION == L.nfp_abi_version() == 7


def test_torch_compile_fullgraph_matches_eager(dev):
    m = _module(16, dict(R=1, measure="cosine", padding=1), seed=3).to(dev)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 16, 9, 9, generator=g).to(dev)
    go = torch.randn(2, 8, 9, 9, generator=g).to(dev)
    eager = _run(m, x, go)
    torch._dynamo.reset()
    cm = torch.compile(m, fullgraph=True)
    compiled = _run(cm, x, go)
    assert _variant().startswith("bias_bwd<"), _variant()
    for u, v in zip(eager[:4], compiled[:4]):
        assert rel_err(v, u) <= 1e-6


@pytest.mark.parametrize("measure", ["cosine", "norm"])
def test_opcheck(measure, dev):
    from neighbour_feature_pooling_amd import _ops
    from neighbour_feature_pooling_amd.functional import NfpConfig
    cfg = NfpConfig(R=1, measure=measure, padding=1, diff_weights=measure == "norm")
    x = torch.randn(2, 4, 6, 5, device=dev, requires_grad=True)
    bc = torch.randn(4, device=dev, requires_grad=True)
    nb = torch.randn(32, device=dev, requires_grad=True)
    torch.library.opcheck(torch.ops.nfp_amd.nfp_biased.default, (x, bc, nb, *_ops.cfg_args(cfg)),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    out, saved = torch.ops.nfp_amd.nfp_biased(x.detach(), bc.detach(), nb.detach(), *_ops.cfg_args(cfg))
    torch.library.opcheck(torch.ops.nfp_amd.nfp_biased_backward.default,
                          (x.detach(), bc.detach(), nb.detach(), out, saved, torch.randn_like(out), *_ops.cfg_args(cfg)),
                          test_utils=("test_schema", "test_faketensor"))


def test_cuda_graph_replay_matches_eager(dev):
    m = _module(16, dict(R=1, measure="gfc", padding=1), seed=6).to(dev)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 16, 8, 8, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(2, 8, 8, 8, generator=g).to(dev)
    ref = _run(m, x, go)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):            # eager warm-up on the capture stream
            m.zero_grad(set_to_none=True)
            x.grad = None
            m(x).backward(go)
    torch.cuda.current_stream().wait_stream(s)
    m.zero_grad(set_to_none=False)
    x.grad = torch.zeros_like(x)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(x)
        out.backward(go)
    for p in m.parameters():
        p.grad.zero_()
    x.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.detach().cpu().numpy(), ref[0])
    assert rel_err(x.grad.cpu().numpy(), ref[1]) <= 1e-6
    assert rel_err(m.center_value.bias.grad.cpu().numpy(), ref[2]) <= 1e-6
    assert rel_err(m.comp_neighbors.bias.grad.cpu().numpy(), ref[3]) <= 1e-6


def test_multi_radius_equals_cat_of_blocks(dev):
    from neighbour_feature_pooling_amd.nfp import MultiRadiusNFPPooling
    torch.manual_seed(8)
    mr = MultiRadiusNFPPooling(8, R_list=(1, 2), measure="cosine", bias=True).to(dev)
    x = torch.randn(2, 8, 10, 10, device=dev)
    got = mr(x)
    assert _variant().startswith("bias_fwd<"), _variant()
    want = torch.cat([b(x) for b in mr.nfp_blocks], dim=1)
    assert torch.equal(got, want)


def test_pooled_callers_keep_the_bias(dev):
    """nfp_pooling(nfp_layer=<biased layer>) and the multi-stage net's adaptive_avg_pool2d(layer(feat), 1) used to read
    layer.config and call the fused kernels directly, which would drop the bias."""
    from neighbour_feature_pooling_amd.models import MultiStageNFPNet
    from neighbour_feature_pooling_amd.pooling import nfp_pooling
    layer = _module(8, dict(R=1, measure="cosine", padding=1), seed=9).to(dev)   # (C = N: no projection without Params)
    with torch.no_grad():
        layer.comp_neighbors.bias.add_(0.5)
    x = torch.randn(2, 8, 7, 7, device=dev)
    got = nfp_pooling(nfp_layer=layer)(x)
    want = x.mean((2, 3)) * F.adaptive_avg_pool2d(layer(x), 1).flatten(1)
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-7)
    unbiased = _module(8, dict(R=1, measure="cosine", padding=1), seed=9).to(dev)
    with torch.no_grad():
        unbiased.comp_neighbors.bias.zero_()
        unbiased.center_value.bias.zero_()
    assert not torch.allclose(got, x.mean((2, 3)) * F.adaptive_avg_pool2d(unbiased(x), 1).flatten(1), atol=1e-4)

    torch.manual_seed(10)
    net = MultiStageNFPNet(num_classes=4).to(dev).eval()
    from neighbour_feature_pooling_amd import NFPPooling
    for i, old in enumerate(net.nfps):
        torch.manual_seed(20 + i)
        net.nfps[i] = NFPPooling(old.in_channels, R=1, measure="cosine", padding=1, bias=True).to(dev)
        with torch.no_grad():
            net.nfps[i].comp_neighbors.bias.add_(0.3)
    img = torch.randn(2, 3, 64, 64, device=dev)
    with torch.no_grad():
        got = net(img)
        feats = net.backbone.forward_stages(img)
        v = torch.cat([F.adaptive_avg_pool2d(layer(f), 1).flatten(1) for f, layer in zip(feats, net.nfps)], dim=1)
        head = net.conv_head(feats[-1]).mean((2, 3))
        want = net.fc(head * net.nfp_proj(v))
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)


def test_three_sgd_steps_match_the_cpu_path(dev):
    def make():
        torch.manual_seed(12)
        from neighbour_feature_pooling_amd import NFPPooling
        return torch.nn.Sequential(NFPPooling(6, R=1, measure="cosine", padding=1, bias=True), torch.nn.Flatten(),
                                   torch.nn.Linear(8 * 6 * 6, 3))

    g = torch.Generator().manual_seed(13)
    x = torch.randn(4, 6, 6, 6, generator=g)
    y = torch.randint(0, 3, (4,), generator=g)
    nets = {}
    for where in ("cpu", dev):
        net = make().to(where)
        opt = torch.optim.SGD(net.parameters(), lr=0.5)
        for _ in range(3):
            opt.zero_grad()
            torch.nn.functional.cross_entropy(net(x.to(where)), y.to(where)).backward()
            opt.step()
        nets[str(where)] = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    a, b = nets["cpu"], nets[str(dev)]
    for k in a:
        assert torch.allclose(a[k], b[k], rtol=1e-4, atol=1e-5), k
    assert not torch.equal(a["0.comp_neighbors.bias"], make().state_dict()["0.comp_neighbors.bias"])
