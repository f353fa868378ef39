"""NFPHead, MultiRadiusNFPHead, AdaptiveFusionNFP and functional.nfp_compress_pool on the host: the heads against the
reference's fixtures (tests/golden/head_*.npz, make_golden_heads.py), reference-identical initialisation and state dict, the
torch composition of the tail, its routing predicate, the B*P = 1 error, NFPHeadNet(fused_compress=True), and the
nfp_cpool_* declarations with their argument checks (which run before any HIP call).  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases_heads as KH
import neighbour_feature_pooling_amd as pkg
from conftest import ROOT, load_golden, rel_err
from neighbour_feature_pooling_amd import _abi, functional, nfp_compress_pool, nfp_compress_pool_tensors
from neighbour_feature_pooling_amd._host import compress_pool_host

TOL = 1e-5      # the float32 bar of test_sap_host.py / test_bottleneck_host.py: of each tensor's max magnitude
NEW_EXPORTS = {"nfp_cpool_saved_floats", "nfp_cpool_scratch_floats", "nfp_cpool_forward", "nfp_cpool_backward"}


def head_module(c, g=None):
    """The case's head with the fixture's parameters and BatchNorm buffers (strict load), in the case's mode."""
    g = load_golden(c["name"]) if g is None else g
    m = getattr(pkg, c["cls"])(**{KH.IN_KW[c["cls"]]: c["shape"][1]}, **c["ctor"])
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p:")}, strict=True)
    m.train(c["train"])
    return m, g


def run_head(m, c, dev="cpu"):
    """out, grad_x, {parameter gradients}, {BatchNorm buffers after the step} (numpy float32) of the case's seeded step."""
    x = torch.from_numpy(KH.make_input(c)).to(dev).requires_grad_(True)
    m.zero_grad(set_to_none=True)
    out = m(x)
    out.backward(torch.from_numpy(KH.make_grad_out(c, out.shape)).to(dev))
    grads = {k: p.grad.detach().float().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    after = {k: v.detach().float().cpu().numpy() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    return out.detach().float().cpu().numpy(), x.grad.detach().float().cpu().numpy(), grads, after


def fixture_errors(got, g):
    """{tensor name: error relative to the fixture tensor's max magnitude}: out, grad_x, every parameter gradient, every
    BatchNorm buffer after the step."""
    out, gx, grads, after = got
    assert out.shape == g["out"].shape
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


@pytest.mark.parametrize("name", [c["name"] for c in KH.HEAD_CASES])
def test_cpu_matches_reference_fixture(name):
    c = KH.HEAD_BY_NAME[name]
    m, g = head_module(c)
    errs = fixture_errors(run_head(m, c), g)
    print(errs)
    assert {"g:compress.0.weight", "g:compress.1.weight", "g:compress.1.bias", "after:compress.1.running_mean",
            "after:compress.1.running_var", "after:compress.1.num_batches_tracked"} <= set(errs)
    for k, e in errs.items():
        assert e <= TOL, (k, e)


def test_the_train_step_moves_the_running_statistics_and_eval_leaves_them():
    g = load_golden("head_nfp_4x16x7x7")
    assert not np.array_equal(g["after:compress.1.running_mean"], g["p:compress.1.running_mean"])
    assert int(g["after:compress.1.num_batches_tracked"]) == int(g["p:compress.1.num_batches_tracked"]) + 1
    g = load_golden("head_nfp_eval_4x16x7x7")
    assert np.abs(g["p:compress.1.running_mean"]).max() > 0          # (the fixture's statistics are not the initial ones)
    for k in g:
        if k.startswith("after:"):
            assert np.array_equal(g[k], g["p:" + k[6:]])


@pytest.mark.parametrize("name,cls,C,ctor,seed", KH.HEAD_INIT_CASES, ids=[c[0] for c in KH.HEAD_INIT_CASES])
def test_init_matches_the_reference_bitwise(name, cls, C, ctor, seed):
    g = load_golden(name)
    torch.manual_seed(seed)
    m = getattr(pkg, cls)(**{KH.IN_KW[cls]: C}, **ctor)
    sd = m.state_dict()
    stored = [k[2:] for k in g if k.startswith("p:")]
    assert stored and sorted(sd) == [str(k) for k in g["sd_keys"]]
    for k in stored:
        assert np.array_equal(sd[k].numpy(), g["p:" + k]), k
    assert isinstance(m.compress, torch.nn.Sequential) and isinstance(m.compress[1], torch.nn.BatchNorm2d)
    if cls == "NFPHead":
        assert m.nfp_out_channels == 8 and isinstance(m.gap, torch.nn.AdaptiveAvgPool2d) and len(m.fusion_mlp) == 3
    elif cls == "MultiRadiusNFPHead":
        assert len(m.nfp_blocks) == 2 and m.compress[0].in_channels == 32 and len(m.se_gate) == 4
    else:
        assert m.nfp_dim == 24 * 49 and m.dropout.p == 0.2 and len(m.fusion_gate) == 4


@pytest.mark.parametrize("name", [c["name"] for c in KH.HEAD_CASES[:3]])
def test_state_dict_round_trip_is_strict(name):
    c = KH.HEAD_BY_NAME[name]
    m, g = head_module(c)
    sd = m.state_dict()
    assert sorted(sd) == [str(k) for k in g["sd_keys"]]
    fresh = getattr(pkg, c["cls"])(**{KH.IN_KW[c["cls"]]: c["shape"][1]}, **c["ctor"])
    fresh.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)     # (with the frozen one-hot conv weights)
    assert torch.equal(fresh.compress[0].weight.detach(), torch.from_numpy(g["p:compress.0.weight"]))


def test_no_conv_head_is_left_out():
    assert not hasattr(pkg, "NFPHead_NoConv")


def _tail_inputs(B=3, N=8, H=5, W=4, D=6, dtype=torch.float32, seed=3):
    gen = torch.Generator().manual_seed(seed)
    maps = torch.randn(B, N, H, W, generator=gen, dtype=dtype)
    w = torch.randn(D, N, 1, 1, generator=gen, dtype=dtype)
    gamma, beta = torch.rand(D, generator=gen, dtype=dtype) + 0.5, torch.randn(D, generator=gen, dtype=dtype)
    rm, rv = torch.randn(D, generator=gen, dtype=dtype), torch.rand(D, generator=gen, dtype=dtype) + 0.5
    return maps, w, gamma, beta, rm, rv


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_host_composition_equals_the_aten_ops_bitwise(training, dtype):
    maps, w, gamma, beta, rm, rv = _tail_inputs(dtype=dtype)
    rm1, rv1, rm2, rv2 = rm.clone(), rv.clone(), rm.clone(), rv.clone()
    got = compress_pool_host(maps, w, gamma, beta, rm1, rv1, training, 0.1, 1e-5)
    want = F.relu(F.batch_norm(F.conv2d(maps, w), rm2, rv2, gamma, beta, training, 0.1, 1e-5)).mean((2, 3))
    assert got.shape == (3, 6) and torch.equal(got, want)
    assert torch.equal(rm1, rm2) and torch.equal(rv1, rv2) and torch.equal(rm1, rm) != training
    # [B,N,P] maps and a [D,N] weight; the public call on CPU tensors is the composition
    assert torch.allclose(compress_pool_host(maps.flatten(2), w.reshape(6, 8), gamma, beta, rm.clone(), rv.clone(), training,
                                             0.1, 1e-5), want, rtol=0, atol=1e-6)
    assert torch.equal(nfp_compress_pool_tensors(maps, w, gamma, beta, rm.clone(), rv.clone(), training, 0.1, 1e-5), want)


def test_module_form_follows_batchnorm_forward():
    maps, w, *_ = _tail_inputs()
    for kw in (dict(), dict(momentum=None), dict(affine=False), dict(track_running_stats=False)):
        a, b = torch.nn.BatchNorm2d(6, **kw), torch.nn.BatchNorm2d(6, **kw)
        for step in range(2):
            got, want = nfp_compress_pool(maps + step, w, a), F.relu(b(F.conv2d(maps + step, w))).mean((2, 3))
            assert torch.equal(got, want), kw
        for k, v in a.state_dict().items():
            assert torch.equal(v, b.state_dict()[k]), (kw, k)
        a.eval(), b.eval()
        assert torch.equal(nfp_compress_pool(maps, w, a), F.relu(b(F.conv2d(maps, w))).mean((2, 3)))
        # training= overrides the module's mode
        assert torch.equal(nfp_compress_pool(maps, w, a, training=True), F.relu(b.train()(F.conv2d(maps, w))).mean((2, 3)))


def test_one_value_per_channel_raises_as_torch_does():
    maps, w, gamma, beta, rm, rv = _tail_inputs(B=1, H=1, W=1)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        nfp_compress_pool_tensors(maps, w, gamma, beta, rm, rv, True)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        nfp_compress_pool(maps, w, torch.nn.BatchNorm2d(6))
    assert nfp_compress_pool_tensors(maps, w, gamma, beta, rm, rv, False).shape == (1, 6)      # eval is fine


def test_argument_errors():
    maps, w, gamma, beta, rm, rv = _tail_inputs()
    with pytest.raises(RuntimeError):
        nfp_compress_pool_tensors(maps, w[:, :4], gamma, beta, rm, rv, True)
    with pytest.raises(RuntimeError):
        nfp_compress_pool_tensors(maps[0, 0], w, gamma, beta, rm, rv, True)
    with pytest.raises(RuntimeError):
        nfp_compress_pool_tensors(maps, w, gamma, beta, None, None, False)


class _Fake:
    """What cpool_hip_serves looks at, without a device."""

    def __init__(self, shape=(4, 8, 7, 7), dtype=torch.float32, cuda=True, contiguous=True):
        self.shape, self.dtype, self.is_cuda, self._c = shape, dtype, cuda, contiguous

    def is_contiguous(self):
        return self._c

    def numel(self):
        return int(np.prod(self.shape))


def test_routing_predicate(monkeypatch):
    monkeypatch.delenv("NFP_CPOOL_TORCH", raising=False)
    serves = functional.cpool_hip_serves
    g = torch.ones(4)
    assert serves(_Fake(), g, g, 0.1)
    assert serves(_Fake(dtype=torch.bfloat16), g, g, 0.1)
    # more than 8 maps measured slower than the composition: routed to it unless NFP_CPOOL_TORCH=0 forces the HIP tail
    assert not serves(_Fake(shape=(4, 32, 7, 7)), g, g, 0.1) and not serves(_Fake(shape=(4, 9, 7, 7)), g, g, 0.1)
    monkeypatch.setenv("NFP_CPOOL_TORCH", "0")
    assert serves(_Fake(shape=(4, 32, 7, 7), dtype=torch.bfloat16), g, g, 0.1) and serves(_Fake(shape=(4, 24, 7, 7)), g, g, 0.1)
    assert not serves(_Fake(shape=(4, 33, 7, 7)), g, g, 0.1) and not serves(_Fake(cuda=False), g, g, 0.1)
    monkeypatch.delenv("NFP_CPOOL_TORCH")
    assert not serves(_Fake(cuda=False), g, g, 0.1)
    assert not serves(_Fake(dtype=torch.float16), g, g, 0.1)
    assert not serves(_Fake(dtype=torch.float64), g, g, 0.1)
    assert not serves(_Fake(contiguous=False), g, g, 0.1)
    assert not serves(_Fake(shape=(4, 33, 7, 7)), g, g, 0.1)                  # more than 32 maps
    assert not serves(_Fake(shape=(0, 8, 7, 7)), g, g, 0.1)
    assert not serves(_Fake(), None, None, 0.1)                               # affine=False
    assert not serves(_Fake(), g, g, None)                                    # momentum=None
    monkeypatch.setenv("NFP_CPOOL_TORCH", "1")                                # the A/B switch, read at call time
    assert not serves(_Fake(), g, g, 0.1)
    monkeypatch.delenv("NFP_CPOOL_TORCH")
    assert serves(_Fake(), g, g, 0.1)
    assert functional.CPOOL_MAX_MAPS == 32 and functional.CPOOL_ROUTED_MAPS == 8


def test_head_net_with_the_fused_tail_equals_the_default_on_the_cpu():
    from neighbour_feature_pooling_amd.models import NFPHeadNet
    torch.manual_seed(5)
    a = NFPHeadNet(num_classes=5, bottleneck_dim=24)
    b = NFPHeadNet(num_classes=5, bottleneck_dim=24, fused_compress=True)
    assert a.fused_compress is False and b.fused_compress is True
    b.load_state_dict(a.state_dict(), strict=True)
    x = torch.randn(2, 3, 64, 64)
    ya, yb = a(x), b(x)
    assert torch.equal(ya, yb)
    ya.sum().backward(), yb.sum().backward()
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p.grad, q.grad), k
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k


def test_new_exports_are_declared_and_loadable():
    src = open(os.path.join(ROOT, "include", "nfp.h")).read()
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(nfp_[a-z_]+)\s*\(", body))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(_abi.EXPORTS)
    assert int(re.search(r"#define NFP_ABI_VERSION (\d+)", src).group(1)) == _abi.ABI_VERSION == 7
    from neighbour_feature_pooling_amd import build
    assert "nfp_cpool.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "nfp_cpool.hip"))
    build.build_hip()
    L = _abi.load()
    for n in NEW_EXPORTS:
        assert hasattr(L, n)


def test_invalid_arguments_are_refused_before_any_launch():
    from neighbour_feature_pooling_amd.build import build_hip
    build_hip()
    L = _abi.load()
    assert L.nfp_cpool_saved_floats(8, 512) == 2 * 8 + 64 + 512
    assert L.nfp_cpool_scratch_floats(4, 8, 49, 32, 0) == 4 * (16 + 64)               # one chunk per image
    assert L.nfp_cpool_scratch_floats(2, 32, 1600, 16, 0) == 2 * 7 * (64 + 1024)       # 1600 pixels in chunks of 256
    assert L.nfp_cpool_scratch_floats(4, 8, 49, 32, 1) == 4 * 32 * 9 + 1 * (8 + 64)
    p = 0x1000      # (never dereferenced: every call below is refused, or returns, before any HIP call)
    n0 = L.nfp_launch_count()

    def fwd(B=4, N=8, P=49, D=32, dtype=0, training=1, maps=p, w=p, gamma=p, beta=p, rm=p, rv=p, mom=0.1, eps=1e-5, out=p,
            saved=p, ns=112, scratch=p, nscr=320):
        return L.nfp_cpool_forward(B, N, P, D, dtype, training, maps, w, gamma, beta, rm, rv, mom, eps, out, saved, ns, scratch,
                                   nscr, None)

    def bwd(B=4, N=8, P=49, D=32, dtype=0, training=1, maps=p, w=p, gamma=p, beta=p, rm=p, rv=p, eps=1e-5, saved=p, ns=112,
            go=p, gm=p, gw=p, gg=p, gb=p, scratch=p, nscr=1224):
        return L.nfp_cpool_backward(B, N, P, D, dtype, training, maps, w, gamma, beta, rm, rv, eps, saved, ns, go, gm, gw, gg, gb,
                                    scratch, nscr, None)

    for kw in (dict(maps=None), dict(w=None), dict(gamma=None), dict(beta=None), dict(out=None), dict(B=-1), dict(N=0),
               dict(P=0), dict(D=0), dict(dtype=2), dict(rm=None), dict(rv=None), dict(training=0, rm=None, rv=None),
               dict(eps=-1.0), dict(saved=None), dict(ns=111), dict(scratch=None), dict(nscr=319)):
        assert fwd(**kw) == -1, kw
        assert L.nfp_last_error()
    for kw in (dict(maps=None), dict(w=None), dict(gamma=None), dict(beta=None), dict(go=None), dict(B=-1), dict(N=0),
               dict(P=0), dict(D=0), dict(dtype=-1), dict(training=0, rm=None), dict(training=0, rv=None), dict(saved=None),
               dict(ns=111), dict(scratch=None), dict(nscr=1223), dict(gm=None, nscr=0), dict(training=0, gm=None, nscr=0)):
        assert bwd(**kw) == -1, kw
    assert b"scratch" in L.nfp_last_error()
    for kw in (dict(N=33), dict(N=2, P=1 << 30), dict(B=1, P=1), dict(D=(1 << 22) + 1)):
        assert fwd(**kw) == -2 and bwd(**kw) == -2, kw                    # NFP_E_UNSUPPORTED
    assert fwd(B=0, maps=None, out=None, scratch=None, nscr=0) == 0       # an empty batch: OK, no launch
    assert bwd(B=0, maps=None, go=None, gm=None, scratch=None, nscr=0) == 0
    assert bwd(gm=None, gw=None, gg=None, gb=None, scratch=None, nscr=0) == 0      # nothing wanted: nothing done
    assert L.nfp_launch_count() == n0
