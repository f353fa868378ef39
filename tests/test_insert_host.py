"""NFPInsert, NFPInsertNet, NFPBottleneck(fused_project=True) and functional.nfp_compress_map on the host: the block against
the reference's fixtures (tests/golden/insert_*.npz, make_golden_insert.py), reference-identical initialisation and state
dict, the torch composition of the projection with and without its ReLU, the B*P = 1 error, and the nfp_cproj_*
declarations.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases_insert as KI
from conftest import ROOT, load_golden, rel_err
from neighbour_feature_pooling_amd import (NFPBottleneck, NFPInsert, _abi, functional, nfp_compress_map,
                                           nfp_compress_map_tensors)
from neighbour_feature_pooling_amd._host import compress_map_host
from neighbour_feature_pooling_amd.models import NFPInsertNet

TOL = 1e-5      # the float32 bar of test_heads_host.py: of each tensor's max magnitude
NEW_EXPORTS = {"nfp_cproj_scratch_floats", "nfp_cproj_forward", "nfp_cproj_backward"}


def insert_module(c, g=None):
    """The case's block with the fixture's parameters and BatchNorm buffers (strict load), in the case's mode."""
    g = load_golden(c["name"]) if g is None else g
    m = NFPInsert(c["shape"][1], **c["kw"])
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p:")}, strict=True)
    m.train(c["train"])
    return m, g


def run_insert(m, c, dev="cpu"):
    """out, grad_x, {parameter gradients}, {BatchNorm buffers after the step} (numpy float32) of the case's seeded step."""
    x = torch.from_numpy(KI.make_input(c)).to(dev).requires_grad_(True)
    m.zero_grad(set_to_none=True)
    out = m(x)
    out.backward(torch.from_numpy(KI.make_grad_out(c, out.shape)).to(dev))
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


@pytest.mark.parametrize("name", [c["name"] for c in KI.INSERT_CASES])
def test_cpu_matches_reference_fixture(name):
    c = KI.INSERT_BY_NAME[name]
    m, g = insert_module(c)
    errs = fixture_errors(run_insert(m, c), g)
    print(errs)
    assert {"g:nfp_proj.0.weight", "g:nfp_proj.1.weight", "g:nfp_proj.1.bias", "after:nfp_proj.1.running_mean",
            "after:nfp_proj.1.running_var", "after:nfp_proj.1.num_batches_tracked"} <= set(errs)
    for k, e in errs.items():
        assert e <= TOL, (k, e)


def test_the_fixtures_cover_a_shrinking_map_24_maps_and_both_modes():
    assert load_golden("insert_default_2x12x9x9")["out"].shape == (2, 12, 7, 7)       # padding 0: smaller by 2R
    g = load_golden("insert_r2_2x8x9x11")
    assert g["out"].shape == (2, 8, 5, 7) and g["p:nfp_proj.0.weight"].shape == (8, 24, 1, 1)
    g = load_golden("insert_cosine_3x16x7x7")
    assert not np.array_equal(g["after:nfp_proj.1.running_mean"], g["p:nfp_proj.1.running_mean"])
    assert int(g["after:nfp_proj.1.num_batches_tracked"]) == int(g["p:nfp_proj.1.num_batches_tracked"]) + 1
    g = load_golden("insert_cosine_eval_3x16x7x7")
    assert np.abs(g["p:nfp_proj.1.running_mean"]).max() > 0          # (the fixture's statistics are not the initial ones)
    for k in g:
        if k.startswith("after:"):
            assert np.array_equal(g[k], g["p:" + k[6:]])


@pytest.mark.parametrize("name,C,kw,seed", KI.INSERT_INIT_CASES, ids=[c[0] for c in KI.INSERT_INIT_CASES])
def test_init_matches_the_reference_bitwise(name, C, kw, seed):
    g = load_golden(name)
    torch.manual_seed(seed)
    m = NFPInsert(C, **kw)
    sd = m.state_dict()
    stored = [k[2:] for k in g if k.startswith("p:")]
    assert stored and sorted(sd) == [str(k) for k in g["sd_keys"]]
    for k in stored:
        assert np.array_equal(sd[k].numpy(), g["p:" + k]), k
    assert isinstance(m.nfp_proj, torch.nn.Sequential) and len(m.nfp_proj) == 3
    assert isinstance(m.nfp_proj[1], torch.nn.BatchNorm2d) and isinstance(m.nfp_proj[2], torch.nn.ReLU)
    assert m.nfp_proj[0].in_channels == m.nfp.out_channels and m.out_channels == C


def test_defaults_are_the_class_defaults_and_out_channels_may_differ():
    m = NFPInsert(6)
    assert (m.nfp.measure, m.nfp.p, m.nfp.padding, m.nfp.padding_mode, m.nfp.R) == ("norm", 1, 0, "reflect", 1)
    m = NFPInsert(6, out_channels=10, R=2)
    assert m.nfp_proj[0].weight.shape == (10, 24, 1, 1) and m(torch.randn(2, 6, 7, 8)).shape == (2, 10, 3, 4)


def test_state_dict_round_trip_is_strict():
    c = KI.INSERT_CASES[1]
    m, g = insert_module(c)
    sd = m.state_dict()
    assert sorted(sd) == [str(k) for k in g["sd_keys"]]
    fresh = NFPInsert(c["shape"][1], **c["kw"])
    fresh.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)     # (with the frozen one-hot conv weights)
    assert torch.equal(fresh.nfp_proj[0].weight.detach(), torch.from_numpy(g["p:nfp_proj.0.weight"]))


def _inputs(B=3, N=8, H=5, W=4, D=6, dtype=torch.float32, seed=3):
    gen = torch.Generator().manual_seed(seed)
    maps = torch.randn(B, N, H, W, generator=gen, dtype=dtype)
    w = torch.randn(D, N, 1, 1, generator=gen, dtype=dtype)
    gamma, beta = torch.rand(D, generator=gen, dtype=dtype) + 0.5, torch.randn(D, generator=gen, dtype=dtype)
    rm, rv = torch.randn(D, generator=gen, dtype=dtype), torch.rand(D, generator=gen, dtype=dtype) + 0.5
    return maps, w, gamma, beta, rm, rv


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("training", [True, False])
def test_compress_map_on_cpu_is_the_composition(training, relu):
    maps, w, gamma, beta, rm, rv = _inputs()
    rm0, rv0 = rm.clone(), rv.clone()
    y = F.batch_norm(F.conv2d(maps, w), rm0, rv0, gamma, beta, training, 0.1, 1e-5)
    want = F.relu(y) if relu else y
    rm1, rv1 = rm.clone(), rv.clone()
    got = compress_map_host(maps, w, gamma, beta, rm1, rv1, training, 0.1, 1e-5, relu)
    assert got.shape == (3, 6, 5, 4) and torch.equal(got, want) and torch.equal(rm1, rm0) and torch.equal(rv1, rv0)
    assert (not training) or not torch.equal(rm1, rm)
    assert relu or bool((got < 0).any())
    rm2, rv2 = rm.clone(), rv.clone()
    assert torch.equal(nfp_compress_map_tensors(maps, w, gamma, beta, rm2, rv2, training, 0.1, 1e-5, relu), want)
    assert torch.equal(rm2, rm0) and torch.equal(rv2, rv0)
    # [B,N,P] maps and a [D,N] weight
    flat = nfp_compress_map_tensors(maps.flatten(2), w.reshape(6, 8), gamma, beta, rm.clone(), rv.clone(), training, 0.1, 1e-5,
                                    relu)
    assert flat.shape == (3, 6, 20) and torch.allclose(flat, want.flatten(2), rtol=0, atol=1e-6)


@pytest.mark.parametrize("relu", [True, False])
def test_compress_map_follows_the_batchnorm_module(relu):
    maps, w = _inputs()[:2]
    for kw in (dict(), dict(momentum=None), dict(track_running_stats=False), dict(affine=False)):
        a, b = torch.nn.BatchNorm2d(6, **kw), torch.nn.BatchNorm2d(6, **kw)
        act = F.relu if relu else (lambda t: t)
        for step in range(2):
            got, want = nfp_compress_map(maps + step, w, a, relu=relu), act(b(F.conv2d(maps + step, w)))
            assert torch.equal(got, want), kw
        for k, v in b.state_dict().items():
            assert torch.equal(a.state_dict()[k], v), (kw, k)
        a.eval(), b.eval()
        assert torch.equal(nfp_compress_map(maps, w, a, relu=relu), act(b(F.conv2d(maps, w))))
        assert torch.equal(nfp_compress_map(maps, w, a, relu=relu, training=True), act(b.train()(F.conv2d(maps, w))))


def test_compress_map_gradients_are_autograds():
    maps, w, gamma, beta, rm, rv = _inputs()
    leaves = [t.clone().requires_grad_(True) for t in (maps, w, gamma, beta)]
    ref = [t.clone().requires_grad_(True) for t in (maps, w, gamma, beta)]
    go = torch.randn(3, 6, 5, 4, generator=torch.Generator().manual_seed(9))
    nfp_compress_map_tensors(*leaves, rm.clone(), rv.clone(), True).backward(go)
    F.relu(F.batch_norm(F.conv2d(ref[0], ref[1]), rm.clone(), rv.clone(), ref[2], ref[3], True, 0.1, 1e-5)).backward(go)
    for a, b in zip(leaves, ref):
        assert torch.equal(a.grad, b.grad)


def test_one_value_per_channel_is_torchs_value_error():
    maps, w, gamma, beta, rm, rv = _inputs(B=1, H=1, W=1)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        nfp_compress_map_tensors(maps, w, gamma, beta, rm, rv, True)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        nfp_compress_map(maps, w, torch.nn.BatchNorm2d(6))
    assert nfp_compress_map_tensors(maps, w, gamma, beta, rm, rv, False).shape == (1, 6, 1, 1)      # eval is fine


def test_malformed_arguments_are_refused():
    maps, w, gamma, beta, rm, rv = _inputs()
    with pytest.raises(RuntimeError, match="1x1 conv weight"):
        nfp_compress_map_tensors(maps, w[:, :4], gamma, beta, rm, rv, True)
    with pytest.raises(RuntimeError, match="expects"):
        nfp_compress_map_tensors(maps[0, 0], w, gamma, beta, rm, rv, True)
    with pytest.raises(RuntimeError, match="running mean and variance are required"):
        nfp_compress_map_tensors(maps, w, gamma, beta, None, None, False)


def test_routing_predicate(monkeypatch):
    """What cproj_hip_serves looks at, without a device."""
    class Fake:
        def __init__(self, shape, dtype=torch.float32, cuda=True, dense=True):
            self.shape, self.dtype, self.is_cuda, self._dense = torch.Size(shape), dtype, cuda, dense

        def is_contiguous(self):
            return self._dense

        def numel(self):
            return int(np.prod(self.shape))

    g = torch.ones(32)
    w = torch.ones(32, 8, 1, 1)
    serves = functional.cproj_hip_serves
    monkeypatch.setenv("NFP_CPROJ_TORCH", "0")
    assert serves(Fake((4, 8, 7, 7)), w, g, g, 0.1)
    assert serves(Fake((4, 8, 7, 7), torch.bfloat16), w, g, g, 0.1)
    assert serves(Fake((4, 32, 7, 7)), torch.ones(32, 32, 1, 1), g, g, 0.1)
    assert not serves(Fake((4, 33, 7, 7)), torch.ones(32, 33, 1, 1), g, g, 0.1)
    assert not serves(Fake((4, 8, 7, 7), cuda=False), w, g, g, 0.1)
    assert not serves(Fake((4, 8, 7, 7), torch.float16), w, g, g, 0.1)
    assert not serves(Fake((4, 8, 7, 7), torch.float64), w, g, g, 0.1)
    assert not serves(Fake((4, 8, 7, 7), dense=False), w, g, g, 0.1)
    assert not serves(Fake((0, 8, 7, 7)), w, g, g, 0.1)
    assert not serves(Fake((4, 8, 7, 7)), w, None, None, 0.1)                  # affine=False
    assert not serves(Fake((4, 8, 7, 7)), w, g, g, None)                       # a cumulative average
    assert not serves(Fake((1, 8, 2 ** 14, 2 ** 14)), w, g, g, 0.1)            # N * P = 2^31
    assert not serves(Fake((1, 1, 2 ** 13, 2 ** 13)), torch.ones(32, 1, 1, 1), g, g, 0.1)      # D * P = 2^31
    monkeypatch.setenv("NFP_CPROJ_TORCH", "1")                                 # the A/B switch, read at call time
    assert not serves(Fake((4, 8, 7, 7)), w, g, g, 0.1)
    monkeypatch.delenv("NFP_CPROJ_TORCH")
    # the default: what DESIGN 4g's table shows faster than the composition beyond the spread — at most 8 maps, and either
    # the train-mode step from 64 images of 54 x 54 map pixels up, or the forward on running statistics without a backward
    assert (functional.CPROJ_ROUTED_MAPS, functional.CPROJ_ROUTED_TRAIN_PIXELS) == (8, 64 * 54 * 54)
    w24 = torch.ones(24, 8, 1, 1)
    assert serves(Fake((64, 8, 54, 54)), w24, g, g, 0.1) and serves(Fake((64, 8, 110, 110)), w24, g, g, 0.1)
    assert serves(Fake((128, 8, 54, 27)), w24, g, g, 0.1, True, True)
    assert not serves(Fake((64, 8, 26, 26)), w24, g, g, 0.1) and not serves(Fake((4, 8, 7, 7)), w, g, g, 0.1)
    assert not serves(Fake((64, 24, 54, 54)), torch.ones(24, 24, 1, 1), g, g, 0.1)
    assert serves(Fake((4, 8, 7, 7)), w, g, g, 0.1, False, False)              # eval, nothing to differentiate
    assert not serves(Fake((4, 8, 7, 7)), w, g, g, 0.1, False, True)           # a backward on running statistics: not measured
    assert not serves(Fake((4, 24, 7, 7)), torch.ones(32, 24, 1, 1), g, g, 0.1, False, False)


def _bottleneck_step(m, x0, go):
    x = x0.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    out = m(x)
    out.backward(go)
    return out.detach(), x.grad, {k: p.grad for k, p in m.named_parameters()}, {k: v.clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("cin,cout,stride,train", [(16, 32, 1, True), (32, 32, 1, True), (16, 32, 2, True), (16, 32, 1, False)])
def test_bottleneck_fused_project_equals_the_two_ops(cin, cout, stride, train):
    torch.manual_seed(5)
    a = NFPBottleneck(cin, cout, stride)
    b = NFPBottleneck(cin, cout, stride, fused_project=True)
    assert not a.fused_project and b.fused_project and sorted(a.state_dict()) == sorted(b.state_dict())
    b.load_state_dict(a.state_dict(), strict=True)
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(3, cin, 10, 10, generator=gen)
    if not train:
        with torch.no_grad():
            a(x), b(x)
    a.train(train), b.train(train)
    go = torch.randn(a(x).shape, generator=gen)
    b(x)                                                   # (one step each before the compared one)
    ra, rb = _bottleneck_step(a, x, go), _bottleneck_step(b, x, go)
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
    assert sorted(ra[2]) == sorted(rb[2]) and all(g is not None for g in ra[2].values())
    for k in ra[2]:
        assert torch.equal(ra[2][k], rb[2][k]), k
    for k in ra[3]:
        assert torch.equal(ra[3][k], rb[3][k]), k


def test_bottleneck_fused_project_is_keyword_only():
    with pytest.raises(TypeError):
        NFPBottleneck(16, 32, 1, True)


@pytest.mark.parametrize("idx,kw", [(0, None), (3, dict(measure="cosine", padding=1, padding_mode="replicate")),
                                    (6, dict(measure="cosine", padding=1, padding_mode="replicate"))])
def test_insert_net_runs_a_step(idx, kw):
    torch.manual_seed(idx)
    m = NFPInsertNet(num_classes=5, nfp_insert_idx=idx, nfp_kwargs=kw)
    assert m.insert.in_channels == m.insert.out_channels == NFPInsertNet.BLOCK_CHANNELS[idx]
    out = m(torch.randn(2, 3, 32, 32))
    assert out.shape == (2, 5)
    F.cross_entropy(out, torch.tensor([1, 3])).backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert float(m.insert.nfp_proj[0].weight.grad.abs().max()) > 0
    assert int(m.insert.nfp_proj[1].num_batches_tracked) == 1


@pytest.mark.parametrize("idx", [7, -1, 1.0, None])
def test_insert_net_rejects_other_indices(idx):
    with pytest.raises(ValueError, match="nfp_insert_idx"):
        NFPInsertNet(nfp_insert_idx=idx)


def test_insert_net_block_ends_are_the_trunks_channel_counts():
    m = NFPInsertNet(nfp_insert_idx=2)
    x = torch.randn(1, 3, 64, 64)
    seen = []
    with torch.no_grad():
        for i, layer in enumerate(m.backbone.features.eval()):
            x = layer(x)
            if i in NFPInsertNet.BLOCK_ENDS:
                seen.append(x.shape[1])
    assert tuple(seen) == NFPInsertNet.BLOCK_CHANNELS


def test_header_binding_and_library_declare_the_cproj_calls():
    header = open(os.path.join(ROOT, "include", "nfp.h")).read()
    declared = set(re.findall(r"\b(nfp_[a-z0-9_]+)\s*\(", header))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(_abi.EXPORTS)
    assert "#define NFP_ABI_VERSION 7" in header or re.search(r"NFP_ABI_VERSION\s+7\b", header)
    if os.path.exists(_abi.LIB_PATH):
        L = _abi.load()
        for n in NEW_EXPORTS:
            assert hasattr(L, n), n
        # the forward's scratch is the moments'; the backward's: S slices of [D][N + 1], then [k, Q] per 32 channels
        assert L.nfp_cproj_scratch_floats(4, 8, 49, 32, 0) == L.nfp_cpool_scratch_floats(4, 8, 49, 32, 0)
        assert L.nfp_cproj_scratch_floats(4, 8, 49, 32, 1) == 4 * 32 * 9 + 1 * (8 + 64)       # one 64-pixel pass per image
        assert L.nfp_cproj_scratch_floats(2, 32, 1600, 16, 1) == 2 * 25 * 16 * 33 + 1 * (32 + 1024)
        assert L.nfp_cproj_scratch_floats(0, 8, 49, 32, 1) == 1 and L.nfp_cproj_scratch_floats(4, 33, 49, 32, 1) == 1
