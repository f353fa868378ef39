"""NFPPooling(bias=True) on the host: construction, reference-identical initialisation and state dict, the CPU
formulation against the reference's fixtures (tests/golden/bias_*.npz, make_golden_bias.py), the ABI 7 declarations and
a two-rank DDP step.  No GPU needed."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cases as K
import cases_bias as KB
from conftest import ROOT, assert_matches_golden, load_golden, rel_err
from neighbour_feature_pooling_amd import NFPPooling, _abi
from neighbour_feature_pooling_amd.nfp import EnhancedNFPPooling, MultiRadiusNFPPooling


def _module(c, dtype=torch.float32):
    """The case's module with the fixture's biases."""
    g = load_golden(c["name"])
    m = NFPPooling(c["shape"][1], bias=True, **c["ctor"])
    with torch.no_grad():
        m.center_value.bias.copy_(torch.from_numpy(g["bc"]))
        m.comp_neighbors.bias.copy_(torch.from_numpy(g["nb"]))
    return m.to(dtype), g


def test_construction_and_parameters():
    C = 6
    m = NFPPooling(C, R=1, measure="cosine", padding=1, bias=True)
    params = dict(m.named_parameters())
    assert sorted(params) == ["center_value.bias", "comp_neighbors.bias"]
    assert params["comp_neighbors.bias"].shape == (C * 8,) and params["center_value.bias"].shape == (C,)
    assert all(p.requires_grad for p in params.values())
    m2 = NFPPooling(C, R=2, measure="norm", padding=2, bias=True)
    assert m2.comp_neighbors.bias.shape == (C * 24,)
    # the subclasses pass bias through **kw
    assert EnhancedNFPPooling(4, R=1, measure="cosine", padding=1, bias=True).comp_neighbors.bias.shape == (32,)
    mr = MultiRadiusNFPPooling(4, R_list=(1, 2), bias=True)
    assert sorted(n for n, _ in mr.named_parameters()) == sorted(
        f"nfp_blocks.{i}.{k}.bias" for i in (0, 1) for k in ("comp_neighbors", "center_value"))
    assert "bias=True" in repr(m)


def test_bias_false_is_unchanged():
    torch.manual_seed(3)
    m = NFPPooling(5, R=1, measure="cosine", padding=1)
    after = torch.rand(4)
    torch.manual_seed(3)
    assert torch.equal(after, torch.rand(4))       # no RNG use
    assert list(m.parameters()) == []
    assert sorted(m.state_dict()) == ["center_value.weight", "comp_neighbors.weight"]


@pytest.mark.parametrize("name,C,ctor,seed", KB.INIT_CASES, ids=[c[0] for c in KB.INIT_CASES])
def test_init_matches_the_reference_bitwise(name, C, ctor, seed):
    g = load_golden(name)
    torch.manual_seed(seed)
    m = NFPPooling(C, bias=True, **ctor)
    assert np.array_equal(m.center_value.bias.detach().numpy(), g["bc"])
    assert np.array_equal(m.comp_neighbors.bias.detach().numpy(), g["nb"])


def test_state_dict_round_trip_and_reference_layout():
    c = KB.BIAS_BY_NAME["bias_m_cosine"]
    m, g = _module(c)
    sd = m.state_dict()
    assert sorted(sd) == ["center_value.bias", "center_value.weight", "comp_neighbors.bias", "comp_neighbors.weight"]
    C, k = c["shape"][1], 3
    assert sd["comp_neighbors.weight"].shape == (C * 8, 1, k, k) and sd["center_value.weight"].shape == (C, 1, k, k)
    # a reference-shaped state dict (frozen one-hot weights + the fixture's biases) loads strictly
    ref_sd = {"comp_neighbors.weight": sd["comp_neighbors.weight"].clone(), "center_value.weight": sd["center_value.weight"].clone(),
              "comp_neighbors.bias": torch.from_numpy(g["nb"]), "center_value.bias": torch.from_numpy(g["bc"])}
    fresh = NFPPooling(C, bias=True, **c["ctor"])
    fresh.load_state_dict(ref_sd, strict=True)
    assert torch.equal(fresh.comp_neighbors.bias.detach(), torch.from_numpy(g["nb"]))
    assert torch.equal(fresh.center_value.bias.detach(), torch.from_numpy(g["bc"]))


def run_case(m, c, dtype=torch.float64, dev="cpu", channels_last=False):
    x = torch.from_numpy(K.make_input(c)).to(dtype).to(dev)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    out = m(x)
    go = torch.from_numpy(K.make_grad_out(c, tuple(out.shape))).to(dtype).to(dev)
    out.backward(go)
    gbc = m.center_value.bias.grad
    return (out.detach().float().cpu().numpy(), x.grad.float().cpu().numpy(),
            None if gbc is None else gbc.float().cpu().numpy(), m.comp_neighbors.bias.grad.float().cpu().numpy())


def check_bias_grads(gbc, gnb, g, tol):
    assert rel_err(gnb, g["gnb"]) <= tol
    if int(g["gbc_none"]):
        assert gbc is None
    else:
        assert gbc is not None and rel_err(gbc, g["gbc"]) <= tol


@pytest.mark.parametrize("name", [c["name"] for c in KB.BIAS_CASES])
def test_cpu_matches_reference_fixture(name):
    c = KB.BIAS_BY_NAME[name]
    m, g = _module(c)
    out, gx, gbc, gnb = run_case(m, c, torch.float32)     # (float32, as the reference ran)
    assert_matches_golden(out, gx, g, 1e-5)
    check_bias_grads(gbc, gnb, g, 1e-5)


@pytest.mark.parametrize("measure", ["cosine", "norm", "Norm", "pearson", "attention", "smith"])
def test_zero_biases_reproduce_the_unbiased_map(measure):
    torch.manual_seed(0)
    x = torch.randn(2, 6, 7, 5, dtype=torch.float64)
    mb = NFPPooling(6, R=1, measure=measure, padding=1, padding_mode="zeros", bias=True).double()
    with torch.no_grad():
        mb.comp_neighbors.bias.zero_()
        mb.center_value.bias.zero_()
    mu = NFPPooling(6, R=1, measure=measure, padding=1, padding_mode="zeros").double()
    assert torch.allclose(mb(x), mu(x), rtol=0, atol=1e-12)


def test_zero_padded_taps_carry_the_bias():
    """nn.Conv2d adds its bias after padding: on an all-zero input Norm reads -sum_c |beta[c, n]| everywhere."""
    m = NFPPooling(3, R=1, measure="norm", padding=1, padding_mode="zeros", bias=True)
    out = m(torch.zeros(1, 3, 4, 4))
    expect = -m.comp_neighbors.bias.detach().reshape(3, 8).abs().sum(0)
    assert torch.allclose(out[0], expect[:, None, None].expand(8, 4, 4))


def test_new_exports_are_declared_and_versioned():
    src = open(os.path.join(ROOT, "include", "nfp.h")).read()
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(nfp_[a-z_]+)\s*\(", body))
    new = {"nfp_bias_saved_floats", "nfp_bias_scratch_floats", "nfp_bias_forward", "nfp_bias_backward"}
    assert new <= declared and new <= set(_abi.EXPORTS)
    assert int(re.search(r"#define NFP_ABI_VERSION (\d+)", src).group(1)) == _abi.ABI_VERSION == 7
    from neighbour_feature_pooling_amd.build import build_hip
    build_hip()
    L = _abi.load()
    for n in new:
        assert hasattr(L, n)
    assert L.nfp_abi_version() == 7


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _net():
    torch.manual_seed(5)
    return torch.nn.Sequential(NFPPooling(4, R=1, measure="cosine", padding=1, bias=True), torch.nn.Flatten(),
                               torch.nn.Linear(8 * 5 * 5, 3))


def _batch():
    g = torch.Generator().manual_seed(9)
    return torch.randn(4, 4, 5, 5, generator=g), torch.randint(0, 3, (4,), generator=g)


def _ddp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from torch.nn.parallel import DistributedDataParallel as DDP
        net = _net()
        ddp = DDP(net)
        x, y = _batch()
        lo, hi = rank * 2, rank * 2 + 2
        torch.nn.CrossEntropyLoss()(ddp(x[lo:hi]), y[lo:hi]).backward()
        if rank == 0:
            np.savez(os.path.join(out_dir, "ddp.npz"),
                     **{k.replace(".", "/"): p.grad.numpy() for k, p in net.named_parameters()})
    finally:
        dist.destroy_process_group()


def test_ddp_two_ranks_bias_gradients(tmp_path):
    world = 2
    mp.spawn(_ddp_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = np.load(tmp_path / "ddp.npz")
    net = _net()
    x, y = _batch()
    torch.nn.CrossEntropyLoss()(net(x), y).backward()
    for k, p in net.named_parameters():
        np.testing.assert_allclose(got[k.replace(".", "/")], p.grad.numpy(), rtol=1e-5, atol=1e-6)
    assert "0/comp_neighbors/bias" in got.files and "0/center_value/bias" in got.files
