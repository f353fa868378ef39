"""NFPInsert, NFPBottleneck(fused_project=True) and NFPInsertNet on the MI355X with the projection on the cproj kernels
(NFP_CPROJ_TORCH=0): the block against the reference's fixtures (tests/golden/insert_*.npz) and its own CPU run, the
bottleneck with its bn2(conv2(.)) as one call against the existing bneck_*.npz fixtures at test_gpu_bottleneck.py's bars,
and one train step of the whole net.  Bar: 1e-5 of each tensor's max magnitude (float32)."""
import pytest
import torch

import cases_bottleneck as KB
import cases_insert as KI
from conftest import load_golden, rel_err
from test_bottleneck_host import fixture_errors as bneck_errors
from test_bottleneck_host import run_bneck
from test_gpu_bottleneck import BARS, kind_of
from test_insert_host import fixture_errors, insert_module, run_insert

pytestmark = pytest.mark.gpu

F32 = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from neighbour_feature_pooling_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _hip_projection(monkeypatch):
    monkeypatch.setenv("NFP_CPROJ_TORCH", "0")


def _lib():
    from neighbour_feature_pooling_amd import _abi
    return _abi.load()


@pytest.mark.parametrize("name", [c["name"] for c in KI.INSERT_CASES])
def test_insert_matches_the_fixture_and_its_cpu_run(name, dev):
    c = KI.INSERT_BY_NAME[name]
    m, g = insert_module(c)
    cpu = run_insert(m, c)
    m = insert_module(c, g)[0].to(dev)
    # the layer's own launches, each way
    x = torch.from_numpy(KI.make_input(c)).to(dev).requires_grad_(True)
    n0 = _lib().nfp_launch_count()
    maps = m.nfp(x)
    torch.autograd.grad(maps, x, torch.ones_like(maps))
    torch.cuda.synchronize()
    k_layer = _lib().nfp_launch_count() - n0
    n0 = _lib().nfp_launch_count()
    got = run_insert(m, c, dev)
    torch.cuda.synchronize()
    # ... plus the projection: 3 + 3 launches in training, 1 + 3 in eval
    assert _lib().nfp_launch_count() - n0 == k_layer + (6 if c["train"] else 4), (_lib().nfp_launch_count() - n0, k_layer)
    errs = fixture_errors(got, g)
    print(name, "fixture", errs)
    for k, e in errs.items():
        assert e <= F32, (k, e)
    own = {"out": rel_err(got[0], cpu[0]), "grad_x": rel_err(got[1], cpu[1])}
    own.update({"g:" + k: rel_err(got[2][k], cpu[2][k]) for k in cpu[2]})
    own.update({"after:" + k: rel_err(got[3][k], cpu[3][k]) for k in cpu[3]})
    print(name, "own CPU run", own)
    for k, e in own.items():
        assert e <= F32, (k, e)
    moved = any(k.endswith("running_mean") and not (got[3][k] == g["p:" + k]).all() for k in got[3])
    assert moved == c["train"]


@pytest.mark.parametrize("name", [c["name"] for c in KB.BNECK_CASES])
def test_bottleneck_with_the_fused_projection_matches_the_fixture(name, dev):
    from neighbour_feature_pooling_amd import NFPBottleneck
    c = KB.BNECK_BY_NAME[name]
    g = load_golden(name)
    m = NFPBottleneck(c["cin"], c["cout"], c["stride"], fused_project=True)
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p:")}, strict=True)
    m.train(c["train"])
    m = m.to(dev)
    seen = []
    hook = m.bn2.register_forward_hook(lambda *a: seen.append("bn2"))         # (the two ATen ops must not run)
    n0 = _lib().nfp_launch_count()
    got = run_bneck(m, c, dev)
    torch.cuda.synchronize()
    hook.remove()
    assert not seen
    # the layer's one launch each way, plus the projection: 3 + 3 in training, 1 + 3 in eval
    assert _lib().nfp_launch_count() - n0 == 2 + (6 if c["train"] else 4)
    errs = bneck_errors(got, g)
    print(name, errs)
    for k, e in errs.items():
        assert e <= BARS[kind_of(k)], (k, e)


def test_the_fused_bottleneck_launches_the_projection_kernels(dev):
    from neighbour_feature_pooling_amd import NFPBottleneck
    torch.manual_seed(0)
    m = NFPBottleneck(16, 32, fused_project=True).to(dev)
    x = torch.randn(4, 16, 9, 9, device=dev)
    L = _lib()
    with torch.no_grad():
        n0 = L.nfp_launch_count()
        m(x)
        assert L.nfp_launch_count() - n0 == 1 + 3 and L.nfp_last_variant().decode() == "cproj_fwd<f32,train,lin>"
        m.eval()
        n0 = L.nfp_launch_count()
        m(x)
        assert L.nfp_launch_count() - n0 == 1 + 1 and L.nfp_last_variant().decode() == "cproj_fwd<f32,eval,lin>"


def test_insert_net_takes_a_train_step(dev):
    from neighbour_feature_pooling_amd.models import NFPInsertNet
    torch.manual_seed(0)
    m = NFPInsertNet(num_classes=5, nfp_insert_idx=1).to(dev)
    opt = torch.optim.SGD(m.parameters(), lr=0.01)
    x = torch.randn(4, 3, 64, 64, device=dev)
    L = _lib()
    n0 = L.nfp_launch_count()
    out = m(x)
    assert L.nfp_last_variant().decode() == "cproj_fwd<f32,train,relu>"
    loss = torch.nn.functional.cross_entropy(out, torch.tensor([0, 1, 2, 3], device=dev))
    loss.backward()
    torch.cuda.synchronize()
    assert L.nfp_launch_count() - n0 >= 6 + 2
    assert out.shape == (4, 5) and bool(torch.isfinite(loss))
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert float(m.insert.nfp_proj[0].weight.grad.abs().max()) > 0
    opt.step()
    assert int(m.insert.nfp_proj[1].num_batches_tracked) == 1
