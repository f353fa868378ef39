"""NFPHead, MultiRadiusNFPHead and AdaptiveFusionNFP on the MI355X: against the reference's fixtures (tests/golden/head_*.npz)
and against their own CPU run, the running statistics after a train step, the peak memory of the fused tail, and
NFPHeadNet(fused_compress=True) against its default.  Bar: 1e-5 of each tensor's max magnitude (float32)."""
import pytest
import torch

import cases_heads as KH
from conftest import rel_err
from test_heads_host import fixture_errors, head_module, run_head

pytestmark = pytest.mark.gpu

F32 = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from neighbour_feature_pooling_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


def _count():
    from neighbour_feature_pooling_amd import _abi
    return _abi.load().nfp_launch_count()


@pytest.mark.parametrize("name", [c["name"] for c in KH.HEAD_CASES])
def test_head_matches_the_fixture_and_its_cpu_run(name, dev, monkeypatch):
    monkeypatch.setenv("NFP_CPOOL_TORCH", "0")      # the HIP tail also for MultiRadiusNFPHead's 32 maps (routed away by default)
    c = KH.HEAD_BY_NAME[name]
    m, g = head_module(c)
    cpu = run_head(m, c)
    m, _ = head_module(c, g)
    m = m.to(dev)
    # launches of the head's first step alone (GAP and the maps from one pass), each way
    x = torch.from_numpy(KH.make_input(c)).to(dev).requires_grad_(True)
    n0 = _count()
    gap, maps = m._gap_nfp(x)
    k_first = _count() - n0
    torch.autograd.grad([gap, maps], x, [torch.ones_like(gap), torch.ones_like(maps)])
    torch.cuda.synchronize()
    k_first = _count() - n0
    n0 = _count()
    got = run_head(m, c, dev)
    torch.cuda.synchronize()
    # ... plus the tail: 3 + 3 launches in training, 1 + 3 in eval — nothing else of the head is ours
    assert _count() - n0 == k_first + (6 if c["train"] else 4), (_count() - n0, k_first)
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
    # the train step moved the running statistics (and eval left them)
    moved = any(k.endswith("running_mean") and not (got[3][k] == g["p:" + k]).all() for k in got[3])
    assert moved == c["train"]


def test_fused_tail_never_holds_the_compress_activation(dev):
    """[64,8,14,14] -> D = 512: forward plus backward of the fused tail raises the peak by less than ONE [B,D,P] float32
    activation (the composition holds several)."""
    from neighbour_feature_pooling_amd import nfp_compress_pool
    B, N, H, D = 64, 8, 14, 512
    torch.manual_seed(0)
    maps = torch.randn(B, N, H, H, device=dev, requires_grad=True)
    conv = torch.nn.Conv2d(N, D, 1, bias=False).to(dev)
    bn = torch.nn.BatchNorm2d(D).to(dev)
    go = torch.randn(B, D, device=dev)
    one = B * D * H * H * 4

    def step():
        out = nfp_compress_pool(maps, conv.weight, bn)
        out.backward(go)
        maps.grad = conv.weight.grad = bn.weight.grad = bn.bias.grad = None

    step()      # (first-call allocations: the library, the caching allocator's pools)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    n0 = _count()
    step()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(dev) - base
    print("peak rise", rise, "one activation", one)
    assert _count() - n0 == 6 and rise < one


def test_head_net_with_the_fused_tail_agrees_with_the_default(dev):
    from neighbour_feature_pooling_amd.models import NFPHeadNet
    torch.manual_seed(5)
    a = NFPHeadNet(num_classes=5, bottleneck_dim=24).to(dev)
    b = NFPHeadNet(num_classes=5, bottleneck_dim=24, fused_compress=True).to(dev)
    b.load_state_dict(a.state_dict(), strict=True)
    x = torch.randn(4, 3, 96, 96, device=dev)
    gy = torch.randn(4, 5, device=dev)
    n0 = _count()
    ya = a(x)
    ka = _count() - n0
    ya.backward(gy)
    n0 = _count()
    yb = b(x)
    assert _count() - n0 == ka + 3          # the default's launches plus the tail's three
    yb.backward(gy)
    torch.cuda.synchronize()
    assert rel_err(yb.detach().cpu().numpy(), ya.detach().cpu().numpy()) <= F32
    for k in ("compress.1.running_mean", "compress.1.running_var", "compress.1.num_batches_tracked"):
        va, vb = a.state_dict()[k], b.state_dict()[k]
        assert rel_err(vb.float().cpu().numpy(), va.float().cpu().numpy()) <= F32, k
    # The gradients are printed, not held to a bar here: both arms are float32 computations with errors of their own against
    # exact arithmetic.  test_gpu_cpool.py holds the tail's gradients to the float64 composition, the fixture tests above a
    # whole head's to the reference's.
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        if k.startswith("compress") or k.startswith("fc"):
            assert pb.grad is not None and torch.isfinite(pb.grad).all()
            print(k, rel_err(pb.grad.cpu().numpy(), pa.grad.cpu().numpy()))
