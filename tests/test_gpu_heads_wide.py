"""NFPHead(R=3) and MultiRadiusNFPHead(R_list=(1, 2, 3)) on the MI355X — 48 and 80 NFP maps, the compress tail through the
wide kernels (NFP_CPOOL_TORCH=0) — against the reference's fixtures (tests/golden/cases_heads_wide.py), at test_gpu_heads.py's
bar: 1e-5 of each tensor's max magnitude.  With NFP_CPOOL_TORCH=1 the same step is the composition's."""
import pytest
import torch

import cases_heads_wide as KW
from test_heads_host import fixture_errors, head_module, run_head

pytestmark = pytest.mark.gpu

F32 = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from neighbour_feature_pooling_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


def _lib():
    from neighbour_feature_pooling_amd import _abi
    return _abi.load()


def _first_step_launches(m, c, dev):
    """Launches of the head's first step alone (GAP and the maps from one pass), forward and backward."""
    import cases_heads as KH
    x = torch.from_numpy(KH.make_input(c)).to(dev).requires_grad_(True)
    n0 = _lib().nfp_launch_count()
    gap, maps = m._gap_nfp(x)
    torch.autograd.grad([gap, maps], x, [torch.ones_like(gap), torch.ones_like(maps)])
    torch.cuda.synchronize()
    return _lib().nfp_launch_count() - n0, maps.shape[1]


@pytest.mark.parametrize("switch", ["0", "1"])
@pytest.mark.parametrize("name", [c["name"] for c in KW.HEAD_WIDE_CASES])
def test_head_matches_the_fixture(name, switch, dev, monkeypatch):
    monkeypatch.setenv("NFP_CPOOL_TORCH", switch)
    monkeypatch.delenv("NFP_CPOOL_WIDE", raising=False)
    c = KW.HEAD_WIDE_BY_NAME[name]
    m, g = head_module(c)
    m = m.to(dev)
    k_first, maps = _first_step_launches(m, c, dev)
    assert maps == KW.HEAD_WIDE_MAPS[name]
    n0 = _lib().nfp_launch_count()
    got = run_head(m, c, dev)
    torch.cuda.synchronize()
    k = _lib().nfp_launch_count() - n0
    if switch == "0":       # ... plus the wide tail: 5 + 3 launches in training, 1 + 3 in eval
        assert k == k_first + (8 if c["train"] else 4), (k, k_first)
    else:                   # the composition: nothing of the tail is ours
        assert k == k_first, (k, k_first)
    errs = fixture_errors(got, g)
    print(name, "NFP_CPOOL_TORCH=" + switch, errs)
    assert {"g:compress.0.weight", "g:compress.1.weight", "g:compress.1.bias", "after:compress.1.running_mean",
            "after:compress.1.running_var", "after:compress.1.num_batches_tracked"} <= set(errs)
    for key, e in errs.items():
        assert e <= F32, (key, e)
    moved = any(key.endswith("running_mean") and not (got[3][key] == g["p:" + key]).all() for key in got[3])
    assert moved == c["train"]
