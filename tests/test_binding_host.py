"""The Python binding's own bookkeeping (functional.py / _ops.py), checked WITHOUT a GPU: one descriptor builder behind
every user, the shape-only scratch bounds of the compiled graph, and what the plan cache keeps and forgets."""
import ctypes
import gc
import itertools
from collections import OrderedDict

import pytest
import torch

from neighbour_feature_pooling_amd import _abi, _ops
from neighbour_feature_pooling_amd import functional as F
from neighbour_feature_pooling_amd.build import build_hip


@pytest.fixture(scope="module")
def lib():
    build_hip()
    return _abi.load()


def _cfg(measure, p=1, R=1, inner_R=0):
    return F.NfpConfig(R=R, measure=measure, p=p, padding=R, diff_weights=measure in ("norm", "rmse"), inner_R=inner_R)


def _tensors(dtype):
    tok = torch.zeros(4, 1 + 30, 8, dtype=dtype)
    return {"nchw": torch.zeros(2, 8, 6, 6, dtype=dtype),
            "channels_last": torch.zeros(2, 8, 6, 6, dtype=dtype).contiguous(memory_format=torch.channels_last),
            "class_token_view": tok[:, 1:].transpose(1, 2).unflatten(2, (5, 6)),
            "one": torch.zeros(1, 1, 1, 1, dtype=dtype)}


MEASURES = [(m, 1) for m in _abi.MEASURES] + [("norm", 2)]
RADII = [(1, 0), (2, 0), (2, 1)]        # (R, inner_R)


@pytest.mark.parametrize("kind", ["nchw", "channels_last", "class_token_view", "one"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_one_builder_and_its_four_users_agree(kind, dtype, lib):
    """make_desc is build_desc on the tensor's shape and canonical strides; the shape-only sizes the fake implementations
    state (_ops._saved_floats, _ops._bias_saved_floats: a dense NCHW descriptor) are the library's sizes for the tensor's
    own descriptor, whatever its layout and batch stride."""
    x = _tensors(dtype)[kind]
    assert F._inner_layout(x) == F._layout_of(tuple(x.shape), x.stride()) == F._dense(x)[1]
    for (measure, p), (R, inner_R) in itertools.product(MEASURES, RADII):
        cfg = _cfg(measure, p, R, inner_R)
        d = F.make_desc(x, cfg)
        xd, layout = F._dense(x)
        assert xd is x
        assert bytes(d) == bytes(F.build_desc(x.shape, F._canonical_strides(x, layout), x.dtype, cfg)), (measure, p, R, inner_R)
        assert not d.ws
        shape = tuple(x.shape)
        assert _ops._saved_floats(shape, dtype, cfg, True) == max(lib.nfp_saved_floats(ctypes.byref(d)), 0), cfg
        if inner_R == 0:
            assert _ops._bias_saved_floats(shape, dtype, cfg) == max(lib.nfp_bias_saved_floats(ctypes.byref(d)), 0), cfg


def test_static_servability_builds_the_same_descriptor(lib, monkeypatch):
    """gap_servable_static goes through build_desc too: the descriptor it asks the library about is the tensor's own
    (plus the stand-in workspace)."""
    seen = []
    real = F.build_desc
    monkeypatch.setattr(F, "build_desc", lambda *a: seen.append(real(*a)) or seen[-1])
    cfg = _cfg("cosine")
    for x in _tensors(torch.float32).values():
        seen.clear()
        F.gap_servable_static(tuple(x.shape), x.stride(), x.dtype, cfg)
        d = F.make_desc(x, cfg)
        seen[0].ws = None
        assert bytes(seen[0]) == bytes(d)


@pytest.mark.parametrize("shape", [(2, 8, 6, 6), (2, 16, 24, 24), (1, 4, 3, 300), (2, 8, 40, 3)])
def test_the_compiled_graphs_scratch_bounds_hold(shape, lib):
    """What the compiled graph allocates from the shape alone (_pool_saved_bound, _gap_saved_bound) is never less than what
    the library asks for on the descriptor it would run: a dry run with the workspace stood in for."""
    served = 0
    for (measure, p), layout, dtype in itertools.product([("cosine", 1), ("norm", 2)], ["nchw", "nhwc"],
                                                         [torch.float32, torch.bfloat16]):
        cfg = _cfg(measure, p)
        d = F.build_desc(shape, F._canon(shape, layout), dtype, cfg)
        if lib.nfp_workspace_bytes(ctypes.byref(d)) > 0:
            d.ws = 0x1000       # (never dereferenced: nothing is launched)
        if lib.nfp_pool_supported(ctypes.byref(d)):
            served += 1
            need, bound = lib.nfp_pool_saved_floats(ctypes.byref(d)), _ops._pool_saved_bound(shape, dtype, cfg)
            print(shape, measure, layout, dtype, "pool", need, bound)
            assert bound >= need
        if lib.nfp_gap_supported(ctypes.byref(d)):
            served += 1
            need, bound = lib.nfp_gap_saved_floats(ctypes.byref(d)), _ops._gap_saved_bound(shape, dtype, cfg)
            print(shape, measure, layout, dtype, "gap", need, bound)
            assert bound >= need
    if shape[3] <= 254:         # (rows the pooled kernels take: the test must not pass by asking nothing)
        assert served


@pytest.fixture
def host_plans(monkeypatch, lib):
    """An empty plan cache of the test's own, and no workspace: planning then touches no device."""
    monkeypatch.setattr(F, "_PLANS", OrderedDict())
    monkeypatch.setattr(F, "_workspace", lambda d, device: None)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    return F


def test_a_cleared_or_replaced_cache_forgets_everything(host_plans, monkeypatch):
    x, cfg = torch.zeros(2, 16, 24, 24), _cfg("cosine")
    p1 = F._plan(x, "nchw", cfg)
    assert F._plan(x, "nchw", cfg) is p1 and list(F._PLANS.values()) == [p1]
    ns = p1.ask("nfp_pool_saved_floats")
    assert ns > 0 and p1._asked == {"nfp_pool_saved_floats": ns} and list(F._PLANS.values()) == [p1]
    F._PLANS.clear()
    p2 = F._plan(x, "nchw", cfg)
    assert p2 is not p1 and p2._asked == {}
    monkeypatch.setattr(F, "_PLANS", OrderedDict())
    p3 = F._plan(x, "nchw", cfg)
    assert p3 is not p2 and p3._asked == {} and list(F._PLANS.values()) == [p3]
    assert (p3.oshape, p3.saved_floats, p3.no_bwd, p3.cacheable, p3.nhwc) == ((2, 8, 24, 24), 2 * 576, None, True, False)


def test_a_plan_made_under_capture_without_tables_is_not_cached(host_plans, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    x, cfg = torch.zeros(2, 16, 24, 24), _cfg("cosine")
    p1 = F._plan(x, "nchw", cfg)
    assert not p1.cacheable and not p1.desc.ws and len(F._PLANS) == 0
    p1.ask("nfp_pool_supported"), p1.ask("nfp_gap_supported"), p1.ask("nfp_pool_saved_floats"), p1.ask("nfp_gap_saved_floats")
    assert len(F._PLANS) == 0
    assert F._plan(x, "nchw", cfg) is not p1 and len(F._PLANS) == 0
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    p2 = F._plan(x, "nchw", cfg)
    assert p2.cacheable and p2._asked == {} and list(F._PLANS.values()) == [p2]


def test_the_descriptor_tensor_outlives_its_plan(host_plans):
    x, cfg = torch.zeros(3, 8, 5, 7), _cfg("norm", 2, R=2)
    plan = F._plan(x, "nchw", cfg)
    t, want = plan.desc_tensor, bytes(plan.desc)
    assert t.numel() == ctypes.sizeof(_abi.NfpDesc) and t.data_ptr() == ctypes.addressof(plan.desc)
    del plan
    F._PLANS.clear()
    gc.collect()
    junk = [F.build_desc((1, 1, 1, 1), (1, 1, 1, 1), torch.float32, _cfg("dot")) for _ in range(64)]   # reuse freed memory, if any
    assert bytes(t.numpy()) == want and len(junk) == 64
