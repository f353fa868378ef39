"""The two kinds of plan behind `functional._plan` — with the workspace tables (the maps', pooled and GAP kernels) and without
(the biased and the valid-map kernels) — checked WITHOUT a GPU: what a table-less plan skips, that the kinds do not share
cache entries, that both valid families ask the one plan of a signature, and that the LRU bound covers both kinds."""
from collections import OrderedDict

import pytest
import torch

from neighbour_feature_pooling_amd import _abi
from neighbour_feature_pooling_amd import functional as F
from neighbour_feature_pooling_amd.build import build_hip


@pytest.fixture(scope="module")
def lib():
    build_hip()
    return _abi.load()


@pytest.fixture
def host_plans(monkeypatch, lib):
    """An empty plan cache of the test's own, and no workspace: planning then touches no device."""
    monkeypatch.setattr(F, "_PLANS", OrderedDict())
    monkeypatch.setattr(F, "_workspace", lambda d, device: None)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    return F


COSINE0 = F.NfpConfig(R=1, measure="cosine", padding=0, diff_weights=False)
NORM1_0 = F.NfpConfig(R=1, measure="norm", p=1, padding=0, diff_weights=True)


def _x():
    return torch.zeros(2, 8, 6, 6)


def test_a_table_less_plan_touches_neither_workspace_nor_dry_run(host_plans, monkeypatch):
    def no_workspace(d, device):
        raise AssertionError("a table-less plan asked for a workspace")

    def no_ordering(device):
        raise AssertionError("a table-less plan ordered itself after table fills")

    monkeypatch.setattr(F, "_workspace", no_workspace)
    monkeypatch.setattr(F, "_order_after_fills", no_ordering)
    monkeypatch.setattr(F, "_PENDING_FILLS", [object()])        # (a fill in flight: only a table plan may look at it)
    x = _x()
    plan = F._plan(x, "nchw", COSINE0, tables=False)
    assert not plan.desc.ws
    assert (plan.no_bwd, plan.no_fwd, plan.saved_floats, plan.cacheable, plan._asked) == (None, None, 0, True, {})
    assert plan.oshape == (2, 8, 4, 4) and not plan.nhwc
    assert bytes(plan.desc) == bytes(F.make_desc(x, COSINE0, "nchw"))
    assert F._plan(x, "nchw", COSINE0, tables=False) is plan and list(F._PLANS.values()) == [plan]
    with pytest.raises(AssertionError, match="ordered itself after table fills"):
        F._plan(x, "nchw", COSINE0)                             # (the table kind does go there ...)
    monkeypatch.setattr(F, "_PENDING_FILLS", [])
    with pytest.raises(AssertionError, match="asked for a workspace"):
        F._plan(x, "nchw", COSINE0)                             # (... and there)


def test_the_two_kinds_of_one_signature_are_two_entries(host_plans):
    x = _x()
    with_tables = F._plan(x, "nchw", COSINE0)
    without = F._plan(x, "nchw", COSINE0, tables=False)
    assert with_tables is not without and len(F._PLANS) == 2
    assert F._plan(x, "nchw", COSINE0, tables=True) is with_tables and F._plan(x, "nchw", COSINE0, tables=False) is without
    assert with_tables.saved_floats == 2 * 36 and without.saved_floats == 0     # (only the table kind asks nfp_saved_floats)
    assert bytes(with_tables.desc) == bytes(without.desc)                       # (no workspace on the host: the same bytes)
    assert len(set(F._PLANS)) == 2 and len({k[-6:] for k in F._PLANS}) == 1     # the keys differ in the kind alone


@pytest.mark.parametrize("cfg, valid, valid_abs", [(COSINE0, 1, 0), (NORM1_0, 0, 1)])
def test_both_valid_families_ask_the_one_table_less_plan(cfg, valid, valid_abs, host_plans):
    x = _x()
    plan = F._plan(x, "nchw", cfg, tables=False)
    assert plan.ask(F.VALID.supported) == valid and plan.ask(F.VALID_ABS.supported) == valid_abs
    assert (F.VALID.supported, F.VALID_ABS.supported) == ("nfp_valid_supported", "nfp_valid_abs_supported")
    assert plan._asked == {"nfp_valid_supported": valid, "nfp_valid_abs_supported": valid_abs}
    assert list(F._PLANS.values()) == [plan]                    # one plan per configuration, whichever family asks
    assert F._plan(x, "nchw", cfg, tables=False)._asked is plan._asked


def test_the_lru_bound_holds_across_kinds(host_plans, monkeypatch):
    monkeypatch.setattr(F, "_PLANS_MAX", 6)
    x = _x()
    cfgs = [F.NfpConfig(R=1, measure="cosine", padding=0, diff_weights=False, eps=10.0 ** -(i + 3)) for i in range(5)]
    first = F._plan(x, "nchw", cfgs[0], tables=False)
    for cfg in cfgs:
        F._plan(x, "nchw", cfg, tables=True)
        F._plan(x, "nchw", cfg, tables=False)
        assert F._plan(x, "nchw", cfgs[0], tables=False) is first           # kept hot: never the one to go
        assert len(F._PLANS) <= 6
    assert len(F._PLANS) == 6
    kinds = [k[0] == "no tables" for k in F._PLANS]
    assert any(kinds) and not all(kinds)                        # one LRU: both kinds live in it, and both were evicted from it
    assert F._plan(x, "nchw", cfgs[0], tables=True).oshape == (2, 8, 4, 4) and len(F._PLANS) == 6
