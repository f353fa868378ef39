"""The wide form of the heads' compress-BN-ReLU-GAP tail on the MI355X (csrc/nfp_cpool.hip: the cpw kernels, include/nfp.h
nfp_cpool_wide_*; 33 to 96 maps) against the float64 torch composition of the same inputs, with test_gpu_cpool.py's recipe,
helpers and bars: 1e-5 of each tensor's max magnitude for float32 (grad_w 5e-5), 1e-2 / 2e-2 for bf16 maps.

Every case fixes the first seed for which the float64 reference keeps min|a| >= 1e-5 max|a| in training and in eval (and,
for the two bf16 cases, on the bf16-rounded maps too), searched on the CPU; the guard is asserted on the reference before
anything is compared, and no element is excluded.

Launch budgets: forward 5 in training (moments, mu, Sigma, var, main) and 1 in eval; backward at most 3."""
import functools
from unittest import mock

import pytest
import torch

import test_gpu_cpool as base
from test_gpu_cpool import errors, reference64, run_hip
from conftest import rel_err

pytestmark = pytest.mark.gpu

F32, F32_GW, BF_OUT, BF_GRAD, GUARD = base.F32, base.F32_GW, base.BF_OUT, base.BF_GRAD, base.GUARD

# name: (maps shape, D, seed, what it covers) — added to a copy of test_gpu_cpool.CASES
WIDE_CASES = dict(base.CASES)
WIDE_CASES.update({
    "n33": ((3, 33, 5, 7), 48, 2, "the first count past the old limit, padded rows, non-square"),
    "r3_head": ((4, 48, 7, 7), 40, 0, "the R = 3 head"),
    "three_radii": ((3, 80, 7, 7), 130, 1, "80 maps, three D tiles with a ragged last one"),
    "n96_chunked": ((2, 96, 16, 16), 24, 0, "the maximum, an image walked in several chunks"),
    "one_pixel_wide": ((5, 40, 1, 1), 16, 0, "P = 1"),
    "one_image_wide": ((1, 48, 7, 7), 32, 0, "B = 1"),
    "zero_row_wide": ((4, 48, 7, 7), 32, 5, "an all-zero weight row: var = 0, a = beta"),
})
NEW = [n for n in WIDE_CASES if n not in base.CASES]
MODES = base.MODES


def make_inputs(name):
    with mock.patch.object(base, "CASES", WIDE_CASES):
        ins = base.make_inputs(name)
    if name == "zero_row_wide":
        ins[1][3] = 0
    return ins


@functools.lru_cache(maxsize=None)
def case_ref(name, training, bf16=False):
    """(inputs, float64 reference) of a case — computed once, shared by the tests, never modified."""
    ins = make_inputs(name)
    return ins, reference64(ins, training, torch.bfloat16 if bf16 else torch.float32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from neighbour_feature_pooling_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _hip_tail_wherever_it_can_serve(monkeypatch):
    """NFP_CPOOL_TORCH=0: the kernels wherever any form can serve (by default 33 to 96 maps are the composition's)."""
    monkeypatch.setenv("NFP_CPOOL_TORCH", "0")
    monkeypatch.delenv("NFP_CPOOL_WIDE", raising=False)


def _lib():
    from neighbour_feature_pooling_amd import _abi
    return _abi.load()


def _variant():
    return _lib().nfp_last_variant().decode()


def _np16(n):
    return (n + 15) // 16 * 16


def _check_f32(ins, ref, got, training, maps):
    e = errors(got, ref)
    assert got["out"].dtype == torch.float32 and got["gm"].shape == ins[0].shape and got["gw"].shape == ins[1].shape
    for k in ("out", "gm", "gg", "gb"):
        assert e[k] <= F32, (k, e[k])
    assert e["gw"] <= F32_GW, e["gw"]
    assert _variant() == f"cpool_wide_bwd<f32,{'train' if training else 'eval'},n{_np16(maps)}>"
    return e


@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("name", NEW)
def test_float32_matches_the_float64_composition(name, training, dev):
    ins, ref = case_ref(name, training)
    assert ref["guard"] >= GUARD, ref["guard"]
    got = run_hip(ins, training, dev)
    print(name, "train" if training else "eval", errors(got, ref), got["fwd"], got["bwd"])
    _check_f32(ins, ref, got, training, ins[0].shape[1])
    # launch budgets: forward 5 in training, 1 in eval; backward 3.  (On the parent nothing launches at 33 maps and more.)
    assert got["fwd"] == (5 if training else 1) and got["bwd"] == 3
    if training:
        e = dict(rm=rel_err(base._np(got["rm"]), base._np(ref["rm"])), rv=rel_err(base._np(got["rv"]), base._np(ref["rv"])))
        print(name, e)
        assert e["rm"] <= F32 and e["rv"] <= F32
        assert not torch.equal(got["rm"].cpu(), ins[4])
    else:
        assert torch.equal(got["rm"].cpu(), ins[4]) and torch.equal(got["rv"].cpu(), ins[5])       # eval leaves them
    if name == "zero_row_wide" and training:
        want = torch.relu(ins[3][3]).expand(4)              # var = 0: a = beta, whatever the maps
        assert torch.allclose(got["out"][:, 3].cpu(), want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("name", ["r3_head", "three_radii"])
def test_bf16_maps(name, training, dev):
    ins, ref = case_ref(name, training, True)
    assert ref["guard"] >= GUARD, ref["guard"]
    got = run_hip(ins, training, dev, torch.bfloat16)
    e = errors(got, ref)
    print(name, "train" if training else "eval", e)
    assert got["out"].dtype == torch.bfloat16 and got["gm"].dtype == torch.bfloat16 and got["gw"].dtype == torch.float32
    assert got["gg"].dtype == torch.float32 and got["gb"].dtype == torch.float32
    assert e["out"] <= BF_OUT
    for k in ("gm", "gw", "gg", "gb"):
        assert e[k] <= BF_GRAD, (k, e[k])
    assert _variant() == f"cpool_wide_bwd<bf16,{'train' if training else 'eval'},n{_np16(ins[0].shape[1])}>"


@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("name", ["three_radii", "n96_chunked"])
def test_two_runs_agree_bitwise(name, training, dev):
    ins, _ = case_ref(name, training)
    a, b = run_hip(ins, training, dev), run_hip(ins, training, dev)
    assert a["fwd"] > 0 and a["bwd"] > 0
    for k in ("out", "gm", "gw", "gg", "gb", "rm", "rv"):
        assert torch.equal(a[k], b[k]), k


def test_eval_rows_do_not_depend_on_the_batch(dev):
    ins, _ = case_ref("three_radii", False)
    full = run_hip(ins, False, dev)
    part = run_hip(tuple(t[:2] if i in (0, 6) else t for i, t in enumerate(ins)), False, dev)
    assert part["fwd"] == 1
    assert torch.equal(part["out"], full["out"][:2]) and torch.equal(part["gm"], full["gm"][:2])


@pytest.mark.parametrize("training", MODES)
def test_each_gradient_switched_off_in_turn(training, dev):
    ins, _ = case_ref("n33", training)
    full = run_hip(ins, training, dev)
    keys = ("gm", "gw", "gg", "gb")
    for off in range(4):
        want = tuple(i != off for i in range(4))
        got = run_hip(ins, training, dev, want=want)
        assert got[keys[off]] is None
        for i, k in enumerate(keys):
            if i != off:
                assert torch.equal(got[k], full[k]), (keys[off], k)
        assert got["bwd"] == (2 if off == 0 else 3)       # without grad_maps its kernel is skipped
    # the maps alone: in eval no batch sum is needed — one launch
    got = run_hip(ins, training, dev, want=(True, False, False, False))
    assert torch.equal(got["gm"], full["gm"]) and got["bwd"] == (3 if training else 1)
    got = run_hip(ins, training, dev, want=(False,) * 4)
    assert torch.equal(got["out"], full["out"]) and got["bwd"] == 0


@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("name", ["n32_nonsquare", "r1_head"])
def test_the_wide_switch_runs_the_old_range_through_the_wide_form(name, training, dev, monkeypatch):
    """NFP_CPOOL_WIDE=1 (measurement): 9 to 32 maps through the wide kernels, within the same bars; 8 maps and fewer, and
    every call without the variable, report today's variant."""
    ins, ref = base.case_ref(name, training)
    assert ref["guard"] >= GUARD, ref["guard"]
    mode = "train" if training else "eval"
    got = run_hip(ins, training, dev)
    assert _variant() == f"cpool_bwd<f32,{mode}>" and got["fwd"] == (3 if training else 1)
    monkeypatch.setenv("NFP_CPOOL_WIDE", "1")
    got = run_hip(ins, training, dev)
    if ins[0].shape[1] <= 8:
        assert _variant() == f"cpool_bwd<f32,{mode}>"
        return
    print(name, mode, errors(got, ref))
    _check_f32(ins, ref, got, training, ins[0].shape[1])
    assert got["fwd"] == (5 if training else 1) and got["bwd"] == 3


def test_the_wide_switch_at_eight_maps_through_the_entry(dev):
    """The entries themselves serve every count from 1: the R = 1 head's inputs through nfp_cpool_wide_* meet the bars."""
    from neighbour_feature_pooling_amd import functional as Fn
    ins, ref = base.case_ref("r1_head", True)
    maps, w, gamma, beta, rm, rv, go = (t.to(dev) for t in ins)
    w2 = w.reshape(w.shape[0], -1).contiguous()
    rm, rv = rm.clone(), rv.clone()
    out, saved = Fn.cpool_forward_call(maps, w2, gamma, beta, rm, rv, True, base.MOM, base.EPS, "wide")
    assert _variant() == "cpool_wide_fwd<f32,train,n16>"
    gm, gw, gg, gb = Fn.cpool_backward_call(maps, w2, gamma, beta, rm, rv, saved, True, base.EPS, go, (True,) * 4, "wide")
    torch.cuda.synchronize()
    got = dict(out=out, gm=gm, gw=gw.reshape(w.shape), gg=gg, gb=gb)
    e = errors(got, ref)
    print("r1_head through the wide entries", e)
    for k in ("out", "gm", "gg", "gb"):
        assert e[k] <= F32, (k, e[k])
    assert e["gw"] <= F32_GW


def test_the_switch_takes_the_composition(dev, monkeypatch):
    from neighbour_feature_pooling_amd import nfp_compress_pool_tensors
    from neighbour_feature_pooling_amd._host import compress_pool_host
    ins, _ = case_ref("r3_head", True)
    d = [t.to(dev) for t in ins]

    def call():
        n0 = _lib().nfp_launch_count()
        out = nfp_compress_pool_tensors(d[0], *d[1:4], d[4].clone(), d[5].clone(), True, base.MOM, base.EPS)
        want = compress_pool_host(d[0], *d[1:4], d[4].clone(), d[5].clone(), True, base.MOM, base.EPS)
        return out, want, _lib().nfp_launch_count() - n0

    assert call()[2] == 5
    monkeypatch.setenv("NFP_CPOOL_TORCH", "1")
    out, want, k = call()
    assert k == 0 and torch.equal(out, want)
    monkeypatch.delenv("NFP_CPOOL_TORCH")           # the default routing: no (maps, B * P) class is routed to the wide form
    out, want, k = call()
    assert k == 0 and torch.equal(out, want)
