"""The heads' compress-BN-ReLU-GAP tail on the MI355X (csrc/nfp_cpool.hip, include/nfp.h nfp_cpool_*) against the float64
torch composition (conv2d, batch_norm, relu, mean) of the same inputs: the output and all four gradients, training and eval.

Bars, of each tensor's max magnitude: 1e-5 for float32 — grad_w, a difference of two larger sums, 5e-5; 1e-2 (out) and
2e-2 (gradients) for bf16 maps, against the reference on the bf16-rounded maps; 1e-4 on every tensor for maps of mean 10
and spread 0.1 (second moments taken uncentred in float32 miss that by a factor of ten and more).

The ReLU mask: a pre-activation whose sign differs between float32 and float64 changes a gradient by a whole term, so
every case fixes a seed for which the float64 reference has min|a| >= 1e-5 max|a| (float32 error of a: about 2e-7 of
max|a|), in training and in eval; the guard is asserted on the reference before anything is compared, and no element is
ever excluded.  The seeds were searched on the CPU: the first that passes in both modes (and, for the two bf16 cases, on
the bf16-rounded maps too) — the chunked case, 51200 pre-activations, took 139 tries."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

F32, F32_GW, BF_OUT, BF_GRAD, OFFSET = 1e-5, 5e-5, 1e-2, 2e-2, 1e-4
GUARD = 1e-5
EPS, MOM = 1e-5, 0.1

# name: (maps shape, D, seed, what it covers)
CASES = {
    "r1_head": ((4, 8, 7, 7), 32, 2, "the R = 1 head"),
    "n32_nonsquare": ((3, 32, 5, 7), 48, 10, "32 maps, non-square, D not a wave multiple"),
    "chunked": ((2, 32, 40, 40), 16, 138, "an image larger than the LDS budget, walked in chunks"),
    "one_pixel": ((5, 24, 1, 1), 16, 0, "P = 1"),
    "d_tiles": ((2, 8, 3, 3), 520, 4, "several D tiles and a ragged last one"),
    "one_image": ((1, 8, 7, 7), 32, 0, "B = 1"),
    "zero_row": ((4, 8, 7, 7), 32, 2, "an all-zero weight row: var = 0, a = beta"),
    "offset": ((4, 8, 7, 7), 32, 0, "maps = 10 + 0.1 randn"),
    "n12": ((3, 12, 6, 5), 70, 1, "12 maps: the NP = 16 instantiations"),
}


def make_inputs(name, seed=None):
    """maps [B,N,H,W], w [D,N,1,1], gamma, beta, running_mean, running_var [D], grad_out [B,D]: float32 CPU tensors."""
    shape, D, dflt, _ = CASES[name]
    seed = dflt if seed is None else seed
    g = torch.Generator().manual_seed(7919 * seed + sum(shape) + D)
    B, N = shape[:2]
    maps = torch.randn(*shape, generator=g)
    if name == "offset":
        maps = 10 + 0.1 * maps
    w = torch.randn(D, N, 1, 1, generator=g) * 0.5
    if name == "zero_row":
        w[3] = 0
    gamma = torch.rand(D, generator=g) + 0.5
    beta = torch.randn(D, generator=g) * 0.5
    rm = torch.randn(D, generator=g) * 0.3
    if name == "offset":
        rm = rm + 10 * w.reshape(D, N).sum(1)      # (near the conv output's mean, as a trained BatchNorm's would be)
    rv = torch.rand(D, generator=g) + 0.5
    go = torch.randn(B, D, generator=g)
    return maps, w, gamma, beta, rm, rv, go


def reference64(ins, training, maps_dtype=torch.float32):
    """dict(out, gm, gw, gg, gb, rm, rv, guard) of the float64 composition on `ins` (the maps rounded to maps_dtype first)."""
    maps, w, gamma, beta, rm, rv, go = ins
    maps = maps.to(maps_dtype)
    m, w_, ga, be = (t.double().requires_grad_(True) for t in (maps, w, gamma, beta))
    rm, rv = rm.double().clone(), rv.double().clone()
    a = F.batch_norm(F.conv2d(m, w_), rm, rv, ga, be, training, MOM, EPS)
    out = F.relu(a).mean((2, 3))
    gm, gw, gg, gb = torch.autograd.grad(out, (m, w_, ga, be), go.double())
    aa = a.detach().abs()
    return dict(out=out.detach(), gm=gm, gw=gw, gg=gg, gb=gb, rm=rm, rv=rv, guard=float(aa.min() / aa.max()))


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
    """NFP_CPOOL_TORCH=0: the kernels are tested for every maps count they serve, also the ones (more than 8 maps) the
    default routing hands to the composition because they measured slower."""
    monkeypatch.setenv("NFP_CPOOL_TORCH", "0")


def _lib():
    from neighbour_feature_pooling_amd import _abi
    return _abi.load()


def _count():
    return _lib().nfp_launch_count()


def run_hip(ins, training, dev, dtype=torch.float32, want=(True, True, True, True)):
    """dict(out, gm, gw, gg, gb, rm, rv, fwd, bwd) of nfp_compress_pool_tensors on the device: None for a gradient not asked
    for; fwd / bwd the launch-counter deltas."""
    from neighbour_feature_pooling_amd import nfp_compress_pool_tensors
    maps, w, gamma, beta, rm, rv, go = ins
    t = [x.to(dev) for x in (maps.to(dtype), w, gamma, beta)]
    t = [x.requires_grad_(r) for x, r in zip(t, want)]
    rm, rv = rm.clone().to(dev), rv.clone().to(dev)
    n0 = _count()
    out = nfp_compress_pool_tensors(t[0], t[1], t[2], t[3], rm, rv, training, MOM, EPS)
    n1 = _count()
    asked = [x for x in t if x.requires_grad]
    grads = iter(torch.autograd.grad(out, asked, go.to(dev).to(out.dtype)) if asked else ())
    torch.cuda.synchronize()
    n2 = _count()
    res = dict(zip(("gm", "gw", "gg", "gb"), (next(grads) if r else None for r in want)))
    res.update(out=out.detach(), rm=rm, rv=rv, fwd=n1 - n0, bwd=n2 - n1)
    return res


def _np(t):
    return t.detach().double().cpu().numpy()


def errors(got, ref):
    e = {k: rel_err(_np(got[k]).reshape(-1), _np(ref[k]).reshape(-1)) for k in ("out", "gm", "gw", "gg", "gb")}
    e["guard"] = ref["guard"]
    return e


MODES = [pytest.param(True, id="train"), pytest.param(False, id="eval")]


@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("name", [n for n in CASES if n != "offset"])
def test_float32_matches_the_float64_composition(name, training, dev):
    ins, ref = case_ref(name, training)
    assert ref["guard"] >= GUARD, ref["guard"]
    got = run_hip(ins, training, dev)
    e = errors(got, ref)
    print(name, "train" if training else "eval", e, got["fwd"], got["bwd"])
    assert got["out"].dtype == torch.float32 and got["gm"].shape == ins[0].shape and got["gw"].shape == ins[1].shape
    for k in ("out", "gm", "gg", "gb"):
        assert e[k] <= F32, (k, e[k])
    assert e["gw"] <= F32_GW, e["gw"]
    # launch budgets: forward 3 in training, 2 in eval; backward 3
    assert 1 <= got["fwd"] <= (3 if training else 2) and 1 <= got["bwd"] <= 3
    assert _lib().nfp_last_variant().decode() == f"cpool_bwd<f32,{'train' if training else 'eval'}>"
    if name == "zero_row" and training:
        want = torch.relu(ins[3][3]).expand(4)              # var = 0: a = beta, whatever the maps (eval: beta - s_d rm_d)
        assert torch.allclose(got["out"][:, 3].cpu(), want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("name", ["r1_head", "n32_nonsquare"])
def test_bf16_maps(name, training, dev):
    ins, ref = case_ref(name, training, True)
    assert ref["guard"] >= GUARD, ref["guard"]
    got = run_hip(ins, training, dev, torch.bfloat16)
    e = errors(got, ref)
    print(name, "train" if training else "eval", e)
    assert got["out"].dtype == torch.bfloat16 and got["gm"].dtype == torch.bfloat16 and got["gw"].dtype == torch.float32
    assert e["out"] <= BF_OUT
    for k in ("gm", "gw", "gg", "gb"):
        assert e[k] <= BF_GRAD, (k, e[k])
    assert _lib().nfp_last_variant().decode() == f"cpool_bwd<bf16,{'train' if training else 'eval'}>"


@pytest.mark.parametrize("training", MODES)
def test_offset_maps(training, dev):
    """Maps of mean 10 and spread 0.1: the second moments must be taken centred.  (Uncentred in float32: 1e-3 forward,
    4e-3 to 4e-1 backward.)"""
    ins, ref = case_ref("offset", training)
    assert ref["guard"] >= GUARD, ref["guard"]
    got = run_hip(ins, training, dev)
    e = errors(got, ref)
    print("offset", "train" if training else "eval", e)
    for k in ("out", "gm", "gw", "gg", "gb"):
        assert e[k] <= OFFSET, (k, e[k])


def test_running_statistics_and_num_batches_tracked(dev):
    from neighbour_feature_pooling_amd import nfp_compress_pool
    for name in ("r1_head", "chunked", "offset"):
        ins, ref = case_ref(name, True)
        got = run_hip(ins, True, dev)
        e = dict(rm=rel_err(_np(got["rm"]), _np(ref["rm"])), rv=rel_err(_np(got["rv"]), _np(ref["rv"])))
        print(name, e)
        assert e["rm"] <= F32 and e["rv"] <= F32
        assert not torch.equal(got["rm"].cpu(), ins[4])
        ins, ref = case_ref(name, False)
        got = run_hip(ins, False, dev)
        assert torch.equal(got["rm"].cpu(), ins[4]) and torch.equal(got["rv"].cpu(), ins[5])       # eval leaves them
    # the module form: bn's own buffers, its counter bumped on the Python side
    ins, ref = case_ref("r1_head", True)
    bn = torch.nn.BatchNorm2d(32, eps=EPS, momentum=MOM).to(dev)
    with torch.no_grad():
        bn.weight.copy_(ins[2]), bn.bias.copy_(ins[3]), bn.running_mean.copy_(ins[4]), bn.running_var.copy_(ins[5])
    n0 = _count()
    out = nfp_compress_pool(ins[0].to(dev), ins[1].to(dev), bn)
    assert _count() - n0 == 3
    assert int(bn.num_batches_tracked) == 1
    assert rel_err(_np(out), _np(ref["out"])) <= F32 and rel_err(_np(bn.running_var), _np(ref["rv"])) <= F32
    bn.eval()
    n0 = _count()
    out = nfp_compress_pool(ins[0].to(dev), ins[1].to(dev), bn)
    assert _count() - n0 == 1 and int(bn.num_batches_tracked) == 1
    # track_running_stats=False: batch statistics in both modes, nothing to update
    bn2 = torch.nn.BatchNorm2d(32, eps=EPS, momentum=MOM, track_running_stats=False).to(dev).eval()
    with torch.no_grad():
        bn2.weight.copy_(ins[2]), bn2.bias.copy_(ins[3])
    n0 = _count()
    out = nfp_compress_pool(ins[0].to(dev), ins[1].to(dev), bn2)
    assert _count() - n0 == 3 and rel_err(_np(out), _np(ref["out"])) <= F32


@pytest.mark.parametrize("training", MODES)
def test_each_gradient_switched_off_in_turn(training, dev):
    ins, _ = case_ref("n32_nonsquare", training)
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
    # nothing asked for: no saved state, no backward
    got = run_hip(ins, training, dev, want=(False,) * 4)
    assert torch.equal(got["out"], full["out"]) and got["bwd"] == 0


@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("name", ["r1_head", "chunked"])
def test_two_runs_agree_bitwise(name, training, dev):
    ins, _ = case_ref(name, training)
    a, b = run_hip(ins, training, dev), run_hip(ins, training, dev)
    for k in ("out", "gm", "gw", "gg", "gb", "rm", "rv"):
        assert torch.equal(a[k], b[k]), k


def test_eval_rows_do_not_depend_on_the_batch(dev):
    ins, _ = case_ref("n32_nonsquare", False)
    full = run_hip(ins, False, dev)
    part = run_hip(tuple(t[:2] if i in (0, 6) else t for i, t in enumerate(ins)), False, dev)
    assert torch.equal(part["out"], full["out"][:2]) and torch.equal(part["gm"], full["gm"][:2])


def test_empty_batch(dev):
    from neighbour_feature_pooling_amd import nfp_compress_pool_tensors
    L = _lib()
    p = torch.zeros(2048, device=dev).data_ptr()
    n0 = _count()
    assert L.nfp_cpool_forward(0, 8, 49, 32, 0, 1, None, p, p, p, p, p, MOM, EPS, None, p, 112, None, 0, None) == 0
    assert L.nfp_cpool_backward(0, 8, 49, 32, 0, 1, None, p, p, p, None, None, EPS, p, 112, None, None, p, p, p, None, 0, None) == 0
    assert _count() == n0
    ins = make_inputs("r1_head")
    out = nfp_compress_pool_tensors(ins[0][:0].to(dev), *(t.to(dev) for t in ins[1:6]), False)
    assert out.shape == (0, 32) and _count() == n0


def test_the_switch_and_the_unserved_calls_take_the_composition(dev, monkeypatch):
    from neighbour_feature_pooling_amd import nfp_compress_pool_tensors
    from neighbour_feature_pooling_amd._host import compress_pool_host
    ins, ref = case_ref("r1_head", True)
    d = [t.to(dev) for t in ins]

    def call(maps, params=d[1:4], dtype=None):
        cast = (lambda t: t) if dtype is None else (lambda t: t.to(dtype))
        args = [cast(t) for t in params] + [cast(d[4].clone()), cast(d[5].clone())]
        n0 = _count()
        out = nfp_compress_pool_tensors(maps, *args, True, MOM, EPS)
        want = compress_pool_host(maps, *[cast(t) for t in params], cast(d[4].clone()), cast(d[5].clone()), True, MOM, EPS)
        return out, want, _count() - n0

    out, want, k = call(d[0])
    assert k == 3 and rel_err(_np(out), _np(want)) <= 1e-4
    monkeypatch.setenv("NFP_CPOOL_TORCH", "1")          # the A/B switch, read at call time
    out, want, k = call(d[0])
    assert k == 0 and torch.equal(out, want)
    monkeypatch.delenv("NFP_CPOOL_TORCH")
    assert call(d[0])[2] == 3
    # the default routing: 8 maps on the HIP tail, more on the composition; "0" forces the HIP tail
    ins32 = [t.to(dev) for t in make_inputs("n32_nonsquare")]
    args32 = lambda: ins32[1:4] + [ins32[4].clone(), ins32[5].clone(), True, MOM, EPS]      # noqa: E731
    n0 = _count()
    nfp_compress_pool_tensors(ins32[0], *args32())
    assert _count() == n0
    monkeypatch.setenv("NFP_CPOOL_TORCH", "0")
    nfp_compress_pool_tensors(ins32[0], *args32())
    assert _count() == n0 + 3
    strided = torch.randn(4, 8, 7, 14, device=dev)[..., ::2]
    for maps, dtype in ((strided, None), (d[0].half(), torch.float16), (d[0].double(), torch.float64)):
        out, want, k = call(maps, dtype=dtype)
        assert k == 0 and torch.equal(out, want) and out.dtype == maps.dtype
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out, want, k = call(d[0])
    assert k == 0 and torch.equal(out, want)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        call(d[0][:1, :, :1, :1].contiguous())
