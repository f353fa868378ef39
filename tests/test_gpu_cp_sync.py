"""SyncBatchNorm in the fused compress tails on the MI355X (include/nfp.h nfp_cpsync_*, compress.py "SyncBatchNorm in the
two tails"), on one GPU:

  * emulated ranks — the staged call functions driven shard by shard, the records / rows joined with torch.cat (which is
    what the all-reduce of the zeroed [world, K] buffer yields), against the float64 composition on the concatenated batch:
    tests/test_gpu_cpool.py::reference64 for the pooled tail, and for the projection, which that function does not form,
    tests/test_gpu_cproj.py::reference64 (the same composition with the map kept).  The bars are those files' constants;
  * a one-rank gloo group in this process: the module-taking functions take today's path, the sync node stays inside the
    bars against it;
  * two fresh child processes on the one GPU over gloo, through nfp_compress_pool with an nn.SyncBatchNorm.

The ReLU mask: as in tests/test_gpu_cpool.py every case with a ReLU fixes a seed for which the float64 reference has
min|a| >= 1e-5 max|a| (searched on the CPU: the first seed that passes — pool_chunked, 176000 pre-activations, took 3944
tries); the guard is asserted before anything is compared.
"""
import datetime
import functools
import json
import os
import subprocess
import sys
import time

import pytest
import torch

import test_gpu_cpool as KP
import test_gpu_cproj as KJ
from conftest import ROOT, rel_err
from test_gpu_cpool import BF_GRAD, BF_OUT, EPS, F32, F32_GW, GUARD, MOM, OFFSET

pytestmark = pytest.mark.gpu

# name: (images per shard, N, D, (H, W), kind, relu, channels-last out and grad_out, bf16, seed, what it covers)
CASES = {
    "pool_r1": ((3, 1, 4), 8, 32, (7, 7), "pool", True, False, False, 0, "the R = 1 head, ragged shards"),
    "pool_empty_rank": ((2, 0, 3), 5, 160, (7, 7), "pool", True, False, False, 2, "a rank without an image; N = 5, two D tiles"),
    "pool_two_values": ((1, 1), 32, 32, (1, 1), "pool", True, False, False, 0, "global count 2: one value per channel and rank"),
    "pool_chunked": ((2, 0, 3), 8, 32, (25, 44), "pool", True, False, False, 3943, "P = 1100: two chunks per image"),
    "pool_bf16": ((3, 1, 4), 8, 32, (7, 7), "pool", True, False, True, 2, "bf16 maps"),
    "proj_relu": ((3, 1, 4), 8, 160, (7, 7), "proj", True, False, False, 3, "the insert's projection, NCHW"),
    "proj_lin_nhwc": ((2, 0, 3), 32, 32, (7, 7), "proj", False, True, False, 0, "32 maps, no ReLU, channels-last, an empty rank"),
    "proj_relu_nhwc_bf16": ((3, 1, 4), 5, 32, (7, 7), "proj", True, True, True, 1, "bf16, channels-last"),
    "proj_lin_chunked": ((3, 1, 4), 8, 32, (25, 44), "proj", False, False, False, 0, "P = 1100, no ReLU"),
    "proj_two_values": ((1, 1), 8, 160, (1, 1), "proj", True, False, False, 0, "global count 2, the map kept"),
}
OFFSET_CASE = ((3, 4), 8, 32, (7, 7), "pool", True, False, False, 0, "shard 0 near +100, shard 1 near -100, unit spread")
# The maps of the two cases with a global count of 2 have this spread, not 1.  Two values y1, y2 of a channel normalise to
# +-sqrt(var / (var + eps)), so the gradient of the BatchNorm with respect to them is (ga1 - ga2) / 2 * eps / (var + eps):
# terms of order 1 that cancel to eps / var of their size.  At unit spread (var ~ 1, eps = 1e-5) no float32 arithmetic keeps
# it: torch's own float32 conv2d -> batch_norm -> relu -> mean misses the float64 grad_maps / grad_w of these inputs by
# 3.6e-4 / 4.0e-4 of their max (pooled) and 3.5e-5 / 3.3e-5 (projection), and the staged kernels measured 6.7e-3 / 1.7e-3
# on the pooled case; out, grad_gamma, grad_beta and the running statistics held 1e-5 there.  At spread 0.01 (var ~ 1e-3)
# the cancellation costs two digits, the same torch composition holds 4e-7, and the case checks what it is here for: a
# global count of 2 with one value per channel on each rank, at the bars of every other case.
TWO_VALUE_SPREAD = 0.01


def make_inputs(case, offset=False):
    """maps [B,N,H,W], w [D,N,1,1], gamma, beta, running_mean, running_var [D], grad_out ([B,D] or [B,D,H,W]): float32 CPU
    tensors of the whole batch, B the sum of the shards."""
    shards, N, D, hw, kind, _, _, _, seed, _ = case
    B = sum(shards)
    g = torch.Generator().manual_seed(104729 * seed + 31 * B + N + D + hw[0] * hw[1])
    maps = torch.randn(B, N, *hw, generator=g)
    if B * hw[0] * hw[1] == 2:
        maps *= TWO_VALUE_SPREAD
    if offset:
        maps[:shards[0]] += 100
        maps[shards[0]:] -= 100
    w = torch.randn(D, N, 1, 1, generator=g) * 0.5
    gamma = torch.rand(D, generator=g) + 0.5
    beta = torch.randn(D, generator=g) * 0.5
    rm = torch.randn(D, generator=g) * 0.3
    rv = torch.rand(D, generator=g) + 0.5
    go = torch.randn(*((B, D) if kind == "pool" else (B, D, *hw)), generator=g)
    return maps, w, gamma, beta, rm, rv, go


def reference(case, ins):
    _, _, _, _, kind, relu, _, bf16, _, _ = case
    dtype = torch.bfloat16 if bf16 else torch.float32
    return KP.reference64(ins, True, dtype) if kind == "pool" else KJ.reference64(ins, True, relu, dtype)


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """(case, inputs, float64 reference on the concatenated batch) — computed once, shared, never modified."""
    case = OFFSET_CASE if name == "offset" else CASES[name]
    ins = make_inputs(case, offset=name == "offset")
    return case, ins, reference(case, ins)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from neighbour_feature_pooling_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


def _lib():
    from neighbour_feature_pooling_amd import _abi
    return _abi.load()


def _count():
    return _lib().nfp_launch_count()


def _np(t):
    return t.detach().double().cpu().numpy()


def run_shards(case, ins, dev):
    """The step of `case` by emulated ranks: dict(out, gm: the shards' results concatenated; gw, gg, gb: summed over the
    shards; rm, rv, saved: one per shard; launches: per shard (moments, forward, reduce, maps))."""
    from neighbour_feature_pooling_amd import functional as Fn
    shards, N, D, hw, kind, relu, nhwc, bf16, _, _ = case
    maps, w, gamma, beta, rm, rv, go = ins
    dt = torch.bfloat16 if bf16 else torch.float32
    w2, gamma, beta = w.reshape(D, N).to(dev), gamma.to(dev), beta.to(dev)
    ms = [m.to(dev).to(dt).contiguous() for m in torch.split(maps, shards)]
    gos = [g.to(dev).to(dt if kind == "proj" else torch.float32) for g in torch.split(go, shards)]
    if nhwc:
        gos = [g.contiguous(memory_format=torch.channels_last) for g in gos]
    launches = [[] for _ in shards]

    def counted(r, f, *a, **kw):
        n0 = _count()
        res = f(*a, **kw)
        launches[r].append(_count() - n0)
        return res

    records = torch.cat([counted(r, Fn.cp_sync_moments_call, m)[None] for r, m in enumerate(ms)])
    assert records.dtype == torch.float64 and records.shape == (len(shards), 1 + N + N * N)
    outs, saved, rms, rvs = [], [], [], []
    for r, m in enumerate(ms):
        rms.append(rm.clone().to(dev)), rvs.append(rv.clone().to(dev))
        out, sv = counted(r, Fn.cp_sync_forward_call, kind, m, w2, gamma, beta, rms[r], rvs[r], MOM, EPS, records, relu, nhwc)
        outs.append(out), saved.append(sv)
    part = [counted(r, Fn.cp_sync_reduce_call, kind, m, w2, gamma, beta, saved[r], EPS, gos[r], (True, True, True), relu)
            for r, m in enumerate(ms)]
    rows = torch.cat([p[3][None] for p in part])
    assert rows.dtype == torch.float32 and rows.shape == (len(shards), N + N * N)
    gms = [counted(r, Fn.cp_sync_maps_call, kind, m, w2, gamma, beta, saved[r], EPS, gos[r], rows, relu) for r, m in enumerate(ms)]
    torch.cuda.synchronize()
    if kind == "proj":
        for o in outs:
            assert o.dtype == dt and o.is_contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format)
    return dict(out=torch.cat(outs), gm=torch.cat(gms), gw=sum(p[0] for p in part).reshape(w.shape), gg=sum(p[1] for p in part),
                gb=sum(p[2] for p in part), rm=rms, rv=rvs, saved=saved, launches=launches, records=records, rows=rows)


def errors(got, ref):
    e = {k: rel_err(_np(got[k]).reshape(-1), _np(ref[k]).reshape(-1)) for k in ("out", "gm", "gw", "gg", "gb")}
    e["rm"] = rel_err(_np(got["rm"][0]), _np(ref["rm"]))
    e["rv"] = rel_err(_np(got["rv"][0]), _np(ref["rv"]))
    e["guard"] = ref["guard"]
    return e


def assert_shards_hold_the_same_statistics(got):
    for k in ("saved", "rm", "rv"):
        for t in got[k][1:]:
            assert torch.equal(t, got[k][0]), k


@pytest.mark.parametrize("name", list(CASES))
def test_emulated_ranks_match_the_float64_composition_on_the_whole_batch(name, dev):
    case, ins, ref = case_ref(name)
    shards, N, D, hw, kind, relu, nhwc, bf16, _, _ = case
    if relu:
        assert ref["guard"] >= GUARD, ref["guard"]
    got = run_shards(case, ins, dev)
    e = errors(got, ref)
    print(name, e, got["launches"])
    assert got["gm"].shape == ins[0].shape and got["out"].shape == ref["out"].shape
    bars = dict(out=BF_OUT, gm=BF_GRAD, gw=BF_GRAD, gg=BF_GRAD, gb=BF_GRAD) if bf16 else \
        dict(out=F32, gm=F32, gw=F32_GW, gg=F32, gb=F32)
    for k, bar in bars.items():
        assert e[k] <= bar, (k, e[k])
    assert e["rm"] <= F32 and e["rv"] <= F32, (e["rm"], e["rv"])
    assert_shards_hold_the_same_statistics(got)
    # launches per stage: moments 2, forward 2, reduce 3, maps 1; an empty rank writes its zero record, joins the
    # statistics and writes its zero row: 1, 1, 1, 0
    for b, n in zip(shards, got["launches"]):
        assert n == ([2, 2, 3, 1] if b else [1, 1, 1, 0]), (b, n)
    for r, b in enumerate(shards):
        if b == 0:
            assert not got["records"][r].any() and not got["rows"][r].any()
    variant = _lib().nfp_last_variant().decode()
    assert variant.startswith("cpsync_bwd_maps<" + kind) and ("nhwc" in variant) == nhwc, variant


def test_shards_whose_means_differ_widely(dev):
    """Shard 0 near +100, shard 1 near -100, unit spread: the between-rank term n_r d_r d_r' carries the variance (10^4
    against 1 within).  Held to the bar of tests/test_gpu_cpool.py::test_offset_maps."""
    case, ins, ref = case_ref("offset")
    assert ref["guard"] >= GUARD, ref["guard"]
    got = run_shards(case, ins, dev)
    e = errors(got, ref)
    print("offset", e)
    for k in ("out", "gm", "gw", "gg", "gb", "rm", "rv"):
        assert e[k] <= OFFSET, (k, e[k])
    assert_shards_hold_the_same_statistics(got)


@pytest.mark.parametrize("name", ["pool_chunked", "proj_lin_nhwc"])
def test_two_runs_agree_bitwise(name, dev):
    case, ins, _ = case_ref(name)
    a, b = run_shards(case, ins, dev), run_shards(case, ins, dev)
    for k in ("out", "gm", "gw", "gg", "gb", "records", "rows"):
        assert torch.equal(a[k], b[k]), k
    for k in ("saved", "rm", "rv"):
        assert torch.equal(a[k][0], b[k][0]), k


# ---- a one-rank gloo group in this process ------------------------------------------------------------------------------
@pytest.fixture()
def one_rank_group():
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1, timeout=datetime.timedelta(seconds=30))
    try:
        yield dist.group.WORLD
    finally:
        dist.destroy_process_group()


def _bn_like(cls, ins, dev):
    bn = cls(ins[1].shape[0], eps=EPS, momentum=MOM).to(dev)
    with torch.no_grad():
        bn.weight.copy_(ins[2]), bn.bias.copy_(ins[3]), bn.running_mean.copy_(ins[4]), bn.running_var.copy_(ins[5])
    return bn


def _module_step(fn, maps, w, bn, go, **kw):
    maps, w = maps.clone().requires_grad_(True), w.clone().requires_grad_(True)
    n0 = _count()
    out = fn(maps, w, bn, **kw)
    n1 = _count()
    grads = torch.autograd.grad(out, (maps, w, bn.weight, bn.bias), go)
    torch.cuda.synchronize()
    return dict(out=out.detach(), gm=grads[0], gw=grads[1], gg=grads[2], gb=grads[3], rm=bn.running_mean.clone(),
                rv=bn.running_var.clone(), fwd=n1 - n0, bwd=_count() - n1, steps=int(bn.num_batches_tracked))


@pytest.mark.parametrize("kind", ["pool", "proj"])
def test_one_rank_group_takes_todays_path(kind, dev, one_rank_group, monkeypatch):
    from neighbour_feature_pooling_amd import compress, nfp_compress_map, nfp_compress_pool
    from neighbour_feature_pooling_amd import functional as Fn
    monkeypatch.setenv("NFP_CPROJ_TORCH", "0")
    case, ins, _ = case_ref("pool_r1" if kind == "pool" else "proj_relu")
    d = [t.to(dev) for t in ins]
    fn = nfp_compress_pool if kind == "pool" else nfp_compress_map
    plain = _module_step(fn, d[0], d[1], _bn_like(torch.nn.BatchNorm2d, ins, dev), d[6])
    sbn = _bn_like(torch.nn.SyncBatchNorm, ins, dev)
    assert Fn.cp_sync_group(sbn) is None
    sync = _module_step(fn, d[0], d[1], sbn, d[6])
    assert sync["fwd"] == plain["fwd"] == 3 and sync["bwd"] == plain["bwd"] == 3 and sync["steps"] == 1
    for k in ("out", "gm", "gw", "gg", "gb", "rm", "rv"):
        assert torch.equal(sync[k], plain[k]), k
    # the sync node itself, handed the group: the staged kernels, one rank's records
    D, N = ins[1].shape[:2]
    t = [d[0].clone().requires_grad_(True), d[1].reshape(D, N).clone().requires_grad_(True),
         d[2].clone().requires_grad_(True), d[3].clone().requires_grad_(True)]
    rm, rv = d[4].clone(), d[5].clone()
    n0 = _count()
    out = compress._CpSyncHip.apply(*t, (rm, rv), MOM, EPS, True, True, kind, False, one_rank_group)
    n1 = _count()
    grads = torch.autograd.grad(out, t, d[6])
    torch.cuda.synchronize()
    n2 = _count()
    print(kind, "sync node launches", n1 - n0, n2 - n1)
    assert (n1 - n0, n2 - n1) == (4, 4)
    got = dict(out=out.detach(), gm=grads[0], gw=grads[1].reshape(ins[1].shape), gg=grads[2], gb=grads[3], rm=rm, rv=rv)
    e = {k: rel_err(_np(got[k]).reshape(-1), _np(plain[k]).reshape(-1)) for k in got}
    print(kind, e)
    for k, bar in dict(out=F32, gm=F32, gw=F32_GW, gg=F32, gb=F32, rm=F32, rv=F32).items():
        assert e[k] <= bar, (k, e[k])


# ---- two fresh child processes on the one GPU, over gloo ---------------------------------------------------------------
CHILD_SHARDS = (3, 2)
CHILD_CASE = (CHILD_SHARDS, 8, 32, (7, 7), "pool", True, False, False, 0, "two processes")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).tolist()


def child(rank, world, store_path, out_path):
    """One rank: its shard through nfp_compress_pool under an nn.SyncBatchNorm, against the float64 reference on the whole
    batch; then the same call under a plain BatchNorm2d.  Writes its verdict and running statistics as JSON."""
    import torch.distributed as dist
    from neighbour_feature_pooling_amd import _abi, nfp_compress_pool
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", store=dist.FileStore(store_path, world), rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=30))
    try:
        ins = make_inputs(CHILD_CASE)
        ref = reference(CHILD_CASE, ins)
        lo = sum(CHILD_SHARDS[:rank])
        hi = lo + CHILD_SHARDS[rank]
        d = [t.to(dev) for t in ins]
        res = {}
        for name, cls in (("sync", torch.nn.SyncBatchNorm), ("plain", torch.nn.BatchNorm2d)):
            bn = _bn_like(cls, ins, dev)
            maps, w = d[0][lo:hi].clone().requires_grad_(True), d[1].clone().requires_grad_(True)
            n0 = _abi.load().nfp_launch_count()
            out = nfp_compress_pool(maps, w, bn)
            n1 = _abi.load().nfp_launch_count()
            gm, gw, gg, gb = torch.autograd.grad(out, (maps, w, bn.weight, bn.bias), d[6][lo:hi])
            n2 = _abi.load().nfp_launch_count()
            variant = _abi.load().nfp_last_variant().decode()
            for g in (gw, gg, gb):
                dist.all_reduce(g)
            e = dict(out=rel_err(_np(out), _np(ref["out"][lo:hi])), gm=rel_err(_np(gm), _np(ref["gm"][lo:hi])),
                     gw=rel_err(_np(gw), _np(ref["gw"])), gg=rel_err(_np(gg), _np(ref["gg"])), gb=rel_err(_np(gb), _np(ref["gb"])),
                     rm=rel_err(_np(bn.running_mean), _np(ref["rm"])), rv=rel_err(_np(bn.running_var), _np(ref["rv"])))
            bars = dict(out=F32, gm=F32, gw=F32_GW, gg=F32, gb=F32, rm=F32, rv=F32)
            res[name] = dict(errors=e, passed=all(e[k] <= bars[k] for k in bars), launches=[n1 - n0, n2 - n1], variant=variant,
                             steps=int(bn.num_batches_tracked), rm=_bits(bn.running_mean), rv=_bits(bn.running_var))
        res["guard"] = ref["guard"]
        with open(out_path, "w") as f:
            json.dump(res, f)
    finally:
        dist.destroy_process_group()


def test_two_processes_share_one_batch_norm(tmp_path):
    world = len(CHILD_SHARDS)
    store = str(tmp_path / "store")
    outs = [str(tmp_path / f"rank{r}.json") for r in range(world)]
    flags = ["-s"] if sys.flags.no_user_site else []
    env = {k: v for k, v in os.environ.items() if k != "NFP_CPOOL_TORCH"}
    procs = [subprocess.Popen([sys.executable, *flags, os.path.abspath(__file__), "--child", str(r), str(world), store, outs[r]],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    deadline = time.monotonic() + 120
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=max(1.0, deadline - time.monotonic()))[0])
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
        pytest.fail("the two ranks did not finish within 120 s")
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-4000:]
    res = [json.load(open(o)) for o in outs]
    print([r["sync"]["errors"] for r in res], [r["sync"]["launches"] for r in res])
    for r in res:
        assert r["guard"] >= GUARD
        assert r["sync"]["passed"], r["sync"]["errors"]
        assert r["sync"]["launches"] == [4, 4] and r["sync"]["variant"].startswith("cpsync_bwd_maps<pool"), r["sync"]
        assert r["plain"]["launches"] == [3, 3] and r["plain"]["variant"] == "cpool_bwd<f32,train>", r["plain"]
        assert r["sync"]["steps"] == 1 and r["plain"]["steps"] == 1
    assert res[0]["sync"]["rm"] == res[1]["sync"]["rm"] and res[0]["sync"]["rv"] == res[1]["sync"]["rv"]
    # the plain BatchNorm2d in the same children kept rank-local statistics: they differ, and miss the whole batch's
    assert res[0]["plain"]["rm"] != res[1]["plain"]["rm"] and res[0]["plain"]["rv"] != res[1]["plain"]["rv"]
    assert not res[0]["plain"]["passed"] and not res[1]["plain"]["passed"]


if __name__ == "__main__" and len(sys.argv) == 6 and sys.argv[1] == "--child":
    child(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5])
