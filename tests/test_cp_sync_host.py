"""SyncBatchNorm in the fused compress tails, on the host: the nfp_cpsync_* declarations, their length queries and their
refusals (all before any HIP call), the group rule and the route predicate of compress.py, and a converted head without
a process group.  No GPU needed."""
import copy
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from neighbour_feature_pooling_amd import NFPHead, _abi
from neighbour_feature_pooling_amd import compress
from neighbour_feature_pooling_amd import functional as Fn

NEW_EXPORTS = {"nfp_cpsync_record_doubles", "nfp_cpsync_kq_floats", "nfp_cpsync_saved_floats", "nfp_cpsync_moments",
               "nfp_cpsync_forward", "nfp_cpsync_reduce", "nfp_cpsync_maps"}
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def L():
    from neighbour_feature_pooling_amd.build import build_hip
    build_hip()
    return _abi.load()


def test_new_exports_are_declared_listed_and_present(L):
    src = open(os.path.join(ROOT, "include", "nfp.h")).read()
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(nfp_[a-z_]+)\s*\(", body))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(_abi.EXPORTS)
    for n in NEW_EXPORTS:
        assert hasattr(L, n), n
    assert int(re.search(r"#define NFP_ABI_VERSION (\d+)", src).group(1)) == _abi.ABI_VERSION == L.nfp_abi_version() == 7
    assert re.search(r"enum nfp_cp_kind \{ NFP_CP_POOL = 0, NFP_CP_PROJ = 1 \}", src) and (_abi.CP_POOL, _abi.CP_PROJ) == (0, 1)


@pytest.mark.parametrize("N,D", [(1, 1), (5, 160), (8, 32), (32, 512)])
def test_length_queries(L, N, D):
    assert L.nfp_cpsync_record_doubles(N) == 1 + N + N * N
    assert L.nfp_cpsync_kq_floats(N) == N + N * N
    assert L.nfp_cpsync_saved_floats(N, D) == 2 * N + 2 * N * N + D + 1 == L.nfp_cpool_saved_floats(N, D) + 1 + N * N


def test_refusals_launch_nothing(L):
    p = 0x1000      # (never dereferenced: every call below is refused, or returns, before any HIP call)
    B, N, P, D, W = 4, 8, 49, 32, 3
    nrec, nkq, nsv = 1 + N + N * N, N + N * N, 2 * N + 2 * N * N + D + 1
    big = 1 << 40
    n0 = L.nfp_launch_count()

    def moments(B=B, N=N, maps=p, rec=p, nr=nrec, scr=p, ns=big):
        return L.nfp_cpsync_moments(B, N, P, 0, maps, rec, nr, scr, ns, None)

    def forward(kind=0, B=B, N=N, P=P, maps=p, w=p, recs=p, world=W, nr=W * nrec, count=0, out=p, saved=p, ns=nsv, rm=p, rv=p,
                layout=0, eps=1e-5):
        return L.nfp_cpsync_forward(kind, B, N, P, D, 0, 1, maps, w, p, p, rm, rv, 0.1, eps, recs, world, nr, count, out, saved,
                                    ns, None, layout)

    def reduce(kind=0, N=N, go=p, saved=p, ns=nsv, row=p, nk=nkq, scr=p, nscr=big):
        return L.nfp_cpsync_reduce(kind, B, N, P, D, 0, 1, p, p, p, p, 1e-5, saved, ns, go, p, p, p, row, nk, scr, nscr, None, 0)

    def maps(kind=0, N=N, go=p, saved=p, ns=nsv, rows=p, world=W, nk=W * nkq, gm=p):
        return L.nfp_cpsync_maps(kind, B, N, P, D, 0, 1, p, p, p, p, 1e-5, saved, ns, go, rows, world, nk, gm, None, 0)

    # a null pointer
    for rc in (moments(maps=None), moments(rec=None), moments(scr=None), forward(maps=None), forward(w=None), forward(recs=None),
               forward(out=None), forward(saved=None), forward(rv=None), reduce(go=None), reduce(saved=None), reduce(row=None),
               reduce(scr=None), maps(go=None), maps(saved=None), maps(rows=None), maps(gm=None)):
        assert rc == INVALID and L.nfp_last_error()
    # a short buffer
    need = L.nfp_cpool_scratch_floats(B, N, P, 1, 0)
    for rc in (moments(nr=nrec - 1), moments(ns=need - 1), forward(nr=W * nrec - 1), forward(ns=nsv - 1), reduce(ns=nsv - 1),
               reduce(nk=nkq - 1), reduce(nscr=L.nfp_cpool_scratch_floats(B, N, P, D, 1) - 1),
               reduce(kind=1, nscr=L.nfp_cproj_scratch_floats(B, N, P, D, 1) - 1), maps(nk=W * nkq - 1), maps(ns=nsv - 1)):
        assert rc == INVALID
    assert b"nfp_cpsync_saved_floats" in L.nfp_last_error()
    # records off an 8-byte boundary, an unknown kind or layout, a negative eps or count
    for rc in (moments(rec=p + 4), forward(recs=p + 4), forward(kind=2), reduce(kind=-1), maps(kind=7), forward(kind=1, layout=2),
               forward(eps=-1.0), forward(count=-1)):
        assert rc == INVALID
    # N = 33
    for rc in (moments(N=33, nr=big), forward(N=33, nr=big, ns=big), reduce(N=33, ns=big, nk=big), maps(N=33, ns=big, nk=big)):
        assert rc == UNSUPPORTED
    assert b"N = 33" in L.nfp_last_error()
    # world = 0
    assert forward(world=0) == INVALID and maps(world=0) == INVALID and forward(world=-1) == INVALID
    assert b"world" in L.nfp_last_error()
    # a global count of 1 — one rank, one value per channel — or one below this rank's own
    assert forward(B=1, P=1, world=1, count=1) == UNSUPPORTED
    assert b"global_count = 1" in L.nfp_last_error()
    assert forward(count=B * P - 1) == UNSUPPORTED
    # an empty rank with nothing to write: no launch either
    assert L.nfp_cpsync_maps(0, 0, N, P, D, 0, 1, None, p, p, p, 1e-5, p, nsv, None, p, W, W * nkq, None, None, 0) == 0
    assert L.nfp_launch_count() == n0


class _FakeDist:
    """What cp_sync_group asks torch.distributed."""

    def __init__(self, available=True, initialised=True, sizes=None):
        self.available, self.initialised, self.sizes = available, initialised, sizes or {}
        self.group = types.SimpleNamespace(WORLD="world")

    def is_available(self):
        return self.available

    def is_initialized(self):
        return self.initialised

    def get_world_size(self, group=None):
        return self.sizes["world" if group is None else group]


def test_the_group_rule(monkeypatch):
    plain, sync = torch.nn.BatchNorm2d(4), torch.nn.SyncBatchNorm(4)
    own = torch.nn.SyncBatchNorm(4, process_group="mine")

    def group(bn, training=None, **kw):
        monkeypatch.setattr(torch, "distributed", _FakeDist(**kw))
        return Fn.cp_sync_group(bn, training)

    two = dict(sizes={"world": 2, "mine": 2})
    assert group(plain, **two) is None                                   # a plain BatchNorm2d
    assert group(sync, **two) == "world"                                 # world 2: the group
    assert group(sync.eval(), **two) is None                             # eval
    assert group(sync, True, **two) == "world" and group(sync.train(), False, **two) is None      # the call's mode decides
    assert group(sync, initialised=False, **two) is None                 # not initialised
    assert group(sync, available=False, **two) is None
    assert group(sync, sizes={"world": 1}) is None                       # a one-rank group
    assert group(own, sizes={"world": 1, "mine": 2}) == "mine"           # bn.process_group wins over WORLD
    assert group(own, sizes={"world": 2, "mine": 1}) is None
    untracked = torch.nn.SyncBatchNorm(4, track_running_stats=False).eval()
    assert group(untracked, **two) is None                               # batch statistics in eval: torch does not synchronise
    for bn in (plain, sync, own, untracked):
        assert int(bn.num_batches_tracked or 0) == 0                     # asking moves no counter
    monkeypatch.undo()
    assert Fn.cp_sync_group(sync.train()) is None                        # this process has no process group


def _maps(shape, dtype=torch.float32):
    return types.SimpleNamespace(shape=torch.Size(shape), dtype=dtype, is_cuda=True)


def _dense(shape):
    """... with what the rank-local predicates ask of a tensor besides."""
    n = 1
    for s in shape:
        n *= s
    return types.SimpleNamespace(shape=torch.Size(shape), dtype=torch.float32, is_cuda=True, is_contiguous=lambda: True,
                                 numel=lambda: n)


def test_the_route_does_not_depend_on_the_local_batch(monkeypatch):
    g = b = torch.ones(4)
    shapes = [(0, 8, 7, 7), (1, 8, 1, 1), (64, 8, 54, 54)]
    for env in ("NFP_CPOOL_TORCH", "NFP_CPROJ_TORCH"):
        monkeypatch.delenv(env, raising=False)
    for kind in ("pool", "proj"):
        assert [Fn.cp_sync_serves(kind, _maps(s), g, b, 0.1) for s in shapes] == [True] * 3
        assert [Fn.cp_sync_serves(kind, _maps((s[0], 9) + s[2:]), g, b, 0.1) for s in shapes] == [False] * 3
        assert [Fn.cp_sync_serves(kind, _maps(s, torch.float16), g, b, 0.1) for s in shapes] == [False] * 3
        assert not Fn.cp_sync_serves(kind, _maps(shapes[2]), g, b, None)             # momentum=None: a cumulative average
        assert not Fn.cp_sync_serves(kind, _maps(shapes[2]), None, None, 0.1)        # affine=False
        assert not Fn.cp_sync_serves(kind, types.SimpleNamespace(shape=shapes[2], dtype=torch.float32, is_cuda=False), g, b, 0.1)
        with monkeypatch.context() as mp:      # (torch.autocast("cuda") switches itself off where there is no GPU)
            mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
            assert [Fn.cp_sync_serves(kind, _maps(s), g, b, 0.1) for s in shapes] == [False] * 3
        with monkeypatch.context() as mp:
            mp.setattr(torch.compiler, "is_compiling", lambda: True)
            assert [Fn.cp_sync_serves(kind, _maps(s), g, b, 0.1) for s in shapes] == [False] * 3
        env = "NFP_CPROJ_TORCH" if kind == "proj" else "NFP_CPOOL_TORCH"
        monkeypatch.setenv(env, "1")
        assert [Fn.cp_sync_serves(kind, _maps(s), g, b, 0.1) for s in shapes] == [False] * 3
        monkeypatch.setenv(env, "0")
        assert [Fn.cp_sync_serves(kind, _maps((s[0], 32) + s[2:]), g, b, 0.1) for s in shapes] == [True] * 3
        assert not Fn.cp_sync_serves(kind, _maps((4, 33, 7, 7)), g, b, 0.1)
        monkeypatch.delenv(env)
    # the predicates of the rank-local path are as they were: the projection's still by pixel count, none under compile / autocast
    big, small, w = _dense((64, 8, 54, 54)), _dense((4, 8, 7, 7)), torch.zeros(16, 8, 1, 1)
    local = [lambda m: Fn.cpool_hip_serves(m, g, b, 0.1), lambda m: Fn.cproj_hip_serves(m, w, g, b, 0.1),
             lambda m: compress._cp_can_serve(m, g, b, 0.1)]
    assert [f(big) for f in local] == [True] * 3 and [f(small) for f in local] == [True, False, True]
    monkeypatch.setenv("NFP_CPOOL_TORCH", "0")
    assert Fn.cpool_wide_serves(_dense((4, 48, 7, 7)), g, b, 0.1)
    for name, value in ((torch, "is_autocast_enabled"), (torch.compiler, "is_compiling")):
        with monkeypatch.context() as mp:
            mp.setattr(name, value, lambda *a: True)
            assert [f(big) for f in local] == [False] * 3 and not Fn.cpool_wide_serves(_dense((4, 48, 7, 7)), g, b, 0.1)


def test_a_converted_head_without_a_process_group_is_the_head():
    torch.manual_seed(11)
    head = NFPHead(in_c=16, bottleneck_dim=8).train()
    conv = torch.nn.SyncBatchNorm.convert_sync_batchnorm(copy.deepcopy(head))
    assert any(isinstance(m, torch.nn.SyncBatchNorm) for m in conv.modules())
    assert list(conv.state_dict()) == list(head.state_dict())
    x = torch.randn(3, 16, 7, 7)
    go = None
    res = []
    for m in (head, conv):
        xi = x.clone().requires_grad_(True)
        out = m(xi)
        go = torch.randn_like(out) if go is None else go
        out.backward(go)
        res.append((out.detach(), xi.grad, {k: p.grad for k, p in m.named_parameters()}, m.state_dict()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for k, g in res[0][2].items():
        assert (g is None) == (res[1][2][k] is None) and (g is None or torch.equal(g, res[1][2][k])), k
    for k, v in res[0][3].items():
        assert torch.equal(v, res[1][3][k]), k


def test_the_loose_forms_take_a_process_group(monkeypatch):
    """process_group=None and a one-rank group are today's call; a group of two on CPU tensors is torch's own refusal."""
    torch.manual_seed(5)
    maps, w = torch.randn(3, 8, 5, 5), torch.randn(6, 8, 1, 1)
    g, b = torch.rand(6) + 0.5, torch.randn(6)
    args = lambda: (maps, w, g, b, torch.zeros(6), torch.ones(6), True)      # noqa: E731
    want_p, want_m = Fn.nfp_compress_pool_tensors(*args()), Fn.nfp_compress_map_tensors(*args())
    monkeypatch.setattr(torch, "distributed", _FakeDist(sizes={"one": 1, "two": 2}))
    assert torch.equal(Fn.nfp_compress_pool_tensors(*args(), process_group="one"), want_p)
    assert torch.equal(Fn.nfp_compress_map_tensors(*args(), process_group="one"), want_m)
    assert torch.equal(Fn.nfp_compress_pool_tensors(*args()[:6], False, process_group="two"),
                       Fn.nfp_compress_pool_tensors(*args()[:6], False))        # running statistics: nothing to synchronise
    for fn in (Fn.nfp_compress_pool_tensors, Fn.nfp_compress_map_tensors):
        with pytest.raises(ValueError, match="SyncBatchNorm expected input tensor to be on GPU"):
            fn(*args(), process_group="two")
