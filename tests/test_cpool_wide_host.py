"""The wide form of the compress-BN-ReLU-GAP tail on the host: the nfp_cpool_wide_* entries refuse what include/nfp.h says
they refuse, before any HIP call (the pointers are never dereferenced, the launch counter stands still); their length
queries; functional.cpool_wide_serves and the routing under NFP_CPOOL_TORCH / NFP_CPOOL_WIDE on fake tensors; and the CPU heads
at 48 and 80 maps against the reference's fixtures (tests/golden/cases_heads_wide.py).  No GPU needed."""
import re
import os

import pytest
import torch

import cases_heads_wide as KW
from neighbour_feature_pooling_amd import _abi, compress, functional
from test_heads_host import _Fake, fixture_errors, head_module, run_head

INVALID, UNSUPPORTED = -1, -2
MOM, EPS = 0.1, 1e-5
SIZES = dict(B=4, N=48, P=49, D=32)
PTR = 0x1000      # (never dereferenced)
WIDE_EXPORTS = {"nfp_cpool_wide_scratch_floats", "nfp_cpool_wide_forward", "nfp_cpool_wide_backward"}


@pytest.fixture(scope="module")
def lib():
    from neighbour_feature_pooling_amd.build import build_hip
    build_hip()
    return _abi.load()


def _call(L, direction, B, N, P, D, dtype=0, training=1, short=None, null=None, entry="wide", eps=EPS):
    p = dict(maps=PTR, w=PTR, gamma=PTR, beta=PTR, io=PTR, rm=PTR, rv=PTR)
    if null:
        p[null] = None
    query = L.nfp_cpool_wide_scratch_floats if entry == "wide" else L.nfp_cpool_scratch_floats
    ns = int(L.nfp_cpool_saved_floats(N, D)) - (short == "saved")
    nscr = int(query(B, N, P, D, direction == "bwd")) - (short == "scratch")
    args = [B, N, P, D, dtype, training, p["maps"], p["w"], p["gamma"], p["beta"]]
    prefix = "nfp_cpool_wide_" if entry == "wide" else "nfp_cpool_"
    if direction == "fwd":
        args += [p["rm"], p["rv"], MOM, eps, p["io"], PTR, ns, PTR, nscr, None]
        return L.nfp_cpool_wide_forward(*args) if entry == "wide" else getattr(L, prefix + "forward")(*args)
    args += [None if training else p["rm"], None if training else p["rv"], eps, PTR, ns, p["io"], PTR, PTR, PTR, PTR, PTR, nscr,
             None]
    return getattr(L, prefix + "backward")(*args)


REFUSALS = [
    ("N = 0", dict(N=0), INVALID),
    ("N = 97", dict(N=97), UNSUPPORTED),
    ("P = 0", dict(P=0), INVALID),
    ("D = 0", dict(D=0), INVALID),
    ("B = -1", dict(B=-1), INVALID),
    ("dtype = 2", dict(dtype=2), INVALID),
    ("eps < 0", dict(eps=-1.0), INVALID),
    ("NULL maps", dict(null="maps"), INVALID),
    ("NULL w", dict(null="w"), INVALID),
    ("NULL gamma", dict(null="gamma"), INVALID),
    ("NULL beta", dict(null="beta"), INVALID),
    ("NULL out / grad_out", dict(null="io"), INVALID),
    ("short saved", dict(short="saved"), INVALID),
    ("short scratch", dict(short="scratch"), INVALID),
    # the old limits, with the old codes
    ("D > 2^22", dict(D=(1 << 22) + 1), UNSUPPORTED),
    ("N * P >= 2^31", dict(N=96, P=(1 << 31) // 96 + 1), UNSUPPORTED),
    ("B * P == 1 in training", dict(B=1, P=1), UNSUPPORTED),
]


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("label,kw,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_wide_entries_refuse_without_a_launch(lib, direction, label, kw, code):
    L = lib
    n0 = L.nfp_launch_count()
    assert _call(L, direction, **{**SIZES, **kw}) == code
    err = L.nfp_last_error()
    name = b"nfp_cpool_wide_forward" if direction == "fwd" else b"nfp_cpool_wide_backward"
    assert err.startswith(name + b":"), err
    if kw.get("short") == "scratch":
        assert b"nfp_cpool_wide_scratch_floats is" in err, err
    if kw.get("short") == "saved":
        assert b"nfp_cpool_saved_floats is" in err, err
    assert L.nfp_launch_count() == n0


def test_eval_needs_the_running_statistics_and_an_empty_batch_launches_nothing(lib):
    L = lib
    n0 = L.nfp_launch_count()
    assert _call(L, "fwd", **SIZES, training=0, null="rm") == INVALID
    assert _call(L, "bwd", **SIZES, training=0, null="rv") == INVALID
    assert _call(L, "fwd", **{**SIZES, "B": 0}) == 0 and _call(L, "bwd", **{**SIZES, "B": 0}) == 0
    assert L.nfp_launch_count() == n0


def test_the_old_entries_keep_their_limit(lib):
    L = lib
    n0 = L.nfp_launch_count()
    for direction in ("fwd", "bwd"):
        assert _call(L, direction, **{**SIZES, "N": 33}, entry="pool") == UNSUPPORTED
        assert b"N = 33 maps (more than 32)" in L.nfp_last_error()
    assert L.nfp_cpool_scratch_floats(4, 33, 49, 32, 0) == 1
    assert L.nfp_launch_count() == n0


def test_length_queries(lib):
    L = lib
    # saved: the layout of nfp_cpool_saved_floats — mu as two floats, Sigma, 1 / sqrt(var + eps)
    for N in (33, 48, 96):
        assert L.nfp_cpool_saved_floats(N, 512) == 2 * N + N * N + 512
    # forward: a record [a (N), r (N), Gram (N * N)] per chunk, rounded up to an even count, then mu and Sigma as doubles.
    # Chunks: the whole image up to 128 pixels at 48 maps, up to 64 at 64 maps and more
    rec = lambda N: 2 * N + N * N      # noqa: E731
    even = lambda v: (v + 1) // 2 * 2      # noqa: E731
    assert L.nfp_cpool_wide_scratch_floats(4, 33, 35, 48, 0) == even(4 * rec(33)) + 2 * (33 + 33 * 33)
    assert L.nfp_cpool_wide_scratch_floats(4, 48, 49, 40, 0) == 4 * rec(48) + 2 * (48 + 48 * 48)
    assert L.nfp_cpool_wide_scratch_floats(4, 48, 196, 40, 0) == 4 * 2 * rec(48) + 2 * (48 + 48 * 48)
    assert L.nfp_cpool_wide_scratch_floats(2, 96, 256, 24, 0) == 2 * 4 * rec(96) + 2 * (96 + 96 * 96)
    # backward: [slices][D][N + 1] with one image per slice up to 512 / ceil(D / 64) images, then [k, Q] per 32 channels
    assert L.nfp_cpool_wide_scratch_floats(4, 48, 49, 40, 1) == 4 * 40 * 49 + 2 * (48 + 48 * 48)
    assert L.nfp_cpool_wide_scratch_floats(3, 33, 35, 48, 1) == 3 * 48 * 34 + 2 * (33 + 33 * 33)
    assert L.nfp_cpool_wide_scratch_floats(256, 96, 49, 512, 1) == 64 * 512 * 97 + 16 * (96 + 96 * 96)
    for bad in ((0, 48, 49, 32), (4, 0, 49, 32), (4, 97, 49, 32), (4, 48, 0, 32), (4, 48, 49, 0)):
        assert L.nfp_cpool_wide_scratch_floats(*bad, 0) == 1 and L.nfp_cpool_wide_scratch_floats(*bad, 1) == 1


def test_the_entries_are_declared_exported_and_additive(lib):
    src = open(os.path.join(os.path.dirname(__file__), "..", "include", "nfp.h")).read()
    declared = set(re.findall(r"\b(nfp_\w+)\(", src))
    assert WIDE_EXPORTS <= declared and WIDE_EXPORTS <= set(_abi.EXPORTS)
    assert int(re.search(r"#define NFP_ABI_VERSION (\d+)", src).group(1)) == _abi.ABI_VERSION == 7
    for n in WIDE_EXPORTS:
        assert hasattr(lib, n), n
    assert compress._CP_ENTRIES["wide"] == ("nfp_cpool_wide_forward", "nfp_cpool_wide_backward",
                                              "nfp_cpool_wide_scratch_floats")


def test_cpool_wide_serves(monkeypatch):
    monkeypatch.setenv("NFP_CPOOL_TORCH", "0")
    monkeypatch.delenv("NFP_CPOOL_WIDE", raising=False)
    serves = functional.cpool_wide_serves
    g = torch.ones(4)
    assert functional.CPOOL_WIDE_MAX_MAPS == 96 and functional.CPOOL_MAX_MAPS == 32 and functional.CPOOL_ROUTED_MAPS == 8
    for N in (33, 48, 80, 96):
        assert serves(_Fake(shape=(4, N, 7, 7)), g, g, 0.1)
        assert serves(_Fake(shape=(4, N, 7, 7), dtype=torch.bfloat16), g, g, 0.1)
        assert not functional.cpool_hip_serves(_Fake(shape=(4, N, 7, 7)), g, g, 0.1)
    assert not serves(_Fake(shape=(4, 97, 7, 7)), g, g, 0.1)
    assert not serves(_Fake(shape=(4, 48, 7, 7), cuda=False), g, g, 0.1)
    assert not serves(_Fake(shape=(4, 48, 7, 7), dtype=torch.float16), g, g, 0.1)
    assert not serves(_Fake(shape=(4, 48, 7, 7), contiguous=False), g, g, 0.1)
    assert not serves(_Fake(shape=(0, 48, 7, 7)), g, g, 0.1)
    assert not serves(_Fake(shape=(4, 48, 7, 7)), None, None, 0.1)            # affine=False
    assert not serves(_Fake(shape=(4, 48, 7, 7)), g, g, None)                 # momentum=None
    # under torch.autocast("cuda") and under torch.compile (without a device the first cannot be entered: what the
    # predicate asks torch is answered here)
    with monkeypatch.context() as mp:
        mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert not serves(_Fake(shape=(4, 48, 7, 7)), g, g, 0.1)
    assert serves(_Fake(shape=(4, 48, 7, 7)), g, g, 0.1)
    with monkeypatch.context() as mp:
        mp.setattr(torch.compiler, "is_compiling", lambda: True)
        assert not serves(_Fake(shape=(4, 48, 7, 7)), g, g, 0.1)


def test_routing_under_the_switches(monkeypatch):
    kind = compress._cpool_kind
    g = torch.ones(4)
    f = lambda N: _Fake(shape=(4, N, 7, 7))      # noqa: E731
    monkeypatch.delenv("NFP_CPOOL_WIDE", raising=False)
    # unset: 8 maps on the register form; no class of the wide form measured faster, so everything else is the composition
    monkeypatch.delenv("NFP_CPOOL_TORCH", raising=False)
    assert functional.CPOOL_WIDE_ROUTED_CLASSES == ()
    assert [kind(f(N), g, g, 0.1) for N in (8, 9, 32, 33, 48, 96, 97)] == ["pool", None, None, None, None, None, None]
    # "0": the kernels wherever any form can serve
    monkeypatch.setenv("NFP_CPOOL_TORCH", "0")
    assert [kind(f(N), g, g, 0.1) for N in (8, 9, 32, 33, 48, 96, 97)] == ["pool", "pool", "pool", "wide", "wide", "wide", None]
    # NFP_CPOOL_WIDE=1 (measurement): 9 to 32 maps through the wide form wherever the tail is served
    monkeypatch.setenv("NFP_CPOOL_WIDE", "1")
    assert [kind(f(N), g, g, 0.1) for N in (8, 9, 16, 32, 33, 97)] == ["pool", "wide", "wide", "wide", "wide", None]
    monkeypatch.delenv("NFP_CPOOL_TORCH")
    assert [kind(f(N), g, g, 0.1) for N in (8, 9, 32, 48)] == ["pool", None, None, None]      # default routing unchanged
    # "1": the composition everywhere, whatever NFP_CPOOL_WIDE says
    monkeypatch.setenv("NFP_CPOOL_TORCH", "1")
    assert [kind(f(N), g, g, 0.1) for N in (8, 32, 48)] == [None, None, None]
    # a routed class, were one measured: (min maps, max maps, min B * P)
    monkeypatch.delenv("NFP_CPOOL_TORCH")
    monkeypatch.delenv("NFP_CPOOL_WIDE")
    monkeypatch.setattr(compress, "CPOOL_WIDE_ROUTED_CLASSES", ((33, 48, 4 * 49),))
    assert [kind(f(N), g, g, 0.1) for N in (32, 33, 48, 49)] == [None, "wide", "wide", None]
    assert kind(_Fake(shape=(3, 48, 7, 7)), g, g, 0.1) is None


@pytest.mark.parametrize("name", [c["name"] for c in KW.HEAD_WIDE_CASES])
def test_cpu_heads_match_the_reference_fixtures(name):
    c = KW.HEAD_WIDE_BY_NAME[name]
    m, g = head_module(c)
    assert m.compress[0].in_channels == KW.HEAD_WIDE_MAPS[name]
    errs = fixture_errors(run_head(m, c), g)
    print(name, errs)
    assert {"g:compress.0.weight", "g:compress.1.weight", "g:compress.1.bias", "after:compress.1.running_mean",
            "after:compress.1.running_var", "after:compress.1.num_batches_tracked"} <= set(errs)
    for k, e in errs.items():
        assert e <= 1e-5, (k, e)
