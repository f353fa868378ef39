"""Where radius-3 (7 x 7 window) "same" maps go, checked WITHOUT a GPU through nfp_plan and the dry-run queries: the row-band
kernels fwd_tile<R3,...> / bwd_tile<R3,...> (csrc/nfp_tile.h; nfp_launch.h::tile_r3_geometry) for the product and
squared-difference families, both storage types and layouts, W <= 45; everything else on the any-geometry kernels as
before.  NFP_TILE_R3=0 and NFP_FORCE_GENERIC=1 are the routing from before these instantiations existed, and no R <= 2
descriptor moves with the switch."""
import ctypes
import random

import pytest

from neighbour_feature_pooling_amd import _abi
from test_dispatch_plan import LDS_MAX, desc, launches, lib, plan  # noqa: F401  (lib: the module's fixture)


def _set(lib_, monkeypatch, **env):
    for k in ("NFP_TILE_R3", "NFP_FORCE_GENERIC"):
        if k in env and env[k] is not None:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)
    lib_.nfp_reload_env()


@pytest.fixture(autouse=True)
def _switches_back(lib):
    yield
    lib.nfp_reload_env()   # (monkeypatch has not undone the environment yet: conftest's autouse fixture re-reads at the next test's start)


# (descriptor, the variant's "<measure>,<storage>,<layout>" part, bands per image)
SERVED = [
    (dict(shape=(64, 512, 7, 7)), "cos,f32,nchw", 1),                      # the heads' map: W = 2R + 1
    (dict(shape=(4, 16, 7, 7)), "cos,f32,nchw", 1),
    (dict(shape=(2, 8, 4, 8)), "cos,f32,nchw", 1),                         # H = R + 1: the minimal band
    (dict(shape=(256, 192, 14, 14), measure="norm", dtype=_abi.BF16, channels_last=True), "l2,bf16,nhwc", 2),
    (dict(shape=(64, 40, 28, 28)), "cos,f32,nchw", 7),
    (dict(shape=(2, 8, 14, 14)), "cos,f32,nchw", 3),                       # bands of 5 / 5 / 4 rows
    (dict(shape=(2, 8, 7, 7), measure="gfc", mode="replicate"), "gfc,f32,nchw", 1),
    (dict(shape=(2, 8, 7, 7), measure="dot", mode="zeros"), "dot,f32,nchw", 1),
    (dict(shape=(2, 8, 7, 7), measure="rmse", dtype=_abi.BF16), "rmse,bf16,nchw", 1),
]
# ... and what stays on the any-geometry kernels
NOT_SERVED = [dict(shape=(2, 8, 3, 8), mode="zeros"),                      # H = 3 < R + 1
              dict(shape=(2, 6, 7, 7)),                                    # C % 4
              dict(shape=(2, 8, 7, 7), pad=2), dict(shape=(2, 8, 9, 9), stride=2), dict(shape=(2, 8, 7, 7), mode="circular"),
              dict(shape=(2, 8, 7, 7), measure="norm", p=1.0), dict(shape=(2, 8, 7, 7), measure="canberra")]
W_MAX = 45   # (W + 6) * 10 <= 512: a band of R + 1 rows and its halo in the backward's 512 threads


def _both(lib_, d):
    out = []
    for backward in (False, True):
        rc, text = plan(lib_, d, backward)
        assert rc == 0, lib_.nfp_last_error()
        out.append(text)
    return out


@pytest.mark.parametrize("d_kw,tag,nb", SERVED)
def test_served_rows_plan_the_row_band_kernels(lib, monkeypatch, d_kw, tag, nb):
    _set(lib, monkeypatch, NFP_TILE_R3="1")
    d = desc(R=3, **d_kw)
    f, b = _both(lib, d)
    assert f.split(" | ")[0] == "fwd_tile<R3,%s>x%d" % (tag, nb), f
    assert b.split(" | ")[0] == "bwd_tile<R3,%s>x%d" % (tag, nb), b
    for name, grid, block, lds in launches(f) + launches(b):
        assert block <= 1024 and lds <= LDS_MAX, (f, b)
    assert launches(b)[0][2] <= 512, b            # the k = 7 backward's launch bound
    # no workspace, no tables; both fused tails served, their scratch covering every band's partial sums
    assert lib.nfp_workspace_bytes(ctypes.byref(d)) == 0
    lib.nfp_pool_supported.restype = lib.nfp_gap_supported.restype = ctypes.c_int
    lib.nfp_pool_saved_floats.restype = lib.nfp_gap_saved_floats.restype = ctypes.c_int64
    assert lib.nfp_pool_supported(ctypes.byref(d)) == 1 and lib.nfp_gap_supported(ctypes.byref(d)) == 1
    B, C, H, W = d_kw["shape"]
    base = B * H * W if tag.startswith(("cos", "gfc")) else 0
    assert lib.nfp_pool_saved_floats(ctypes.byref(d)) == base + B * nb * (C + 48)
    assert lib.nfp_gap_saved_floats(ctypes.byref(d)) == base + B * nb * C


def test_map_f32_stays_on_the_general_kernels(lib, monkeypatch):
    _set(lib, monkeypatch, NFP_TILE_R3="1")
    d = desc((4, 16, 7, 7), R=3, dtype=_abi.BF16)
    d.map_f32 = 1
    f, b = _both(lib, d)
    assert f.startswith("fwd_pairs") and b.startswith("bwd_gather"), (f, b)


@pytest.mark.parametrize("d_kw", NOT_SERVED)
def test_rows_outside_the_served_set_stay_on_the_general_kernels(lib, monkeypatch, d_kw):
    _set(lib, monkeypatch, NFP_TILE_R3="1")
    d = desc(R=3, **d_kw)
    f, b = _both(lib, d)
    assert f.startswith("fwd_pairs") and b.startswith(("bwd_gather", "bwd_direct")), (f, b)
    lib.nfp_pool_supported.restype = lib.nfp_gap_supported.restype = ctypes.c_int
    assert lib.nfp_pool_supported(ctypes.byref(d)) == 0 and lib.nfp_gap_supported(ctypes.byref(d)) == 0


def test_forward_and_backward_serve_the_same_maps(lib, monkeypatch):
    """The forward must refuse what the backward refuses — a fused tail needs both, and the backward (512 threads) is the
    narrower: the widest row, the row after it, and a sweep of sizes, the gap query agreeing with both plans."""
    _set(lib, monkeypatch, NFP_TILE_R3="1")
    lib.nfp_gap_supported.restype = ctypes.c_int
    for W, served in ((W_MAX, True), (W_MAX + 1, False)):
        for H in (4, 5, 8, 9, 30):
            d = desc((2, 8, H, W), R=3)
            f, b = _both(lib, d)
            want = served and H % 4 == 0     # (bands of exactly 4 rows at W = 45)
            assert f.startswith("fwd_tile<R3") == want and b.startswith("bwd_tile<R3") == want, (H, W, f, b)
    rnd = random.Random(703)
    n = 0
    for _ in range(1500):
        shape = (rnd.choice([1, 3, 64, 600]), rnd.choice([4, 8, 40, 512]), rnd.randint(4, 60), rnd.randint(4, 48))
        d = desc(shape, R=3, mode=rnd.choice(["reflect", "replicate", "zeros"]), measure=rnd.choice(["cosine", "norm", "gfc"]),
                 dtype=rnd.choice([_abi.F32, _abi.BF16]), channels_last=rnd.random() < 0.5)
        f, b = _both(lib, d)
        ft, bt = f.startswith("fwd_tile<R3"), b.startswith("bwd_tile<R3")
        assert ft == bt == bool(lib.nfp_gap_supported(ctypes.byref(d))), (shape, f, b)
        n += ft
        for name, grid, block, lds in launches(f) + launches(b):
            assert block <= 1024 and lds <= LDS_MAX, (f, b)
    assert n > 800


def _r3_rows():
    return [desc(R=3, **kw) for kw, _, _ in SERVED] + [desc(R=3, **kw) for kw in NOT_SERVED]


@pytest.mark.parametrize("env", [dict(NFP_TILE_R3="0"), dict(NFP_FORCE_GENERIC="1"), dict(NFP_TILE_R3="1", NFP_FORCE_GENERIC="1")])
def test_switched_off_is_the_routing_from_before(lib, monkeypatch, env):
    """fwd_pairs and bwd_gather / bwd_direct for every radius-3 row, no fused tail: what the library planned before it had
    k = 7 instantiations of the row-band kernels."""
    _set(lib, monkeypatch, **env)
    lib.nfp_pool_supported.restype = lib.nfp_gap_supported.restype = ctypes.c_int
    for d in _r3_rows():
        f, b = _both(lib, d)
        assert f.startswith("fwd_pairs | ") and b.startswith(("bwd_gather", "bwd_direct")), (env, f, b)
        assert lib.nfp_pool_supported(ctypes.byref(d)) == 0 and lib.nfp_gap_supported(ctypes.byref(d)) == 0


def test_default_routing_serves_the_classes_that_measured_faster(lib, monkeypatch):
    """NFP_TILE_R3 unset: batches of at least 12 544 pixels (every measured one won there, every measured one
    below lost or tied); smaller batches keep the kernels they had."""
    _set(lib, monkeypatch)
    lib.nfp_gap_supported.restype = ctypes.c_int
    for shape, kw, served in [((256, 512, 7, 7), {}, True), ((64, 192, 14, 14), dict(measure="norm"), True),
                              ((16, 40, 28, 28), {}, True), ((64, 40, 28, 28), {}, True),
                              ((255, 512, 7, 7), {}, False), ((64, 512, 7, 7), {}, False), ((4, 16, 7, 7), {}, False)]:
        d = desc(shape, R=3, **kw)
        f, b = _both(lib, d)
        assert f.startswith("fwd_tile<R3,") == served and b.startswith("bwd_tile<R3,") == served, (shape, f, b)
        assert f.startswith("fwd_pairs") != served
        assert lib.nfp_gap_supported(ctypes.byref(d)) == int(served)


def test_radius_1_and_2_do_not_move_with_the_switch(lib, monkeypatch):
    rnd = random.Random(41)
    ds = []
    for _ in range(400):
        R = rnd.choice([1, 2])
        ds.append(desc((rnd.choice([1, 16, 256]), rnd.choice([4, 16, 192, 510]), rnd.choice([3, 7, 14, 28, 56]), rnd.choice([4, 7, 14, 37, 112])),
                       R=R, pad=rnd.choice([0, R, R]), stride=rnd.choice([1, 1, 2]), mode=rnd.choice(_abi.PAD_MODES),
                       measure=rnd.choice(["cosine", "norm", "gfc", "canberra", "emd"]), p=rnd.choice([1.0, 2.0]),
                       dtype=rnd.choice([_abi.F32, _abi.BF16]), channels_last=rnd.random() < 0.3))
    got = {}
    for sw in ("0", "1"):
        _set(lib, monkeypatch, NFP_TILE_R3=sw)
        got[sw] = [(plan(lib, d, False), plan(lib, d, True)) for d in ds]
    assert got["0"] == got["1"]
    assert sum(rc == 0 for (rc, _), _ in got["0"]) > 300
