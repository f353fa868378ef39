"""The strided kernels (csrc/nfp_strided.hip: fwd_strided / bwd_strided, stride 2 to 4) against the ORACLE (oracle/nfp_oracle.c)
on seeded inputs from synth.feature_map, and against the reference's fixtures (tests/golden/cases_strided.py): the smallest
shapes at which one output, the untouched pixels, the window overlap classes, the ring under the three padding modes, the
channel chunks, the row bands and the two layouts can go wrong; the edge values; determinism; the C++ node; the A/B switch;
the refusals; torch.compile; poisoned and fenced buffers; the LDS-poison build; NFPInsert(strided_layer=True).  Every served
case asserts the kernel family and ONE launch each way.  Bars: those of the valid-map family, the same arithmetic
(tests/test_gpu_valid.py): float32 1e-5 of the tensor's max; bf16 1e-2 (maps) / 2e-2 (grad_x) on bf16-rounded inputs."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases as K
import cases_strided as KS
import poison as P
from conftest import load_golden, rel_err, same_nan_pattern
from test_gpu_valid import TOL, TOL_BF16_GX, TOL_BF16_OUT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_WP = 128        # W + 2P at most (include/nfp.h)


def geo(shape, R=1, s=2, P=0, mode="reflect", meas=("cosine", "norm")):
    return dict(shape=shape, R=R, s=s, P=P, mode=mode, meas=meas)


ONE_OUTPUT = [geo((2, 8, 3, 3)), geo((2, 8, 5, 5), R=2), geo((2, 8, 2, 2), P=1), geo((2, 8, 2, 2), P=1, mode="zeros"),
              geo((2, 8, 3, 3), R=2, P=2)]
UNTOUCHED = [(geo((2, 8, 4, 4)), 7), (geo((2, 8, 7, 7), s=4), 13), (geo((2, 8, 9, 9), R=2, s=3), 17)]
OVERLAP = [geo((2, 8, 5, 5)), geo((2, 8, 6, 6), s=3), geo((2, 8, 7, 7), R=2), geo((2, 8, 9, 9), R=2, s=4)]
ROWS_COLUMNS = [geo((1, 8, 3, 9), meas=("dot",)), geo((1, 8, 9, 3), meas=("gfc",)), geo((2, 16, 7, 6)), geo((1, 12, 5, 13))]
PADDED = [geo(sh, R=R, s=s, P=R, mode=m) for sh, R, s in (((2, 8, 7, 7), 1, 2), ((2, 8, 8, 8), 1, 2), ((2, 8, 7, 6), 2, 3))
          for m in ("zeros", "reflect", "replicate")]
CHANNELS = [geo((2, 1, 6, 6)), geo((2, 3, 6, 7)), geo((2, 6, 7, 7)), geo((2, 512, 7, 7)), geo((2, 192, 14, 14)),
            geo((2, 512, 7, 7), P=1), geo((2, 192, 14, 14), R=2, P=2, mode="replicate")]
BANDS = [geo((2, 8, 24, 23)), geo((2, 8, 24, 23), R=2, P=2, mode="replicate"), geo((1, 16, 41, 37)), geo((1, 16, 41, 37), s=3, P=1),
         geo((1, 8, 130, 126), P=1), geo((1, 8, 130, 126), P=1, mode="zeros", s=4),
         geo((1, 8, 9, MAX_WP)), geo((1, 8, 12, MAX_WP - 2), P=1, mode="replicate"), geo((1, 8, 11, MAX_WP), R=2)]   # the widest served rows
MANY = [geo((300, 8, 6, 6))]
GRID = ONE_OUTPUT + [g for g, _ in UNTOUCHED] + OVERLAP + ROWS_COLUMNS + PADDED + CHANNELS + BANDS + MANY


def _gid(g):
    return "x".join(map(str, g["shape"])) + f"-R{g['R']}s{g['s']}P{g['P']}{g['mode'] if g['P'] else ''}"


def _grid():
    out = []
    for g in GRID:
        for meas in g["meas"]:
            out.append((g, meas, "f32", "nchw"))
            if g["shape"][1] % 8 == 0:
                out += [(g, meas, "f32", "nhwc"), (g, meas, "bf16", "nchw"), (g, meas, "bf16", "nhwc")]
    return out


def _ctor(g, meas, sim=True):
    ctor = dict(R=g["R"], measure=meas, padding=g["P"], stride=g["s"], padding_mode=g["mode"], similarity=sim)
    if meas == "norm":
        ctor["p"] = 2
    return ctor


def _key(g):
    return (g["shape"], g["R"], g["s"], g["P"], g["mode"])


def _bf16_round(a):
    return torch.from_numpy(a).bfloat16().float().numpy()


def _out_hw(g):
    (_, _, H, W), R, s, P = g["shape"], g["R"], g["s"], g["P"]
    return (H + 2 * P - 2 * R - 1) // s + 1, (W + 2 * P - 2 * R - 1) // s + 1


def _inputs(key, tweak=None, kind="normal"):
    from neighbour_feature_pooling_amd.synth import feature_map
    (B, C, H, W), R, s, P, mode = key
    x = feature_map((B, C, H, W), 5 * H + W + 3 * C + B + 7 * s, kind)
    if tweak == "zero_pixels":      # all-zero pixels: a centre, a tap, and (P > 0) the border pixels the ring copies
        for b, y, xx in ((0, R - P if P == 0 else 0, R - P if P == 0 else 0), (0, 3, 2), (0, 3, 3), (1, H - 1, 2), (1, 2, 2), (1, 0, W - 1)):
            x[b, :, y, xx] = 0.0
    elif tweak == "identical":      # two identical adjacent pixels (distance 0), once along a row, once down a column
        x[0, :, 3, 3] = x[0, :, 3, 2]
        x[1, :, 4, 2] = x[1, :, 3, 2]
    Ho, Wo = _out_hw(dict(shape=(B, C, H, W), R=R, s=s, P=P))
    go = feature_map((B, (2 * R + 1) ** 2 - 1, Ho, Wo), 3 * H + W + 1000 + s)
    return x, go


@functools.lru_cache(maxsize=None)
def _reference(key, meas, sim, bf16, tweak=None, kind="normal"):
    """(out, grad_x) of the oracle, computed once per case and shared by the layouts (bf16: on the rounded inputs)."""
    import oracle
    oracle.build()
    x, go = _inputs(key, tweak, kind)
    if bf16:
        x, go = _bf16_round(x), _bf16_round(go)
    shape, R, s, P, mode = key
    ctor = _ctor(dict(R=R, s=s, P=P, mode=mode), meas, sim)
    return oracle.forward(x, **ctor), oracle.backward(x, go, **ctor)


def _config(C, g, meas, sim=True):
    from neighbour_feature_pooling_amd import NFPPooling
    return NFPPooling(C, **_ctor(g, meas, sim)).config


def _device_run(x, go, cfg, dtype, layout, strided=False, expect=True, op=None):
    """(out, grad_x, forward variant, backward variant) of functional.nfp_strided on the device; with `expect` the kernel
    family and the launch counts (one each way) are asserted."""
    from neighbour_feature_pooling_amd import _abi, nfp_strided
    L = _abi.load()
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    xt = torch.from_numpy(x).to(DEV).to(tdt)
    if strided:     # a batch-strided view: the first C channels of a tensor with 2C
        assert layout == "nchw"
        xt = torch.cat([xt, xt + 1], dim=1)[:, :x.shape[1]]
    elif layout == "nhwc":
        xt = xt.contiguous(memory_format=torch.channels_last)
    xt = xt.detach().requires_grad_(True)
    got = torch.from_numpy(go).to(DEV).to(tdt)
    n0 = L.nfp_launch_count()
    out = (op or nfp_strided)(xt, cfg)
    n1 = L.nfp_launch_count()
    fv = L.nfp_last_variant().decode()
    gx, = torch.autograd.grad(out, xt, got)
    torch.cuda.synchronize()
    n2 = L.nfp_launch_count()
    bv = L.nfp_last_variant().decode()
    if expect:
        assert fv.startswith("fwd_strided<") and bv.startswith("bwd_strided<"), (fv, bv)
        assert (n1 - n0, n2 - n1) == (1, 1), (n1 - n0, n2 - n1)
        assert (layout in fv) and (dtype in fv) and (layout in bv) and (dtype in bv), (fv, bv)
    assert out.dtype == tdt and gx.dtype == tdt and gx.shape == xt.shape
    return out.detach().float().cpu().numpy(), gx.float().cpu().numpy(), fv, bv


def _check(got_out, got_gx, ref_out, ref_gx, dtype, what=""):
    assert got_out.shape == ref_out.shape
    assert same_nan_pattern(got_out, ref_out) and same_nan_pattern(got_gx, ref_gx), what
    eo = rel_err(np.nan_to_num(got_out), np.nan_to_num(ref_out))
    eg = rel_err(np.nan_to_num(got_gx), np.nan_to_num(ref_gx))
    print(what, "out", eo, "grad_x", eg)
    assert eo <= (TOL_BF16_OUT if dtype == "bf16" else TOL), what
    assert eg <= (TOL_BF16_GX if dtype == "bf16" else TOL), what


def _case(g, meas, dtype="f32", layout="nchw", sim=True, strided=False, tweak=None, kind="normal"):
    x, go = _inputs(_key(g), tweak, kind)
    ref_out, ref_gx = _reference(_key(g), meas, sim, dtype == "bf16", tweak, kind)
    out, gx, fv, bv = _device_run(x, go, _config(g["shape"][1], g, meas, sim), dtype, layout, strided)
    fam = "prod" if meas in ("cosine", "dot", "gfc") else "dist"
    assert f"<{g['R']},{fam}," in fv and f"<{g['R']},{fam}," in bv, (fv, bv)
    _check(out, gx, ref_out, ref_gx, dtype, f"{_gid(g)} {meas} {dtype} {layout} {fv} {bv}")
    return out, gx, ref_gx


@pytest.mark.parametrize("g,meas,dtype,layout", _grid(), ids=lambda v: _gid(v) if isinstance(v, dict) else str(v))
def test_strided_kernels_match_the_oracle(g, meas, dtype, layout):
    _case(g, meas, dtype, layout)


@pytest.mark.parametrize("g,count", UNTOUCHED, ids=lambda v: _gid(v) if isinstance(v, dict) else str(v))
@pytest.mark.parametrize("meas", ["cosine", "norm"])
@pytest.mark.parametrize("dtype,layout", [("f32", "nchw"), ("bf16", "nhwc")])
def test_pixels_no_window_touches_get_an_explicit_zero(g, count, meas, dtype, layout):
    _, gx, ref_gx = _case(g, meas, dtype, layout)
    untouched = np.all(ref_gx == 0.0, axis=(0, 1))
    assert int(untouched.sum()) == count, untouched.sum()
    assert np.all(gx[:, :, untouched] == 0.0)


@pytest.mark.parametrize("g", [geo((2, 16, 7, 6)), geo((2, 8, 24, 23), R=2, P=2, mode="reflect")], ids=_gid)
@pytest.mark.parametrize("meas,sim", [("dot", True), ("gfc", True), ("rmse", True), ("dot", False), ("gfc", False), ("rmse", False),
                                      ("cosine", False), ("norm", False)])
def test_the_other_hot_measures_and_dissimilarity(g, meas, sim):
    _case(g, meas, "f32", "nchw", sim=sim)
    _case(g, meas, "f32", "nhwc", sim=sim)


@pytest.mark.parametrize("g", [geo((2, 16, 7, 6)), geo((2, 8, 24, 23), P=1)], ids=_gid)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("meas", ["cosine", "norm"])
def test_batch_strided_views_are_read_in_place(g, dtype, meas):
    _case(g, meas, dtype, "nchw", strided=True)


@pytest.mark.parametrize("g,nans", [(geo((2, 8, 7, 7), P=1, mode="replicate"), 192), (geo((2, 8, 7, 6), R=2, s=3, P=2, mode="replicate"), 80)],
                         ids=lambda v: _gid(v) if isinstance(v, dict) else str(v))
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_rmse_under_replicate_has_the_oracle_nan_pattern(g, nans, layout):
    """A centre on the border and its replicated copy are at distance 0: finite maps, grad_x NaN exactly where the oracle's is."""
    out, gx, ref_gx = _case(g, "rmse", "f32", layout)
    assert np.isfinite(out).all() and int(np.isnan(ref_gx).sum()) == nans and int(np.isnan(gx).sum()) == nans


@pytest.mark.parametrize("g", [geo((2, 16, 7, 6)), geo((2, 16, 7, 6), P=1, mode="replicate"), geo((2, 16, 7, 6), R=2, P=2)], ids=_gid)
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_cosine_on_a_relu_input_with_all_zero_pixels(g, layout):
    _case(g, "cosine", "f32", layout, tweak="zero_pixels", kind="relu")


@pytest.mark.parametrize("meas", ["rmse", "norm"])
@pytest.mark.parametrize("g", [geo((2, 8, 24, 23), R=2), geo((2, 8, 24, 23), P=1, mode="zeros")], ids=_gid)
def test_two_identical_adjacent_pixels_follow_the_oracle(meas, g):
    _case(g, meas, "f32", "nchw", tweak="identical")
    _case(g, meas, "f32", "nhwc", tweak="identical")


@pytest.mark.parametrize("name", [c["name"] for c in KS.STRIDED_CASES] + KS.EXISTING)
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_the_kernels_match_the_reference_fixtures(name, layout):
    from neighbour_feature_pooling_amd import NFPPooling
    c = KS.STRIDED_BY_NAME.get(name) or K.BY_NAME[name]
    g = load_golden(name)
    x = K.make_input(c)
    go = K.make_grad_out(c, g["out"].shape)
    out, gx, fv, bv = _device_run(x, go, NFPPooling(c["shape"][1], **c["ctor"]).config, "f32", layout)
    _check(out, gx, g["out"], g["gx"], "f32", f"{name} {layout} {fv} {bv}")


@pytest.mark.parametrize("meas,g,dtype,layout", [("cosine", geo((5, 16, 24, 23), P=1), "f32", "nchw"), ("norm", geo((5, 16, 24, 23), R=2), "f32", "nhwc"),
                                                 ("gfc", geo((5, 16, 24, 23), R=2, P=2, mode="replicate", s=3), "bf16", "nchw"),
                                                 ("rmse", geo((5, 16, 24, 23), s=4), "bf16", "nhwc")], ids=lambda v: _gid(v) if isinstance(v, dict) else str(v))
def test_two_runs_agree_bitwise_and_an_image_does_not_depend_on_the_batch(meas, g, dtype, layout):
    x, go = _inputs(_key(g))
    cfg = _config(16, g, meas)
    a = _device_run(x, go, cfg, dtype, layout)
    b = _device_run(x, go, cfg, dtype, layout)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    one = _device_run(x[:1].copy(), go[:1].copy(), cfg, dtype, layout)
    assert np.array_equal(a[0][:1], one[0]) and np.array_equal(a[1][:1], one[1])


@pytest.mark.parametrize("meas,g,dtype,layout", [("cosine", geo((3, 16, 9, 10), P=1), "f32", "nchw"), ("norm", geo((3, 16, 9, 10), R=2), "bf16", "nhwc")],
                         ids=lambda v: _gid(v) if isinstance(v, dict) else str(v))
def test_the_python_node_agrees_bitwise_with_the_cpp_node(meas, g, dtype, layout, monkeypatch):
    from neighbour_feature_pooling_amd import functional as Fn
    if not Fn._cpp_entry("nfp_strided_apply"):
        pytest.fail("the C++ node nfp_strided_apply is missing from _nfp_torch.so")
    x, go = _inputs(_key(g))
    cfg = _config(16, g, meas)
    a = _device_run(x, go, cfg, dtype, layout)
    monkeypatch.setenv("NFP_PY_NODES", "1")
    monkeypatch.setattr(Fn, "_CPP", None)
    assert Fn._cpp_entry("nfp_strided_apply") is None
    b = _device_run(x, go, cfg, dtype, layout)
    monkeypatch.setattr(Fn, "_CPP", None)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_an_empty_batch_launches_nothing():
    from neighbour_feature_pooling_amd import _abi, nfp_strided
    L = _abi.load()
    x = torch.zeros(0, 8, 7, 7, device=DEV, requires_grad=True)
    n0 = L.nfp_launch_count()
    out = nfp_strided(x, _config(8, geo((0, 8, 7, 7)), "cosine"))
    assert tuple(out.shape) == (0, 8, 3, 3) and out.dtype == torch.float32
    gx, = torch.autograd.grad(out, x, torch.zeros_like(out))
    assert tuple(gx.shape) == (0, 8, 7, 7) and L.nfp_launch_count() == n0


def test_the_switch_routes_to_the_any_geometry_kernels(monkeypatch):
    g = geo((2, 16, 7, 6), P=1)
    x, go = _inputs(_key(g))
    ref_out, ref_gx = _reference(_key(g), "cosine", True, False)
    cfg = _config(16, g, "cosine")
    monkeypatch.setenv("NFP_STRIDED_OFF", "1")
    out, gx, fv, bv = _device_run(x, go, cfg, "f32", "nchw", expect=False)
    assert fv.startswith("fwd_pairs") and bv.startswith("bwd_gather"), (fv, bv)
    _check(out, gx, ref_out, ref_gx, "f32", f"NFP_STRIDED_OFF=1: {fv} {bv}")
    monkeypatch.delenv("NFP_STRIDED_OFF")
    out, gx, fv, bv = _device_run(x, go, cfg, "f32", "nchw")
    _check(out, gx, ref_out, ref_gx, "f32", f"switch unset: {fv} {bv}")


def test_refused_calls_fall_to_nfp_with_its_variants():
    from neighbour_feature_pooling_amd import NFPPooling, nfp_op, nfp_strided
    # canberra, and a row over the bound: nfp serves, bit for bit what nfp itself returns
    for shape, ctor in (((2, 8, 7, 6), dict(measure="canberra", stride=2, padding=1)), ((1, 8, 7, 300), dict(measure="cosine", stride=2))):
        cfg = NFPPooling(8, **ctor).config
        key = (shape, 1, 2, ctor.get("padding", 0), "reflect")
        x, go = _inputs(key)
        x = np.abs(x) + 0.25
        out, gx, fv, bv = _device_run(x, go, cfg, "f32", "nchw", expect=False)
        assert not fv.startswith("fwd_strided") and not bv.startswith("bwd_strided"), (fv, bv)
        out2, gx2, fv2, bv2 = _device_run(x, go, cfg, "f32", "nchw", expect=False, op=nfp_op)
        assert (fv, bv) == (fv2, bv2) and np.array_equal(out, out2) and np.array_equal(gx, gx2)
    with pytest.raises(ValueError):
        nfp_strided(torch.zeros(1, 8, 9, 9, device=DEV), NFPPooling(8, measure="cosine", stride=2, dilation=2).config)


def test_under_torch_compile_the_call_is_nfp():
    from neighbour_feature_pooling_amd import nfp_op, nfp_strided
    g = geo((2, 8, 9, 10), P=1)
    cfg = _config(8, g, "cosine")
    x, go = _inputs(_key(g))
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    got = torch.from_numpy(go).to(DEV)
    ref = nfp_op(xt, cfg)
    ref_gx, = torch.autograd.grad(ref, xt, got)
    out = torch.compile(lambda t: nfp_strided(t, cfg))(xt)
    gx, = torch.autograd.grad(out, xt, got)
    assert torch.equal(out, ref) and torch.equal(gx, ref_gx)


POISON_GEOS = [geo((2, 8, 4, 4)), geo((2, 8, 7, 7), s=4), geo((2, 8, 8, 8), P=1), geo((2, 8, 7, 7), R=2, P=2, mode="replicate")]


@pytest.mark.parametrize("g", POISON_GEOS, ids=_gid)
@pytest.mark.parametrize("meas", ["cosine", "norm"])
@pytest.mark.parametrize("dtype,layout", [("f32", "nchw"), ("bf16", "nhwc")])
def test_poisoned_and_fenced_buffers(g, meas, dtype, layout, monkeypatch):
    """tests/poison.py: out, grad_x and the variants are bit for bit the same under the three fills, no guard byte changes, and
    the zero-fill run meets the bar.  (The Python node allocates in Python: it serves here.)"""
    from neighbour_feature_pooling_amd import _abi, functional as Fn
    monkeypatch.setenv("NFP_PY_NODES", "1")
    monkeypatch.setattr(Fn, "_CPP", None)
    L = _abi.load()
    x, go = _inputs(_key(g))
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    cfg = _config(8, g, meas)
    xd = torch.from_numpy(x).to(DEV).to(tdt)
    if layout == "nhwc":
        xd = xd.contiguous(memory_format=torch.channels_last)
    god = torch.from_numpy(go).to(DEV).to(tdt)

    def case(poison):
        xt = poison.fenced(xd).requires_grad_(True)
        gt = poison.fenced(god)
        out = Fn.nfp_strided(xt, cfg)
        fv = L.nfp_last_variant().decode()
        gx, = torch.autograd.grad(out, xt, gt)
        torch.cuda.synchronize()
        bv = L.nfp_last_variant().decode()
        assert fv.startswith("fwd_strided<") and bv.startswith("bwd_strided<"), (fv, bv)
        return dict(out=out.detach(), gx=gx, fv=fv, bv=bv)

    zero = P.run_fills(case, _gid(g))
    monkeypatch.setattr(Fn, "_CPP", None)
    ref_out, ref_gx = _reference(_key(g), meas, True, dtype == "bf16")
    _check(zero["out"].float().cpu().numpy(), zero["gx"].float().cpu().numpy(), ref_out, ref_gx, dtype, f"poison {_gid(g)} {meas} {dtype} {layout}")


def test_band_cases_with_poisoned_lds():
    """The band, padding and untouched-pixel cases once more on the -DNFP_LDS_POISON build (libnfp_hip_poison.so), loaded the way
    tests/test_gpu_tile.py loads it: every word of a workgroup's LDS is a signalling NaN before the kernel proper starts."""
    if os.environ.get("NFP_TEST_LIB"):
        pytest.skip("this IS the run on the test build")
    env = dict(os.environ, NFP_TEST_LIB="libnfp_hip_poison.so")
    sel = "match_the_oracle and (24x23 or 41x37 or 7x7 or 8x8 or 7x6 or 9x9) or explicit_zero or rmse_under_replicate"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", sel,
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout, tail


def test_insert_with_the_strided_layer_matches_the_block_without():
    from neighbour_feature_pooling_amd import NFPInsert, _abi
    L = _abi.load()
    kw = dict(measure="cosine", stride=2, padding=1)
    torch.manual_seed(4)
    off = NFPInsert(16, **kw).to(DEV)
    torch.manual_seed(4)
    on = NFPInsert(16, strided_layer=True, **kw).to(DEV)
    torch.manual_seed(6)
    x0 = torch.randn(4, 16, 14, 14, device=DEV)
    res = []
    for m in (off, on):
        x = x0.clone().requires_grad_(True)
        cfg = m.nfp.config
        n0 = L.nfp_launch_count()
        maps = m._layer(x)
        fv = L.nfp_last_variant().decode()
        gm, = torch.autograd.grad(maps, x, torch.ones_like(maps))
        torch.cuda.synchronize()
        res.append((fv, L.nfp_last_variant().decode(), L.nfp_launch_count() - n0))
        x = x0.clone().requires_grad_(True)
        out = m(x)
        out.backward(torch.linspace(-1, 1, out.numel(), device=DEV).reshape(out.shape))
        res[-1] += (out.detach().cpu().numpy(), x.grad.cpu().numpy())
        assert cfg.stride == 2
    assert res[1][0].startswith("fwd_strided<") and res[1][1].startswith("bwd_strided<") and res[1][2] == 2, res[1][:3]
    assert res[0][0].startswith("fwd_pairs") and res[0][1].startswith("bwd_gather"), res[0][:3]
    assert rel_err(res[1][3], res[0][3]) <= TOL and rel_err(res[1][4], res[0][4]) <= TOL
