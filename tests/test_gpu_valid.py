"""The valid-map kernels (csrc/nfp_valid.hip: fwd_valid / bwd_valid, padding 0) against the ORACLE (oracle/nfp_oracle.c) with
padding=0 on seeded inputs from synth.feature_map: the smallest shapes at which the half stencil, the row bands, the channel
chunks and the two layouts can go wrong, the edge values, a seeded sweep, determinism, a refusal and the A/B switch.  Every
served case asserts the kernel family and ONE launch each way.  Bars: float32 1e-5 of the tensor's max (test_gpu_tile.TOL);
bf16 1e-2 (maps) / 2e-2 (grad_x) on bf16-rounded inputs.

(2, 1, 6, 6) cosine: with C = 1 every cosine is +-1 and its gradient is identically zero — the float64 oracle returns exact
zeros, so `rel_err` divides by 1 and the bar is an ABSOLUTE 1e-5 on terms of magnitude max|grad_out| / min|x| = 180.  A gather
form that takes the gradient as the difference of two such sums misses it (1.3e-5 / 2.1e-5 at R = 1 / 2; the general kernels
7.9e-6 / 1.4e-5); bwd_valid's projected cosine form cancels inside every pair and returns exact zeros."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err, same_nan_pattern

pytestmark = pytest.mark.gpu
TOL = 1e-5
TOL_BF16_OUT, TOL_BF16_GX = 1e-2, 2e-2

SHAPES = [
    (2, 8, 3, 3), (2, 8, 5, 5),                                    # one output (R = 1 / R = 2): every input but one a border pixel
    (1, 8, 3, 9), (1, 8, 9, 3),                                    # one output row, one output column
    (3, 8, 4, 4),                                                  # every pair has a border end
    (2, 16, 7, 6), (2, 8, 9, 10), (1, 12, 5, 13),                  # odd W, non-square
    (2, 1, 6, 6), (2, 3, 6, 7), (2, 6, 7, 7),                      # C of 1, odd, not a multiple of 4 (NCHW)
    (2, 512, 7, 7), (2, 192, 14, 14),                              # several channel chunks on a small map
    (2, 8, 24, 23), (1, 16, 41, 37), (1, 8, 130, 128),             # several row bands of unequal height, halo rows
    (1, 4, 6, 128),                                                # the widest served row
    (300, 8, 6, 6),                                                # more workgroups than CUs
]


def _radii(shape):
    return [R for R in (1, 2) if shape[2] >= 2 * R + 1 and shape[3] >= 2 * R + 1]


def _grid():
    out = []
    for s in SHAPES:
        for R in _radii(s):
            for meas in ("cosine", "norm"):
                out.append((s, R, meas, "f32", "nchw"))
                if s[1] % 8 == 0:
                    out += [(s, R, meas, "f32", "nhwc"), (s, R, meas, "bf16", "nchw"), (s, R, meas, "bf16", "nhwc")]
    return out


def _ctor(R, meas, sim=True):
    ctor = dict(R=R, measure=meas, padding=0, similarity=sim)
    if meas == "norm":
        ctor["p"] = 2
    return ctor


def _bf16_round(a):
    return torch.from_numpy(a).bfloat16().float().numpy()


def _inputs(shape, R, tweak=None, kind="normal"):
    from neighbour_feature_pooling_amd.synth import feature_map
    B, C, H, W = shape
    x = feature_map(shape, 5 * H + W + 3 * C + B, kind)
    if tweak == "zero_pixels":      # all-zero pixels: a corner, a border pixel, two interior ones next to each other
        for b, y, xx in ((0, 0, 0), (0, 3, 2), (0, 3, 3), (1, H - 1, 2), (1, 2, 2)):
            x[b, :, y, xx] = 0.0
    elif tweak == "identical":      # two identical adjacent interior pixels (distance 0), once along a row, once down a column
        x[0, :, 3, 3] = x[0, :, 3, 2]
        x[1, :, 4, 2] = x[1, :, 3, 2]
    go = feature_map((B, (2 * R + 1) ** 2 - 1, H - 2 * R, W - 2 * R), 3 * H + W + 1000)
    return x, go


@functools.lru_cache(maxsize=None)
def _reference(shape, R, meas, sim, bf16, tweak=None, kind="normal"):
    """(out, grad_x) of the oracle, computed once per case and shared by the layouts (bf16: on the rounded inputs)."""
    import oracle
    oracle.build()
    x, go = _inputs(shape, R, tweak, kind)
    if bf16:
        x, go = _bf16_round(x), _bf16_round(go)
    ctor = _ctor(R, meas, sim)
    return oracle.forward(x, **ctor), oracle.backward(x, go, **ctor)


def _config(C, R, meas, sim=True):
    from neighbour_feature_pooling_amd import NFPPooling
    return NFPPooling(C, **_ctor(R, meas, sim)).config


def _device_run(x, go, cfg, dtype, layout, strided=False, expect_valid=True):
    """(out, grad_x, forward variant, backward variant) of functional.nfp_valid on the device; with expect_valid the kernel
    family and the launch counts (one each way) are asserted."""
    from neighbour_feature_pooling_amd import _abi, nfp_valid
    dev = torch.device("cuda:0")
    L = _abi.load()
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    xt = torch.from_numpy(x).to(dev).to(tdt)
    if strided:     # a batch-strided view: the first C channels of a tensor with 2C
        assert layout == "nchw"
        xt = torch.cat([xt, xt + 1], dim=1)[:, :x.shape[1]]
        assert not xt.is_contiguous() or x.shape[0] == 1
    elif layout == "nhwc":
        xt = xt.contiguous(memory_format=torch.channels_last)
    xt = xt.detach().requires_grad_(True)
    got = torch.from_numpy(go).to(dev).to(tdt)
    n0 = L.nfp_launch_count()
    out = nfp_valid(xt, cfg)
    n1 = L.nfp_launch_count()
    fv = L.nfp_last_variant().decode()
    gx, = torch.autograd.grad(out, xt, got)
    torch.cuda.synchronize()
    n2 = L.nfp_launch_count()
    bv = L.nfp_last_variant().decode()
    if expect_valid:
        assert fv.startswith("fwd_valid<") and bv.startswith("bwd_valid<"), (fv, bv)
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


def _case(shape, R, meas, dtype, layout, sim=True, strided=False, tweak=None, kind="normal"):
    x, go = _inputs(shape, R, tweak, kind)
    ref_out, ref_gx = _reference(shape, R, meas, sim, dtype == "bf16", tweak, kind)
    out, gx, fv, bv = _device_run(x, go, _config(shape[1], R, meas, sim), dtype, layout, strided)
    assert f"<{R}," in fv and ("prod" if meas in ("cosine", "dot", "gfc") else "dist") in fv
    _check(out, gx, ref_out, ref_gx, dtype, f"{shape} R={R} {meas} {dtype} {layout} {fv} {bv}")


@pytest.mark.parametrize("shape,R,meas,dtype,layout", _grid(),
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_valid_kernels_match_the_oracle(shape, R, meas, dtype, layout):
    _case(shape, R, meas, dtype, layout)


@pytest.mark.parametrize("shape", [(2, 16, 7, 6), (2, 8, 24, 23)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("meas,sim", [("dot", True), ("gfc", True), ("rmse", True), ("dot", False), ("gfc", False), ("rmse", False),
                                      ("cosine", False), ("norm", False)])
@pytest.mark.parametrize("R", [1, 2])
def test_the_other_hot_measures_and_dissimilarity(shape, meas, sim, R):
    _case(shape, R, meas, "f32", "nchw", sim=sim)
    _case(shape, R, meas, "f32", "nhwc", sim=sim)


@pytest.mark.parametrize("shape", [(2, 16, 7, 6), (2, 8, 24, 23)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("meas,R", [("cosine", 1), ("norm", 2)])
def test_batch_strided_views_are_read_in_place(shape, dtype, meas, R):
    """xx[:, :C] of a tensor with 2C channels: images dense in NCHW order, a batch stride of 2C planes.  (The same slice of a
    channels-last tensor is not a dense image — its pixels lie 2C apart — and is not a view these kernels read in place.)"""
    _case(shape, R, meas, dtype, "nchw", strided=True)


@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_cosine_on_a_relu_input_with_all_zero_pixels(R, layout):
    _case((2, 16, 7, 6), R, "cosine", "f32", layout, tweak="zero_pixels", kind="relu")


@pytest.mark.parametrize("meas", ["rmse", "norm"])
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_distance_zero_follows_the_oracle(meas, R, layout):
    """Two identical adjacent interior pixels: Norm p = 2 takes gradient 0 there, rmse NaN on the two pixels of the pair and
    nowhere else — the oracle's pattern exactly (values compared after nan_to_num)."""
    shape = (2, 8, 24, 23)
    _case(shape, R, meas, "f32", layout, tweak="identical")
    ref_gx = _reference(shape, R, meas, True, False, "identical")[1]
    assert np.isnan(ref_gx).any() == (meas == "rmse")


def test_seeded_sweep_of_40_random_geometries():
    rng = np.random.RandomState(20240917)
    served = 0
    for _ in range(40):
        R = int(rng.randint(1, 3))
        B, C = int(rng.randint(1, 6)), int(rng.randint(1, 71))
        H, W = int(rng.randint(2 * R + 1, 41)), int(rng.randint(2 * R + 1, 41))
        meas = ["cosine", "dot", "gfc", "norm", "rmse"][int(rng.randint(0, 5))]
        sim = bool(rng.randint(0, 2))
        dtype = ["f32", "bf16"][int(rng.randint(0, 2))]
        nhwc_ok = C % (8 if dtype == "bf16" else 4) == 0
        layout = ["nchw", "nhwc"][int(rng.randint(0, 2))] if nhwc_ok else "nchw"
        _case((B, C, H, W), R, meas, dtype, layout, sim=sim)
        served += 1
    assert served == 40


@pytest.mark.parametrize("meas,R,dtype,layout", [("cosine", 1, "f32", "nchw"), ("norm", 2, "f32", "nhwc"), ("gfc", 2, "bf16", "nchw"),
                                                 ("rmse", 1, "bf16", "nhwc")])
def test_two_runs_agree_bitwise_and_an_image_does_not_depend_on_the_batch(meas, R, dtype, layout):
    shape = (5, 16, 24, 23)
    x, go = _inputs(shape, R)
    cfg = _config(shape[1], R, meas)
    a = _device_run(x, go, cfg, dtype, layout)
    b = _device_run(x, go, cfg, dtype, layout)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    one = _device_run(x[:1].copy(), go[:1].copy(), cfg, dtype, layout)
    assert np.array_equal(a[0][:1], one[0]) and np.array_equal(a[1][:1], one[1])


def test_an_empty_batch_launches_nothing():
    from neighbour_feature_pooling_amd import _abi, nfp_valid
    L = _abi.load()
    x = torch.zeros(0, 8, 6, 6, device="cuda:0", requires_grad=True)
    n0 = L.nfp_launch_count()
    out = nfp_valid(x, _config(8, 1, "cosine"))
    assert tuple(out.shape) == (0, 8, 4, 4) and out.dtype == torch.float32
    gx, = torch.autograd.grad(out, x, torch.zeros_like(out))
    assert tuple(gx.shape) == (0, 8, 6, 6)
    assert L.nfp_launch_count() == n0


def test_a_refused_row_width_falls_to_the_general_kernels():
    shape, R = (1, 8, 7, 300), 1
    x, go = _inputs(shape, R)
    ref_out, ref_gx = _reference(shape, R, "cosine", True, False)
    out, gx, fv, bv = _device_run(x, go, _config(8, R, "cosine"), "f32", "nchw", expect_valid=False)
    assert not fv.startswith("fwd_valid") and not bv.startswith("bwd_valid"), (fv, bv)
    _check(out, gx, ref_out, ref_gx, "f32", f"W = 300: {fv} {bv}")


def test_the_switch_routes_to_the_general_kernels(monkeypatch):
    shape, R = (2, 16, 7, 6), 1
    x, go = _inputs(shape, R)
    ref_out, ref_gx = _reference(shape, R, "cosine", True, False)
    cfg = _config(16, R, "cosine")
    monkeypatch.setenv("NFP_VALID_OFF", "1")
    out, gx, fv, bv = _device_run(x, go, cfg, "f32", "nchw", expect_valid=False)
    assert not fv.startswith("fwd_valid") and not bv.startswith("bwd_valid"), (fv, bv)
    _check(out, gx, ref_out, ref_gx, "f32", f"NFP_VALID_OFF=1: {fv} {bv}")
    monkeypatch.delenv("NFP_VALID_OFF")
    out, gx, fv, bv = _device_run(x, go, cfg, "f32", "nchw")
    _check(out, gx, ref_out, ref_gx, "f32", f"switch unset: {fv} {bv}")
