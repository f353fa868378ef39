"""NFPPooling(bias=True) at the sizes and layouts its kernels (csrc/nfp_bias.hip) run at, against the float64 torch
formulation on the device: the bench shapes, every neighbours-per-workgroup count of bias_fwd (NB, read from the forward's
variant bias_fwd<M,layout>x<NB>), N > 256 neighbours, several channel passes per lane, grids past flat_blocks' cap,
views, grad_out forms, empty and oversized batches, the dtype policy, the ABI's saved = NULL, determinism, the unbiased
kernels as a second opinion, and Pearson's pivot.  Inputs and biases sit on the grid of scripts/stress_bias.py::exact
(every sum the kernels form is exact: signs and ties agree with float64)."""
import ctypes
import importlib.util
import os
import random
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

# (shape, NFPPooling kwargs, dtype, channels-last, NB of bias_fwd): scripts/bench_bias.py
BENCH = [((64, 512, 7, 7), dict(R=1, measure="cosine", padding=1), torch.float32, False, 1),
         ((256, 64, 56, 56), dict(R=1, measure="Norm", p=1, padding=1), torch.float32, False, 8),
         ((256, 192, 14, 14), dict(R=2, measure="norm", p=2, padding=2), torch.bfloat16, True, 24)]
BENCH_IDS = ["cosine_64x512x7x7", "Norm1_256x64x56x56", "L2k5_bf16_nhwc_256x192x14x14"]
_SB = None


def sb():
    """scripts/stress_bias.py: the float64 reference, the comparison and the random draws."""
    global _SB
    if _SB is None:
        spec = importlib.util.spec_from_file_location(
            "stress_bias", os.path.join(os.path.dirname(__file__), "..", "scripts", "stress_bias.py"))
        _SB = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_SB)
    return _SB


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from neighbour_feature_pooling_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _free_memory():
    yield
    torch.cuda.empty_cache()


def _lib():
    from neighbour_feature_pooling_amd import _abi
    return _abi.load()


def _layer(dev, C, ctor, seed=0, zero=False):
    from neighbour_feature_pooling_amd import NFPPooling
    torch.manual_seed(seed)
    m = NFPPooling(C, bias=True, **ctor).to(dev)
    if zero:
        with torch.no_grad():
            m.center_value.bias.zero_()
            m.comp_neighbors.bias.zero_()
        return m
    return sb().quantize_biases(m)


def _oshape(shape, ctor):
    B, C, H, W = shape
    R, pad, s, d = ctor["R"], ctor.get("padding", 0), ctor.get("stride", 1), ctor.get("dilation", 1)
    span = d * 2 * R + 1
    return B, (2 * R + 1) ** 2 - 1, (H + 2 * pad - span) // s + 1, (W + 2 * pad - span) // s + 1


def _data(dev, shape, ctor, dtype=torch.float32, seed=0, normal=False):
    """(x, go): x on the exact grid (uniform(0.25, 1.25), or standard normal), go standard normal, both in dtype."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(shape, generator=g, device=dev) if normal else torch.rand(shape, generator=g, device=dev) + 0.25
    go = torch.randn(_oshape(shape, ctor), generator=g, device=dev)
    return sb().exact(x).to(dtype), go.to(dtype)


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _check64(m, xr, x, go, what=""):
    """Run the layer on xr (x's values in some layout), compare with float64 on x; the forward and backward variants."""
    S = sb()
    got = S.run(m, xr, go)
    ok, errs = S.compare(got, S.ref64(m, x, go), x.dtype == torch.bfloat16, m.measure.lower() in S.LOOSE)
    assert ok, (what, ["%.2e" % e for e in errs], got[4])
    assert got[5].startswith("bias_bwd<"), got[5]
    return got[4], got[5]


def _nb(fv):
    return sb().fwd_nb(fv)


# ---- 1. the bench shapes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(3), ids=BENCH_IDS)
def test_bench_shapes_against_float64(i, dev):
    shape, ctor, dt, cl, nb = BENCH[i]
    m = _layer(dev, shape[1], ctor, seed=i)
    x, go = _data(dev, shape, ctor, dt, seed=i, normal=True)
    fv, bv = _check64(m, _cl(x) if cl else x, x, go, BENCH_IDS[i])
    assert _nb(fv) == ("nhwc" if cl else "nchw", nb), fv   # (the NB heuristic of nfp_bias.hip::bias_forward)
    assert bv.startswith("bias_bwd<") and bv.split(">")[0].endswith("nhwc" if cl else "nchw"), bv


# ---- 2. batch independence --------------------------------------------------------------------------------------------
def _images_match_single_calls(m, x, go, images, cl, single_nb=None):
    """out[b] and grad_x[b] of the batch bitwise against B = 1 calls on x[b:b+1] (whose forward runs single_nb neighbours
    per workgroup, when given); returns the batch's forward variant, its bias gradients and the single calls'."""
    S = sb()
    got = S.run(m, _cl(x) if cl else x, go)
    out, gx, gbc, gnb, fv = got[0], got[1], got[2], got[3], got[4]
    singles = {}
    for b in images:
        one = S.run(m, _cl(x[b:b + 1]) if cl else x[b:b + 1], go[b:b + 1])
        assert single_nb is None or _nb(one[4])[1] == single_nb, one[4]
        assert torch.equal(out[b], one[0][0]), (b, fv, one[4])
        assert torch.equal(gx[b], one[1][0]), (b, fv, one[4])
        singles[b] = (None if one[2] is None else one[2].double(), one[3].double())
    return fv, gbc, gnb, singles


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
def test_batch_independence_bitwise(cl, dt, dev):
    """Each pair's channel sum and each pixel's gather run in an order that depends on neither NB nor B: an image of a
    batch whose forward runs NB > 1 neighbours per workgroup gives the bits of a B = 1 call (NB = 1); the batch's bias
    gradients are the sum of the images'."""
    shape = (64, 16, 32, 32)
    ctor = dict(R=1, measure="cosine", padding=1)
    m = _layer(dev, 16, ctor, seed=21)
    x, go = _data(dev, shape, ctor, dt, seed=22)
    B = shape[0]
    fv, gbc, gnb, singles = _images_match_single_calls(m, x, go, range(B), cl, single_nb=1)
    assert _nb(fv)[1] > 1, fv
    S = sb()
    assert S.rel(gnb, sum(singles[b][1] for b in range(B))) <= 1e-6
    assert S.rel(gbc, sum(singles[b][0] for b in range(B))) <= 1e-6


# ---- 3. past flat_blocks' cap of 2^20 workgroups (the grid-stride loops of bias_coef and bias_gx) -----------------------
@pytest.mark.parametrize("case", ["pairs", "elements"])
def test_grid_stride_loops_beyond_the_flat_grid_cap(case, dev):
    """More than 2^28 (output, neighbour) pairs (bias_coef) / input elements (bias_gx): images of the big batch bitwise
    against B = 1 calls, which run one pass of the grid."""
    if case == "pairs":   # 300 * 288 * 64 * 64 = 3.5e8 pairs
        shape, ctor, cl = (300, 16, 64, 64), dict(R=8, measure="cosine", padding=8), False
        B, N, Ho, Wo = _oshape(shape, ctor)
        assert B * N * Ho * Wo > 1 << 28
    else:                 # 1100 * 256 * 32 * 32 = 2.9e8 elements
        shape, ctor, cl = (1100, 256, 32, 32), dict(R=1, measure="norm", p=2, padding=1), True
        assert shape[0] * shape[1] * shape[2] * shape[3] > 1 << 28
    m = _layer(dev, shape[1], ctor, seed=31)
    x, go = _data(dev, shape, ctor, seed=32)
    fv, _, _, _ = _images_match_single_calls(m, x, go, (0, shape[0] // 2, shape[0] - 1), cl)
    assert _nb(fv)[0] == ("nhwc" if cl else "nchw"), fv


# ---- 4. neighbour counts -------------------------------------------------------------------------------------------
NEIGHBOURS = [  # (id, shape, ctor)
    ("R3_stride2", (6, 8, 30, 30), dict(R=3, measure="gfc", padding=3, stride=2, padding_mode="zeros")),
    ("R3_dil2", (3, 5, 20, 22), dict(R=3, measure="canberra", padding=4, dilation=2, padding_mode="replicate")),
    ("R4_partial_nchw", (25, 6, 20, 20), dict(R=4, measure="cosine", padding=4)),       # NB = 3 of 80
    ("R4_partial_nhwc", (8, 6, 10, 10), dict(R=4, measure="norm", p=2, padding=4)),     # NB = 3 of 80
    ("R8", (2, 6, 20, 20), dict(R=8, measure="cosine", padding=8)),                     # N = 288: two bias_part chunks
    ("R8_zeros_dil2", (2, 6, 20, 20), dict(R=8, measure="pearson", padding=8, dilation=2, padding_mode="zeros")),
]


@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name,shape,ctor", NEIGHBOURS, ids=[c[0] for c in NEIGHBOURS])
def test_neighbour_counts_against_float64(name, shape, ctor, cl, dev):
    m = _layer(dev, shape[1], ctor, seed=41)
    x, go = _data(dev, shape, ctor, seed=42)
    fv, _ = _check64(m, _cl(x) if cl else x, x, go, name)
    N = _oshape(shape, ctor)[1]
    lay, nb = _nb(fv)
    assert lay == ("nhwc" if cl else "nchw"), fv
    if name == "R4_partial_" + lay:
        assert N == 80 and nb == 3 and N % nb != 0, fv
    if name.startswith("R8"):
        assert N == 288, N


# ---- 5. channel passes -----------------------------------------------------------------------------------------------
CHANNEL_CASES = [  # (C, layout, measure, batch at NB = 1, batch at NB > 1, map side)
    (65, "nhwc", "chisquared2", 2, 64, 12), (130, "nhwc", "cosine", 2, 64, 12), (512, "nhwc", "pearson", 2, 64, 12),
    (3, "nchw", "geman", 2, 256, 16), (257, "nchw", "rmse", 2, 256, 16)]


@pytest.mark.parametrize("many", [False, True], ids=["NB1", "NBgt1"])
@pytest.mark.parametrize("C,layout,measure,b1,bn,hw", CHANNEL_CASES, ids=[f"{c[1]}_C{c[0]}" for c in CHANNEL_CASES])
def test_channel_passes_against_float64(C, layout, measure, b1, bn, hw, many, dev):
    """Channels-last: C > 64 gives each lane several channels before wave_sum; NCHW: C = 3 leaves most of the 4 channel
    groups idle, C = 257 ends on a partial pass."""
    ctor = dict(R=1, measure=measure, padding=1)
    shape = (bn if many else b1, C, hw, hw)
    m = _layer(dev, C, ctor, seed=51)
    x, go = _data(dev, shape, ctor, seed=52)
    fv, _ = _check64(m, _cl(x) if layout == "nhwc" else x, x, go, (C, layout))
    lay, nb = _nb(fv)
    assert lay == layout and (nb > 1) == many, fv


# ---- 6. the random stress -----------------------------------------------------------------------------------------------
def test_random_stress_of_the_biased_kernels(dev):
    """40 draws of scripts/stress_bias.py (the long form: python scripts/stress_bias.py 400 1).  The seed is one whose
    draws reach, in both layouts, NB = 1, 1 < NB < N, NB = N and N % NB != 0 — as the forwards' variants report."""
    S = sb()
    rnd = random.Random(3466)
    seen = set()
    for _ in range(40):
        ok, desc, errs, vs = S.one_case(rnd, dev)
        assert ok, (desc, ["%.2e" % e for e in errs], vs)
        lay, kind, partial = S.coverage(vs[0], desc)
        seen.add((lay, kind))
        if partial:
            seen.add((lay, "N%NB"))
        torch.cuda.empty_cache()
    want = {(lay, k) for lay in ("nchw", "nhwc") for k in ("NB=1", "1<NB<N", "NB=N", "N%NB")}
    assert want <= seen, sorted(want - seen)


# ---- 7. views and grad_out forms ------------------------------------------------------------------------------------------
def test_batch_strided_view_is_read_in_place(dev):
    S = sb()
    ctor = dict(R=1, measure="cosine", padding=1)
    m = _layer(dev, 24, ctor, seed=71)
    x, go = _data(dev, (5, 24, 9, 11), ctor, seed=72)
    v = S.batch_strided(x)
    assert v.stride(0) > 24 * 9 * 11
    fv, bv = _check64(m, v, x, go, "batch-strided")
    assert _nb(fv)[0] == "nhwc" and "nhwc" in bv, (fv, bv)


@pytest.mark.parametrize("view", ["rows", "channels"])
def test_non_dense_views_match_their_copies_bitwise(view, dev):
    S = sb()
    ctor = dict(R=1, measure="gfc", padding=1)
    g = torch.Generator(device=dev).manual_seed(73)
    big = S.exact(torch.rand(4, 20, 18, 9, generator=g, device=dev) + 0.25)
    v = big[:, :, ::2] if view == "rows" else big[:, 3:15]
    C = v.shape[1]
    m = _layer(dev, C, ctor, seed=74)
    go = torch.randn(_oshape(tuple(v.shape), ctor), generator=g, device=dev)
    a, b = S.run(m, v, go), S.run(m, v.contiguous(), go)
    for u, w in zip(a[:4], b[:4]):
        assert torch.equal(u, w)


def test_grad_out_forms_match_a_dense_grad_out(dev):
    """channels-last, expanded (the gradient of out.sum()) and other-dtype grad_out: through the module and straight into
    functional.bias_backward_call, bitwise against a dense float32 grad_out of the same values."""
    from neighbour_feature_pooling_amd import functional
    S = sb()
    ctor = dict(R=1, measure="cosine", padding=1)
    m = _layer(dev, 12, ctor, seed=75)
    x, go = _data(dev, (3, 12, 8, 8), ctor, seed=76)
    ref = S.run(m, x, go)
    for form in (_cl(go), go.double()):
        got = S.run(m, x, form)
        for u, w in zip(ref[:4], got[:4]):
            assert torch.equal(u, w)
    ones = S.run(m, x, torch.ones_like(go))
    m.zero_grad(set_to_none=True)
    xs = x.detach().requires_grad_(True)
    m(xs).sum().backward()
    for u, w in zip(ones[1:4], (xs.grad, m.center_value.bias.grad, m.comp_neighbors.bias.grad)):
        assert torch.equal(u, w)
    cb, nb = m.center_value.bias.detach(), m.comp_neighbors.bias.detach()
    out, saved = functional.bias_forward_call(x, cb, nb, m.config)
    expanded = go[:1].expand_as(go)
    for form, dense in ((_cl(go), go), (go.double(), go), (expanded, expanded.contiguous())):
        want = functional.bias_backward_call(x, cb, nb, out, saved, dense, m.config)
        got = functional.bias_backward_call(x, cb, nb, out, saved, form, m.config)
        for u, w in zip(want, got):
            assert torch.equal(u, w)


# ---- 8. edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["cosine", "attention"])
def test_empty_batch_gives_empty_maps_and_zero_bias_gradients(measure, dev):
    """Regression: torch hands a zero-element tensor over as a NULL pointer, and nfp_bias_forward / nfp_bias_backward
    refused those as null tensors — an empty batch raised instead of giving empty maps and zero bias gradients."""
    m = _layer(dev, 8, dict(R=1, measure=measure, padding=1), seed=81)
    x = torch.zeros(0, 8, 6, 7, device=dev, requires_grad=True)
    n0 = _lib().nfp_launch_count()
    out = m(x)
    assert tuple(out.shape) == (0, 8, 6, 7) and out.dtype == x.dtype
    out.backward(torch.zeros_like(out))
    torch.cuda.synchronize()
    assert tuple(x.grad.shape) == (0, 8, 6, 7)
    for p in (m.center_value.bias, m.comp_neighbors.bias):
        assert p.grad is not None and torch.equal(p.grad, torch.zeros_like(p))
    assert _lib().nfp_launch_count() > n0   # (bias_reduce wrote the zeros)


def test_batch_beyond_65535_is_refused_before_any_launch(dev):
    from neighbour_feature_pooling_amd import _abi
    m = _layer(dev, 1, dict(R=1, measure="cosine", padding=1), seed=82)
    x = torch.rand(65536, 1, 3, 3, device=dev)
    torch.cuda.synchronize()
    n0 = _lib().nfp_launch_count()
    with pytest.raises(_abi.NfpUnsupported):
        m(x)
    assert _lib().nfp_launch_count() == n0


@pytest.mark.parametrize("measure", ["cosine", "norm", "smith"])
def test_zero_padding_wider_than_the_kernel_sees_only_biases(measure, dev):
    """pad > R * dilation with zero padding: the border outputs' taps are all padding, i.e. the biases alone."""
    ctor = dict(R=1, measure=measure, padding=3, padding_mode="zeros", dilation=1)
    if measure == "norm":
        ctor["p"] = 2
    m = _layer(dev, 8, ctor, seed=83)
    x, go = _data(dev, (3, 8, 6, 7), ctor, seed=84)
    for xr in (x, _cl(x)):
        _check64(m, xr, x, go, measure)


# ---- 9. dtype policy -----------------------------------------------------------------------------------------------------
DTYPE_CASES = ["float16", "autocast", "float64", "module_double", "module_bfloat16"]


@pytest.mark.parametrize("case", DTYPE_CASES)
def test_dtype_policy_follows_the_unbiased_path(case, dev):
    """Output and grad_x in the types the unbiased path gives for the same input and context (functional._amp_input), each
    bias gradient in its bias's type; values against float64 at the bar of the storage type."""
    import contextlib
    from neighbour_feature_pooling_amd import NFPPooling, functional
    S = sb()
    ctor = dict(R=1, measure="cosine", padding=1)
    x32, go32 = _data(dev, (2, 16, 9, 9), ctor, seed=91)
    m = _layer(dev, 16, ctor, seed=92)
    plain = NFPPooling(16, **ctor).to(dev)
    xdt = {"float16": torch.float16, "autocast": torch.float32, "float64": torch.float64, "module_double": torch.float64,
           "module_bfloat16": torch.bfloat16}[case]
    if case == "module_double":
        m, plain = m.double(), plain.double()
    if case == "module_bfloat16":
        m, plain = m.bfloat16(), plain.bfloat16()
    x = x32.to(xdt)
    ctx = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if case == "autocast" else contextlib.nullcontext

    def run(layer):
        xs = x.detach().requires_grad_(True)
        with ctx():
            out = layer(xs)
        out.backward(go32.to(out.dtype))
        return out.detach(), xs.grad

    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        functional._WARNED_F64 = False
        m.zero_grad(set_to_none=True)
        out, gx = run(m)
        run(m)
        p_out, p_gx = run(plain)
    f64 = [x for x in w if "float64" in str(x.message)]
    assert len(f64) == (1 if xdt == torch.float64 else 0), [str(x.message) for x in w]
    assert out.dtype == p_out.dtype and gx.dtype == p_gx.dtype == x.dtype, (out.dtype, p_out.dtype, gx.dtype, p_gx.dtype)
    for p in (m.center_value.bias, m.comp_neighbors.bias):
        assert p.grad.dtype == p.dtype
    go = go32.to(out.dtype)
    with ctx():
        got = S.run(m, x, go)
    want = S.ref64(m, x, go)
    bar = {torch.float16: (1e-3, 1e-3), torch.bfloat16: (1e-2, 2e-2)}.get(x.dtype, (1e-4, 1e-4))
    eo, eg = S.rel(got[0], want[0]), S.rel(got[1], want[1])
    ec, en = S.rel(got[2], want[2]), S.rel(got[3], want[3])
    assert eo <= bar[0] and max(eg, ec, en) <= bar[1], (case, eo, eg, ec, en)


# ---- 10. the ABI ---------------------------------------------------------------------------------------------------------
def _abi_call(dev, measure):
    from neighbour_feature_pooling_amd import functional
    from neighbour_feature_pooling_amd.functional import NfpConfig
    cfg = NfpConfig(R=1, measure=measure, padding=1, diff_weights=False)
    g = torch.Generator(device=dev).manual_seed(101)
    x = torch.rand(4, 16, 12, 12, generator=g, device=dev)
    plan = functional._plan(x, "nchw", cfg, tables=False)
    d, oshape, ns = plan.desc, plan.oshape, plan.ask("nfp_bias_saved_floats")
    bc, nb = torch.randn(16, generator=g, device=dev), torch.randn(128, generator=g, device=dev)
    stream = functional._raw_stream(x.device)

    def fwd(saved, n):
        out = torch.full(oshape, float("nan"), device=dev)
        rc = _lib().nfp_bias_forward(ctypes.byref(d), x.data_ptr(), bc.data_ptr(), nb.data_ptr(), out.data_ptr(),
                                     None if saved is None else saved.data_ptr(), n, stream)
        return rc, out

    return fwd, ns


def test_forward_without_saved_state_writes_the_same_maps(dev):
    fwd, ns = _abi_call(dev, "cosine")
    saved = torch.empty(ns, device=dev)
    rc1, a = fwd(saved, ns)
    rc2, b = fwd(None, 0)
    torch.cuda.synchronize()
    assert rc1 == 0 and rc2 == 0
    assert torch.equal(a, b)


def test_attention_forward_without_saved_state_is_refused_before_any_launch(dev):
    fwd, ns = _abi_call(dev, "attention")
    assert ns > 0
    torch.cuda.synchronize()
    n0 = _lib().nfp_launch_count()
    rc, _ = fwd(None, 0)
    assert rc == -1 and b"saved" in _lib().nfp_last_error()
    assert _lib().nfp_launch_count() == n0


# ---- 11. determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [1, 2], ids=BENCH_IDS[1:])
def test_bench_shapes_with_several_neighbours_per_workgroup_are_bitwise_reproducible(i, dev):
    shape, ctor, dt, cl, nb = BENCH[i]
    m = _layer(dev, shape[1], ctor, seed=i)
    x, go = _data(dev, shape, ctor, dt, seed=i, normal=True)
    xr = _cl(x) if cl else x
    a = sb().run(m, xr, go)
    assert _nb(a[4])[1] == nb > 1, a[4]
    b = sb().run(m, xr, go)
    assert a[2] is None and b[2] is None   # (Norm: no centre bias gradient)
    for u, v in zip(a[:4], b[:4]):
        assert u is None or torch.equal(u, v)


# ---- 12. the unbiased kernels as a second opinion ------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(3), ids=BENCH_IDS)
def test_zero_biases_match_the_unbiased_hot_path(i, dev):
    """The two kernel families share only nfp_measures.h: with both biases zero they compute the same maps."""
    from neighbour_feature_pooling_amd import NFPPooling
    shape, ctor, dt, cl, nb = BENCH[i]
    S = sb()
    m = _layer(dev, shape[1], ctor, seed=i, zero=True)
    x, go = _data(dev, shape, ctor, dt, seed=i, normal=True)
    xr = _cl(x) if cl else x
    biased = S.run(m, xr, go)
    assert biased[4].startswith("bias_fwd<"), biased[4]
    plain = NFPPooling(shape[1], **ctor).to(dev)
    xs = xr.detach().requires_grad_(True)
    out = plain(xs)
    assert not _lib().nfp_last_variant().decode().startswith("bias_")
    out.backward(go)
    to, tg = (1e-2, 2e-2) if dt == torch.bfloat16 else (1e-5, 1e-5)
    assert S.rel(biased[0], out.detach()) <= to
    assert S.rel(biased[1], xs.grad) <= tg


# ---- 13. Pearson's pivot -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
def test_pearson_pivot_with_biases_on_offset_data(cl, dev):
    """Pearson's channel sums are taken about the pair's channel-0 value (nfp_measures.h::Pivot), which in the biased kernels
    includes the biases (pa, pb; saved = save0 + pa): on data with a large common offset the biased kernels' error against
    float64 is to be no worse than twice the unbiased kernels' on the same data (or 5e-4, the LOOSE bar)."""
    from neighbour_feature_pooling_amd import NFPPooling
    from neighbour_feature_pooling_amd._host import nfp_host
    S = sb()
    ctor = dict(R=1, measure="pearson", padding=1)
    shape = (4, 512, 10, 10)
    g = torch.Generator(device=dev).manual_seed(131)
    x = torch.randn(shape, generator=g, device=dev) + 50
    go = torch.randn(_oshape(shape, ctor), generator=g, device=dev)
    xr = _cl(x) if cl else x
    m = _layer(dev, 512, ctor, seed=132)
    got, want = S.run(m, xr, go), S.ref64(m, x, go)
    plain = NFPPooling(512, **ctor).to(dev)
    xs = xr.detach().requires_grad_(True)
    out = plain(xs)
    out.backward(go)
    x64 = x.double().requires_grad_(True)
    ref = nfp_host(x64, plain.config)
    ref.backward(go.double())
    eu_o, eu_g = S.rel(out.detach(), ref.detach()), S.rel(xs.grad, x64.grad)
    eb_o, eb_g, eb_n = S.rel(got[0], want[0]), S.rel(got[1], want[1]), S.rel(got[3], want[3])
    errs = dict(unbiased=(eu_o, eu_g), biased=(eb_o, eb_g, eb_n))
    assert eb_o <= max(5e-4, 2 * eu_o), errs
    assert eb_g <= max(5e-4, 2 * eu_g), errs
    assert eb_n <= max(5e-4, 2 * eu_g), errs
