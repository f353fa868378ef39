"""nfp_desc.map_f32 — bf16 x / grad_x with float32 out / grad_out, the call torch.autocast makes — checked WITHOUT a GPU
through nfp_plan (include/nfp.h): which kernels serve it, what is refused, and that map_f32 = 0 plans what it always did."""
import ctypes

import pytest

from neighbour_feature_pooling_amd import _abi
from test_dispatch_plan import desc, plan


@pytest.fixture(scope="module")
def lib():
    from neighbour_feature_pooling_amd.build import build_hip
    build_hip()
    return _abi.load()


def mixed(shape, **kw):
    d = desc(shape, dtype=_abi.BF16, **kw)
    d.map_f32 = 1
    return d


# the issue's benchmark shapes that the hot-path kernels serve: (descriptor kwargs, forward, backward)
HOT = [
    (dict(shape=(64, 512, 7, 7)), "fwd_band<R1,cos,mix,nchw>x4", "bwd_fast<R1,cos,mix,nchw>"),
    (dict(shape=(256, 512, 7, 7), channels_last=True), "fwd_band<R1,cos,mix,nhwc>x1", "bwd_fast<R1,cos,mix,nhwc>"),
    (dict(shape=(256, 192, 14, 14), R=2, measure="norm", channels_last=True), "fwd_band<R2,l2,mix,nhwc>x", "bwd_fast<R2,l2,mix,nhwc>"),
    (dict(shape=(256, 64, 56, 56)), "fwd_tile<R1,cos,mix,nchw>x", "bwd_tile<R1,cos,mix,nchw>x"),
    (dict(shape=(256, 64, 56, 56), channels_last=True), "fwd_tile<R1,cos,mix,nhwc>x", "bwd_tile<R1,cos,mix,nhwc"),
]
# mixed descriptors the any-geometry kernels serve
GENERAL = [
    dict(shape=(256, 64, 28, 28), pad=0),                       # the reference's default nfp_kwargs
    dict(shape=(2, 8, 9, 9), stride=2),
    dict(shape=(2, 8, 9, 9), mode="circular"),
    dict(shape=(2, 6, 7, 7)),                                   # C % 4 != 0
    dict(shape=(2, 8, 7, 7), measure="canberra"),
    dict(shape=(2, 8, 7, 7), measure="norm", p=1.0),
]


@pytest.mark.parametrize("kw,fwd,bwd", HOT)
def test_hot_path_kernels_serve_the_bench_shapes(lib, kw, fwd, bwd):
    rc, text = plan(lib, mixed(**kw), False)
    assert rc == 0 and text.startswith(fwd), text
    assert "fwd_gram" not in text and "mfma" not in text and ",dma" not in text
    rc, text = plan(lib, mixed(**kw), True)
    assert rc == 0 and text.startswith(bwd), text
    assert "mfma" not in text


def test_dense_store_backward_and_riders(lib):
    rc, text = plan(lib, mixed((1, 128, 24, 24), channels_last=True), True)
    assert rc == 0 and text.startswith("bwd_tile<R1,cos,mix,nhwc,dense>x"), text
    rc, text = plan(lib, mixed((2, 64, 24, 24), channels_last=True), False)      # the bf16 LDS-DMA class: register staging here
    assert rc == 0 and text.startswith("fwd_tile<R1,cos,mix,nhwc>x"), text
    for measure, tag in (("dot", "dot"), ("gfc", "gfc"), ("rmse", "rmse")):
        for shape, fk, bk in (((2, 16, 6, 6), "fwd_band", "bwd_fast"), ((2, 8, 24, 23), "fwd_tile", "bwd_tile")):
            for back, kern in ((False, fk), (True, bk)):
                rc, text = plan(lib, mixed(shape, measure=measure), back)
                assert rc == 0 and text.startswith(f"{kern}<R1,{tag},mix,nchw>"), text


@pytest.mark.parametrize("kw", GENERAL)
def test_general_kernels_serve_the_rest(lib, kw):
    rc, text = plan(lib, mixed(**kw), False)
    assert rc == 0 and text.startswith("fwd_pairs |"), text
    rc, text = plan(lib, mixed(**kw), True)
    assert rc == 0 and text.startswith("bwd_gather |"), text


def test_wide_rows_go_where_the_bf16_descriptor_goes(lib):
    """Rows too wide for a row band (above 512 pixels, (W + 2R)(3R + 1) > 1024): the any-geometry kernels, the same ones that
    serve the descriptor with bf16 maps."""
    for back, allowed in ((False, ("fwd_pairs", "fwd_direct")), (True, ("bwd_gather", "bwd_gather_banded", "bwd_direct"))):
        rc, text = plan(lib, mixed((1, 8, 4, 300)), back)
        rc_b, text_b = plan(lib, desc((1, 8, 4, 300), dtype=_abi.BF16), back)
        assert rc == rc_b == 0 and text == text_b and text.split(" |")[0] in allowed, (text, text_b)


def test_no_mixed_plan_names_the_matrix_cores(lib):
    for C in (16, 32, 64, 512):
        for shape in ((64, C, 7, 7), (256, C, 14, 14), (4, C, 16, 16), (2, C, 24, 24)):
            for R, measure in ((1, "cosine"), (2, "norm"), (2, "cosine"), (1, "norm")):
                for cl in (False, True):
                    for back in (False, True):
                        rc, text = plan(lib, mixed(shape, R=R, measure=measure, channels_last=cl), back)
                        assert rc == 0 and ",mix," in text and "fwd_gram" not in text and "mfma" not in text, text


def test_refusals(lib):
    buf = ctypes.create_string_buffer(1024)

    def rc_of(d, back=0):
        return lib.nfp_plan(ctypes.byref(d), back, buf, len(buf))

    d = desc((2, 8, 7, 7), dtype=_abi.F32)
    d.map_f32 = 1
    assert rc_of(d) == -1 and rc_of(d, 1) == -1                       # NFP_E_INVALID: float32 storage
    for v in (2, -1, 7):
        d = mixed((2, 8, 7, 7))
        d.map_f32 = v
        assert rc_of(d) == -1 and rc_of(d, 1) == -1
        assert lib.nfp_saved_floats(ctypes.byref(d)) == -1
    d = mixed((2, 8, 7, 7), R=2)
    d.inner_R = 1
    assert rc_of(d) == -2 and rc_of(d, 1) == -2                       # NFP_E_UNSUPPORTED
    for measure in ("attention", "scs"):
        d = mixed((2, 8, 7, 7), measure=measure)
        assert rc_of(d) == -2 and rc_of(d, 1) == -2
    d = mixed((2, 8, 7, 7))
    assert lib.nfp_bias_saved_floats(ctypes.byref(d)) == -1 and lib.nfp_bias_scratch_floats(ctypes.byref(d)) == -1
    rc = lib.nfp_bias_forward(ctypes.byref(d), None, None, None, None, None, 0, None)
    assert rc == -2 and b"map_f32" in lib.nfp_last_error()
    rc = lib.nfp_bias_backward(ctypes.byref(d), None, None, None, None, None, None, 0, None, None, None, None, 0, None)
    assert rc == -2


@pytest.mark.parametrize("kw", [h[0] for h in HOT] + GENERAL)
def test_saved_floats_and_fused_callers(lib, kw):
    m, b = mixed(**kw), desc(dtype=_abi.BF16, **kw)
    assert lib.nfp_saved_floats(ctypes.byref(m)) == lib.nfp_saved_floats(ctypes.byref(b)) >= 0
    assert lib.nfp_workspace_bytes(ctypes.byref(m)) == lib.nfp_workspace_bytes(ctypes.byref(b))
    assert lib.nfp_pool_supported(ctypes.byref(m)) == 0 and lib.nfp_gap_supported(ctypes.byref(m)) == 0
    o = [(ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()) for _ in range(2)]
    for d, (n, ho, wo) in zip((m, b), o):
        assert lib.nfp_output_shape(ctypes.byref(d), ctypes.byref(n), ctypes.byref(ho), ctypes.byref(wo)) == 0
    assert [v.value for v in o[0]] == [v.value for v in o[1]]


# what these descriptors plan with map_f32 = 0 — recorded from the commit before the field existed
UNCHANGED = [
    (dict(shape=(64, 512, 7, 7)), "fwd_gram<R1,cos,bf16,nchw>", "bwd_fast<R1,cos,bf16,nchw,mfma>"),
    (dict(shape=(256, 512, 7, 7), channels_last=True), "fwd_gram<R1,cos,bf16,nhwc>", None),
    (dict(shape=(256, 192, 14, 14), R=2, measure="norm", channels_last=True), "fwd_gram<R2,l2,bf16,nhwc>",
     "bwd_fast<R2,l2,bf16,nhwc,mfma2>"),
    (dict(shape=(256, 200, 14, 14), R=2, measure="norm"), "fwd_band<R2,l2,bf16,nchw>x1", "bwd_fast<R2,l2,bf16,nchw>"),
    (dict(shape=(256, 64, 56, 56)), "fwd_tile<R1,cos,bf16,nchw>x", "bwd_tile<R1,cos,bf16,nchw>x"),
    (dict(shape=(256, 64, 56, 56), channels_last=True), "fwd_tile<R1,cos,bf16,nhwc,dma>x", "bwd_tile<R1,cos,bf16,nhwc,dense>x"),
    (dict(shape=(256, 64, 28, 28), pad=0), "fwd_pairs", "bwd_gather"),
]


@pytest.mark.parametrize("kw,fwd,bwd", UNCHANGED)
def test_map_f32_zero_plans_what_it_did(lib, kw, fwd, bwd):
    d = desc(dtype=_abi.BF16, **kw)
    assert d.map_f32 == 0
    rc, text = plan(lib, d, False)
    assert rc == 0 and text.startswith(fwd) and "mix" not in text, text
    rc, text = plan(lib, d, True)
    assert rc == 0 and "mix" not in text and (bwd is None or text.startswith(bwd)), text
    # and the same launches as a float32-storage descriptor's were never touched by the field either
    f = desc(dtype=_abi.F32, **kw)
    for back, general in ((False, "fwd_pairs |"), (True, "bwd_gather |")):
        rc, text = plan(lib, f, back)
        assert rc == 0 and "mix" not in text and (",f32," in text or text.startswith(general)), text


@pytest.mark.parametrize("family,seed", [("table", 5151), ("band", 5152), ("general", 5153)])
def test_the_stress_seeds_plan_onto_their_family(lib, family, seed):
    """tests/test_gpu_mixed.py runs 24 draws of scripts/stress_mixed.py per family and fails a case the intended kernels do
    not serve: the descriptors of those seeds, planned here without a GPU."""
    import random
    from test_gpu_parity import _load_script
    sm = _load_script("stress_mixed")
    rnd = random.Random(seed)
    plans = []
    for _ in range(24):
        case = sm.draw(rnd, family)
        fwd, bwd = sm.planned(case)
        assert sm.in_family(family, fwd, bwd), (sm.describe(case), fwd, bwd)
        plans.append((fwd, bwd))
    if family == "band":
        assert any(",dense>" in bwd for _, bwd in plans)
    if family == "general":
        assert ("fwd_pairs", "bwd_gather") in plans
