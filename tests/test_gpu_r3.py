"""Radius-3 (7 x 7 window) "same" maps on the row-band kernels (csrc/nfp_tile.h: fwd_tile<3,...> / bwd_tile<3,...>; units
csrc/nfp_tile_r3_*.hip) against the ORACLE on the same inputs, in the manner of test_gpu_tile._run: the variant asserted,
forward and backward run twice with equal bits (NaNs included), rel_err <= 1e-5 for float32 and 1e-2 / 2e-2 (out / grad_x)
for bf16 on the same rounded inputs.  The shapes are the smallest at which each piece can go wrong: W = 2R + 1 (a column that
is the image of a left AND a right ring column — what the old W >= 2R + 2 rule kept away), the minimal band of R + 1 rows,
one channel quad, three bands, one thread per position with the shared channels-last staging, the widest served row.
NFP_TILE_R3=1 throughout (the default routing is pinned by tests/test_r3_plan.py)."""
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import nfp_switch, rel_err
from test_gpu_tile import _run

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _r3_on(monkeypatch):
    from neighbour_feature_pooling_amd import functional
    nfp_switch(monkeypatch, "NFP_TILE_R3", "1")
    functional._PLANS.clear()      # (a cached plan carries what the library answered under the previous switches)
    yield
    functional._PLANS.clear()


def _check(B, C, H, W, meas, mode, dtype=torch.float32, channels_last=False, similarity=True, nb=None, nan_ok=False):
    out, gx, ref, gref, fv, bv = _run(B, C, H, W, 3, meas, mode, DEV, dtype=dtype, channels_last=channels_last,
                                      similarity=similarity)
    lay = "nhwc" if channels_last else "nchw"
    st = "bf16" if dtype == torch.bfloat16 else "f32"
    assert fv.startswith("fwd_tile<R3,") and ",%s,%s>" % (st, lay) in fv, fv
    assert bv.startswith("bwd_tile<R3,") and ",%s,%s>" % (st, lay) in bv, bv
    if nb is not None:
        assert fv.endswith(">x%d" % nb) and bv.endswith(">x%d" % nb), (fv, bv)
    o, g, r, gr = out.float().cpu().numpy(), gx.float().cpu().numpy(), ref.numpy(), gref.numpy()
    assert np.array_equal(np.isnan(o), np.isnan(r)) and np.array_equal(np.isnan(g), np.isnan(gr)), (fv, bv)
    assert nan_ok or not np.isnan(gr).any()
    to, tg = (TOL, TOL) if dtype == torch.float32 else (1e-2, 2e-2)
    eo, eg = rel_err(np.nan_to_num(o), np.nan_to_num(r)), rel_err(np.nan_to_num(g), np.nan_to_num(gr))
    print(f"[{B},{C},{H},{W}] {meas} {mode} {st} {lay}: out {eo:.2e} grad_x {eg:.2e} [{fv} | {bv}]")
    assert eo <= to, fv
    assert eg <= tg, bv
    return gr


MEASURES = [("cosine", True), ("cosine", False), ("norm", True), ("rmse", True), ("dot", True), ("gfc", True)]


@pytest.mark.parametrize("meas,sim", MEASURES, ids=["cos", "cos_dissim", "l2", "rmse", "dot", "gfc"])
@pytest.mark.parametrize("mode", ["reflect", "replicate", "zeros"])
def test_7x7_every_padding_mode_and_measure(mode, meas, sim):
    """W = 2R + 1: pixel column 3 is the fold target of ring columns -3 and 9 under reflect padding.  RMSE under replicate
    padding pairs a pixel with its own copy — distance 0, no derivative: the NaN pattern is the oracle's (reflect padding
    with R >= 2 has such pairs too: x = 1 and its tap dx = -2)."""
    self_pairs = meas == "rmse" and mode != "zeros"
    gr = _check(2, 8, 7, 7, meas, mode, similarity=sim, nb=1, nan_ok=self_pairs)
    if meas == "rmse" and mode == "replicate":
        assert np.isnan(gr).any()


@pytest.mark.parametrize("B,C,H,W,meas,mode,nb", [
    (3, 12, 4, 8, "cosine", "reflect", 1),        # the minimal band (H = R + 1); three quads on two channel groups
    (3, 12, 4, 8, "norm", "replicate", 1),
    (1, 4, 9, 8, "cosine", "replicate", 2),       # one quad; bands of 5 / 4 rows
    (2, 8, 14, 14, "cosine", "reflect", 3),       # bands of 5 / 5 / 4 rows
    (2, 8, 14, 14, "norm", "zeros", 3),
    (2, 8, 4, 45, "cosine", "reflect", 1),        # the widest served row: (45 + 6) * 10 = 510 of the backward's 512 threads
    (2, 8, 8, 45, "norm", "reflect", 2)])
def test_bands_quads_and_the_widest_row(B, C, H, W, meas, mode, nb):
    _check(B, C, H, W, meas, mode, nb=nb)


@pytest.mark.parametrize("dtype,channels_last", [(torch.float32, True), (torch.bfloat16, True), (torch.bfloat16, False)],
                         ids=["f32-nhwc", "bf16-nhwc", "bf16-nchw"])
@pytest.mark.parametrize("B,C,H,W,meas", [(256, 32, 14, 14, "cosine"), (2, 8, 7, 7, "norm")])
def test_storage_forms(B, C, H, W, meas, dtype, channels_last):
    """[256,32,14,14] fills the chip: ONE channel group per position, the wavefront-shared channels-last staging (a partial
    last wavefront included: 260 threads)."""
    _check(B, C, H, W, meas, "reflect", dtype=dtype, channels_last=channels_last)


# ---- the fused tails: nfp_with_gap, nfp_pool ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape,nb", [((2, 8, 7, 7), 1), ((2, 8, 14, 14), 3)])
@pytest.mark.parametrize("meas", ["cosine", "norm"])
def test_with_gap_and_pool_against_the_layer(shape, nb, meas):
    """GAP(x) against x.mean, the maps and grad_x against the layer's own (the plain R = 3 kernels, held to the oracle above)
    at the float32 bar; one forward launch, the fold of the bands' partial sums, one backward launch — and none before the
    first step: radius 3 has no workspace."""
    from neighbour_feature_pooling_amd import NFPPooling, _abi, nfp_pool, nfp_with_gap
    from neighbour_feature_pooling_amd.synth import feature_map
    L = _abi.load()
    B, C, H, W = shape
    kw = dict(R=3, measure=meas, padding=3, **(dict(p=2) if meas == "norm" else {}))
    layer = NFPPooling(C, **kw)
    xh = feature_map(shape, 71)
    go = torch.from_numpy(feature_map((B, 48, H, W), 72)).to(DEV)
    gg = torch.from_numpy(feature_map((B, C), 73)).to(DEV)
    gn = torch.from_numpy(feature_map((B, 48), 74)).to(DEV)
    x0 = torch.from_numpy(xh).to(DEV).requires_grad_(True)
    m0 = layer(x0)
    assert L.nfp_last_variant().decode().startswith("fwd_tile<R3,")
    (g_maps,) = torch.autograd.grad((m0 * go).sum(), x0, retain_graph=True)
    (g_pool,) = torch.autograd.grad((m0.mean((2, 3)) * gn).sum(), x0)
    mean = torch.from_numpy(xh.astype(np.float64).mean((2, 3)))
    torch.cuda.synchronize()

    x = torch.from_numpy(xh).to(DEV).requires_grad_(True)
    n0 = L.nfp_launch_count()
    gap, maps = nfp_with_gap(x, layer.config)
    fv = L.nfp_last_variant().decode()
    assert L.nfp_launch_count() - n0 == 2, fv                     # fwd_tile + pool_fold; nothing set up before them
    assert fv.startswith("fwd_tile<R3,") and fv.endswith(",gap>x%d+pool_fold" % nb), fv
    ((gap * gg).sum() + (maps * go).sum()).backward()
    bv = L.nfp_last_variant().decode()
    assert L.nfp_launch_count() - n0 == 3 and bv.startswith("bwd_tile<R3,") and bv.endswith(",gap>x%d" % nb), bv
    assert rel_err(gap.detach().cpu().numpy(), mean.numpy()) <= TOL
    assert rel_err(maps.detach().cpu().numpy(), m0.detach().cpu().numpy()) <= TOL, fv
    ref_gx = g_maps.double().cpu().numpy() + (gg.double().cpu().numpy() / (H * W))[:, :, None, None]
    assert rel_err(x.grad.cpu().numpy(), ref_gx) <= TOL, bv

    x = torch.from_numpy(xh).to(DEV).requires_grad_(True)
    n0 = L.nfp_launch_count()
    gap, nfpm = nfp_pool(x, layer.config)
    fv = L.nfp_last_variant().decode()
    assert L.nfp_launch_count() - n0 == 2 and fv.startswith("fwd_tile<R3,") and fv.endswith(",pool>x%d+pool_fold" % nb), fv
    ((gap * gg).sum() + (nfpm * gn).sum()).backward()
    bv = L.nfp_last_variant().decode()
    assert L.nfp_launch_count() - n0 == 3 and bv.startswith("bwd_tile<R3,") and bv.endswith(",pool>x%d" % nb), bv
    assert rel_err(gap.detach().cpu().numpy(), mean.numpy()) <= TOL
    assert rel_err(nfpm.detach().cpu().numpy(), m0.detach().double().mean((2, 3)).cpu().numpy()) <= TOL
    ref_gx = g_pool.double().cpu().numpy() + (gg.double().cpu().numpy() / (H * W))[:, :, None, None]
    assert rel_err(x.grad.cpu().numpy(), ref_gx) <= TOL, bv


def test_head_first_step_is_one_pass():
    """NFPHead(R=3) on [4,16,7,7]: GAP(fmap) and the 48 maps from the fused pass — fwd_tile<R3,...,gap> and the fold of its
    partial sums, no torch mean beside the layer — and one backward kernel for both gradients."""
    from neighbour_feature_pooling_amd import _abi
    from neighbour_feature_pooling_amd.heads import NFPHead
    L = _abi.load()
    torch.manual_seed(3)
    head = NFPHead(16, bottleneck_dim=24, R=3).to(DEV)
    x = torch.randn(4, 16, 7, 7, device=DEV, requires_grad=True)
    n0 = L.nfp_launch_count()
    gap, maps = head._gap_nfp(x)
    fv = L.nfp_last_variant().decode()
    assert L.nfp_launch_count() - n0 == 2 and fv == "fwd_tile<R3,cos,f32,nchw,gap>x1+pool_fold", fv
    assert maps.shape == (4, 48, 7, 7) and torch.allclose(gap, x.detach().mean((2, 3)), rtol=0, atol=1e-6)
    (gap.sum() + maps.square().sum()).backward()
    bv = L.nfp_last_variant().decode()
    assert L.nfp_launch_count() - n0 == 3 and bv == "bwd_tile<R3,cos,f32,nchw,gap>x1", bv
    x2 = x.detach().clone().requires_grad_(True)
    head(x2).sum().backward()      # ... and the whole head runs on it
    assert torch.isfinite(x2.grad).all()


# ---- reference goldens ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["r3_cos_reflect_2x8x7x7", "r3_l2_zeros_2x8x7x7", "r3_cos_replicate_2x8x7x7",
                                  "r3_cos_reflect_1x8x14x14"])
def test_r3_kernels_match_reference_golden(name):
    import cases as K
    import cases_r3 as K3
    from conftest import assert_matches_golden, load_golden
    from neighbour_feature_pooling_amd import NFPPooling, _abi
    c = K3.R3_BY_NAME[name]
    x = torch.from_numpy(K.make_input(c)).to(DEV).requires_grad_(True)
    m = NFPPooling(c["shape"][1], **c["ctor"])
    L = _abi.load()
    out = m(x)
    fv = L.nfp_last_variant().decode()
    gx, = torch.autograd.grad(out, x, torch.from_numpy(K.make_grad_out(c, tuple(out.shape))).to(DEV))
    torch.cuda.synchronize()
    bv = L.nfp_last_variant().decode()
    assert fv.startswith("fwd_tile<R3,") and bv.startswith("bwd_tile<R3,"), (fv, bv)
    assert_matches_golden(out.detach().cpu().numpy(), gx.cpu().numpy(), load_golden(name), TOL, TOL)


# ---- poisoned and fenced buffers; the LDS-poison build ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype,layout", [("f32", "nchw"), ("f32", "nhwc"), ("bf16", "nchw"), ("bf16", "nhwc")])
@pytest.mark.parametrize("shape", [(2, 8, 7, 7), (2, 8, 14, 14)], ids=["7x7", "14x14"])
def test_r3_kernels_on_poisoned_and_fenced_buffers(shape, dtype, layout, monkeypatch):
    from neighbour_feature_pooling_amd import functional
    from test_gpu_poison import MapsCase, _flags
    monkeypatch.setenv("NFP_PY_NODES", "1")          # (as test_gpu_poison's own cases run: the Python nodes take the fenced buffers)
    monkeypatch.setattr(functional, "_CPP", None)
    monkeypatch.setattr(functional, "_PLANS", OrderedDict())
    name = "r3_%s_%s_%s" % ("x".join(map(str, shape)), dtype, layout)
    MapsCase(name, shape, dict(R=3, measure="cosine", padding=3), _flags(dtype, layout)).check("fwd_tile<R3", "bwd_tile<R3")


def test_r3_kernels_with_poisoned_lds():
    """The oracle and golden cases of this file once more on the -DNFP_LDS_POISON build (every word of a workgroup's LDS a
    signalling NaN at entry), in one child process — as test_gpu_tile.py::test_row_band_kernels_with_poisoned_lds."""
    if os.environ.get("NFP_TEST_LIB"):
        pytest.skip("this IS the run on the test build")
    env = dict(os.environ, NFP_TEST_LIB="libnfp_hip_poison.so")
    sel = "every_padding_mode or widest_row or storage_forms or reference_golden or against_the_layer"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", sel,
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=900)
    tail = r.stdout[-3000:] + r.stderr[-1000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "failed" not in r.stdout, tail
