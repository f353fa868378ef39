"""The L1 family of the valid-map kernels (csrc/nfp_valid.hip: fwd_valid<R,l1,..> / bwd_valid<R,l1,..> — Norm p = 1 on the
difference weights, the class default, and EMD) against the ORACLE (oracle/nfp_oracle.c) with padding=0 on seeded inputs
from synth.feature_map, with the conventions and helpers of test_gpu_valid.py: the smallest shapes at which the half stencil,
the row bands, the channel chunks, the channel blocks and the two layouts can go wrong, ReLU inputs (about half the values
exact zeros: sgn(0) = 0 on most pairs), the edge values, a seeded sweep inside the served set, determinism, the contract
that the maps may be overwritten before the backward, the fall-backs, both autograd nodes, and NFPInsert /
NFPInsertNet(valid_layer=True).  Every served case asserts the `l1` variant both ways and ONE launch each way.

Bars: float32 1e-5 of the tensor's max; bf16 1e-2 (maps) / 2e-2 (grad_x) on bf16-rounded inputs.  They carry over from the
other families because the forward is a sum of non-negative terms (no cancellation) and the gradient a sum of at most 8 / 24
terms +-grad_out whose signs are exact in float32: a - t of two floats has the sign of the float64 difference."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cases_insert as KI
from conftest import load_golden, rel_err
from test_gpu_valid import TOL, _bf16_round, _check, _device_run, _inputs, _radii
from test_insert_host import fixture_errors, run_insert

pytestmark = pytest.mark.gpu
F32 = 1e-5      # the fixture bar of test_gpu_insert.py

SHAPES = [
    (2, 8, 3, 3), (2, 8, 5, 5),                                    # one output (R = 1 / R = 2): every input but one a border pixel
    (1, 8, 3, 9), (1, 8, 9, 3),                                    # one output row, one output column
    (3, 8, 4, 4),                                                  # every pair has a border end
    (2, 16, 7, 6), (2, 3, 6, 7), (2, 1, 6, 6),                     # odd W; C odd, C of 1 (NCHW)
    (2, 512, 7, 7), (2, 192, 14, 14),                              # several channel chunks and channel blocks on a small map
    (2, 8, 24, 23), (1, 16, 41, 37),                               # several row bands of unequal height, halo rows
    (1, 4, 6, 128),                                                # the widest served row
    (300, 8, 6, 6),                                                # more workgroups than CUs
]
EMD_SHAPES = [(2, 16, 7, 6), (2, 3, 6, 7), (2, 8, 24, 23)]


def _grid():
    out = []
    for s in SHAPES:
        for R in _radii(s):
            out.append((s, R, "norm", "f32", "nchw"))
            if s[1] % 8 == 0:
                out += [(s, R, "norm", "f32", "nhwc"), (s, R, "norm", "bf16", "nchw"), (s, R, "norm", "bf16", "nhwc")]
    for s in EMD_SHAPES:
        for R in _radii(s):
            out.append((s, R, "emd", "f32", "nchw"))
            if s[1] % 8 == 0:
                out.append((s, R, "emd", "bf16", "nhwc"))
    return out


def _ctor(R, meas, sim=True):
    return dict(R=R, measure=meas, padding=0, similarity=sim)       # (p: the class default, 1)


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


def _assert_l1(R, fv, bv):
    assert fv.startswith(f"fwd_valid<{R},l1,") and bv.startswith(f"bwd_valid<{R},l1,"), (fv, bv)


def _case(shape, R, meas, dtype, layout, sim=True, strided=False, tweak=None, kind="normal"):
    x, go = _inputs(shape, R, tweak, kind)
    ref_out, ref_gx = _reference(shape, R, meas, sim, dtype == "bf16", tweak, kind)
    out, gx, fv, bv = _device_run(x, go, _config(shape[1], R, meas, sim), dtype, layout, strided)   # (one launch each way)
    _assert_l1(R, fv, bv)
    assert np.isfinite(gx).all() and np.isfinite(out).all()
    _check(out, gx, ref_out, ref_gx, dtype, f"{shape} R={R} {meas} {dtype} {layout} {fv} {bv}")
    return out, gx


@pytest.mark.parametrize("shape,R,meas,dtype,layout", _grid(),
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_l1_kernels_match_the_oracle(shape, R, meas, dtype, layout):
    _case(shape, R, meas, dtype, layout)


@pytest.mark.parametrize("shape", [(2, 16, 7, 6), (2, 8, 24, 23)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("meas", ["norm", "emd"])
@pytest.mark.parametrize("R", [1, 2])
def test_dissimilarity(shape, meas, R):
    _case(shape, R, meas, "f32", "nchw", sim=False)
    _case(shape, R, meas, "f32", "nhwc", sim=False)
    _case(shape, R, meas, "bf16", "nhwc", sim=False)


@pytest.mark.parametrize("shape", [(2, 16, 7, 6), (2, 8, 24, 23)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("R", [1, 2])
def test_batch_strided_views_are_read_in_place(shape, dtype, R):
    _case(shape, R, "norm", dtype, "nchw", strided=True)


@pytest.mark.parametrize("shape", [(2, 16, 7, 6), (2, 192, 14, 14), (2, 8, 24, 23)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_relu_inputs_take_sign_zero_on_most_pairs(shape, R, layout):
    """About half the values of a ReLU map are exact zeros: most channel differences are 0 - 0, a - 0 or 0 - t."""
    x, _ = _inputs(shape, R, None, "relu")
    assert 0.4 < float((x == 0).mean()) < 0.6
    _case(shape, R, "norm", "f32", layout, kind="relu")


@pytest.mark.parametrize("tweak,kind", [("identical", "normal"), ("zero_pixels", "relu"), ("zero_pixels", "normal")])
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_identical_and_all_zero_pixels_give_finite_gradients(tweak, kind, R, layout):
    """Distance 0 between two adjacent pixels, and all-zero pixels: the gradient of |.| at 0 is 0 — no NaN, no inf."""
    for shape in ((2, 16, 7, 6), (2, 8, 24, 23)):
        out, gx = _case(shape, R, "norm", "f32", layout, tweak=tweak, kind=kind)
        assert not np.isnan(gx).any() and not np.isnan(out).any()
        if tweak == "identical":
            assert (out == 0).any()          # (the pair of identical pixels: an exact zero distance)


def sweep_cases():
    """40 geometries drawn INSIDE the served set: (shape, R, measure, similarity, dtype, layout)."""
    rng = np.random.RandomState(20250611)
    out = []
    for _ in range(40):
        R = int(rng.randint(1, 3))
        B, C = int(rng.randint(1, 6)), int(rng.randint(1, 71))
        H, W = int(rng.randint(2 * R + 1, 41)), int(rng.randint(2 * R + 1, 41))
        meas = ["norm", "emd"][int(rng.randint(0, 2))]
        sim = bool(rng.randint(0, 2))
        dtype = ["f32", "bf16"][int(rng.randint(0, 2))]
        nhwc_ok = C % (8 if dtype == "bf16" else 4) == 0
        layout = ["nchw", "nhwc"][int(rng.randint(0, 2))] if nhwc_ok else "nchw"
        out.append(((B, C, H, W), R, meas, sim, dtype, layout))
    return out


def sweep_descriptor(shape, R, meas, sim, dtype, layout):
    from neighbour_feature_pooling_amd.functional import _canon, build_desc
    return build_desc(shape, _canon(shape, layout), torch.bfloat16 if dtype == "bf16" else torch.float32,
                      _config(shape[1], R, meas, sim))


def test_seeded_sweep_of_40_geometries_inside_the_served_set():
    from neighbour_feature_pooling_amd import _abi
    L = _abi.load()
    cases = sweep_cases()
    assert len(cases) == 40
    for shape, R, meas, sim, dtype, layout in cases:
        assert L.nfp_valid_abs_supported(ctypes.byref(sweep_descriptor(shape, R, meas, sim, dtype, layout))) == 1
        _case(shape, R, meas, dtype, layout, sim=sim)      # (asserts the l1 variant and one launch each way: no fall-back)


@pytest.mark.parametrize("meas,R,dtype,layout", [("norm", 1, "f32", "nchw"), ("norm", 2, "f32", "nhwc"), ("emd", 2, "bf16", "nchw"),
                                                 ("norm", 1, "bf16", "nhwc")])
def test_two_runs_agree_bitwise_and_an_image_does_not_depend_on_the_batch(meas, R, dtype, layout):
    shape = (5, 16, 24, 23)
    x, go = _inputs(shape, R)
    cfg = _config(shape[1], R, meas)
    a = _device_run(x, go, cfg, dtype, layout)
    b = _device_run(x, go, cfg, dtype, layout)
    _assert_l1(R, a[2], a[3])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    one = _device_run(x[:1].copy(), go[:1].copy(), cfg, dtype, layout)
    assert np.array_equal(a[0][:1], one[0]) and np.array_equal(a[1][:1], one[1])


@pytest.mark.parametrize("R", [1, 2])
def test_the_channel_block_split_is_bit_neutral(R):
    """(2, 512, 7, 7) runs 16 channel blocks of 32 along grid.z, (300, 512, 7, 7) two of 256: image 0 agrees bitwise."""
    shape = (2, 512, 7, 7)
    x, go = _inputs(shape, R)
    cfg = _config(512, R, "norm")
    small = _device_run(x, go, cfg, "f32", "nchw")
    big = _device_run(np.tile(x, (150, 1, 1, 1)), np.tile(go, (150, 1, 1, 1)), cfg, "f32", "nchw")
    _assert_l1(R, big[2], big[3])
    assert np.array_equal(small[0], big[0][:2]) and np.array_equal(small[1], big[1][:2])
    assert np.array_equal(big[1][:2], big[1][298:])


def test_an_empty_batch_launches_nothing():
    from neighbour_feature_pooling_amd import _abi, nfp_valid
    L = _abi.load()
    x = torch.zeros(0, 8, 6, 6, device="cuda:0", requires_grad=True)
    n0 = L.nfp_launch_count()
    out = nfp_valid(x, _config(8, 1, "norm"))
    assert tuple(out.shape) == (0, 8, 4, 4) and out.dtype == torch.float32
    gx, = torch.autograd.grad(out, x, torch.zeros_like(out))
    assert tuple(gx.shape) == (0, 8, 6, 6)
    assert L.nfp_launch_count() == n0


def _grad_after_overwriting_the_maps(x, go, cfg, overwrite):
    from neighbour_feature_pooling_amd import _abi, nfp_valid
    xt = torch.from_numpy(x).to("cuda:0").requires_grad_(True)
    out = nfp_valid(xt, cfg)
    fv = _abi.load().nfp_last_variant().decode()
    if overwrite:
        # in place and outside the graph (a recorded out.zero_() would itself have gradient 0): the storage changes and the
        # tensor's version counter moves, which raises in the backward of a node that had saved `out`
        v0 = out._version
        out.detach().zero_()
        assert out._version > v0 and float(out.detach().abs().max()) == 0.0
    gx, = torch.autograd.grad(out, xt, torch.from_numpy(go).to("cuda:0"))
    torch.cuda.synchronize()
    return gx.cpu().numpy(), fv, _abi.load().nfp_last_variant().decode()


@pytest.mark.parametrize("py_nodes", [False, True], ids=["cpp_node", "python_node"])
def test_the_maps_may_be_overwritten_before_the_backward(py_nodes, monkeypatch):
    from neighbour_feature_pooling_amd import functional
    if py_nodes:
        monkeypatch.setenv("NFP_PY_NODES", "1")
        monkeypatch.setattr(functional, "_CPP", None)
        assert not functional._cpp_nodes()
    else:
        assert hasattr(functional._cpp_nodes(), "nfp_valid_abs_apply")
    shape, R = (2, 16, 7, 6), 1
    x, go = _inputs(shape, R)
    cfg = _config(16, R, "norm")
    kept, fv, bv = _grad_after_overwriting_the_maps(x, go, cfg, False)
    _assert_l1(R, fv, bv)
    zeroed, fv, bv = _grad_after_overwriting_the_maps(x, go, cfg, True)
    _assert_l1(R, fv, bv)
    assert np.array_equal(kept, zeroed)
    assert rel_err(kept, _reference(shape, R, "norm", True, False)[1]) <= TOL


@pytest.mark.parametrize("dtype,layout", [("f32", "nchw"), ("bf16", "nhwc")])
def test_the_cpp_node_and_the_python_node_agree_bitwise(dtype, layout, monkeypatch):
    from neighbour_feature_pooling_amd import functional
    shape, R = (2, 16, 24, 23), 2
    x, go = _inputs(shape, R)
    cfg = _config(16, R, "norm")
    assert hasattr(functional._cpp_nodes(), "nfp_valid_abs_apply")
    a = _device_run(x, go, cfg, dtype, layout)
    monkeypatch.setenv("NFP_PY_NODES", "1")
    monkeypatch.setattr(functional, "_CPP", None)
    assert not functional._cpp_nodes()
    b = _device_run(x, go, cfg, dtype, layout)
    _assert_l1(R, a[2], a[3])
    _assert_l1(R, b[2], b[3])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_a_refused_row_width_falls_to_the_general_kernels():
    shape, R = (1, 8, 7, 129), 1
    x, go = _inputs(shape, R)
    ref_out, ref_gx = _reference(shape, R, "norm", True, False)
    out, gx, fv, bv = _device_run(x, go, _config(8, R, "norm"), "f32", "nchw", expect_valid=False)
    assert not fv.startswith("fwd_valid") and not bv.startswith("bwd_valid"), (fv, bv)
    _check(out, gx, ref_out, ref_gx, "f32", f"W = 129: {fv} {bv}")


def test_the_switch_routes_to_the_general_kernels(monkeypatch):
    shape, R = (2, 16, 7, 6), 1
    x, go = _inputs(shape, R)
    ref_out, ref_gx = _reference(shape, R, "norm", True, False)
    cfg = _config(16, R, "norm")
    monkeypatch.setenv("NFP_VALID_OFF", "1")
    out, gx, fv, bv = _device_run(x, go, cfg, "f32", "nchw", expect_valid=False)
    assert not fv.startswith("fwd_valid") and not bv.startswith("bwd_valid"), (fv, bv)
    _check(out, gx, ref_out, ref_gx, "f32", f"NFP_VALID_OFF=1: {fv} {bv}")
    monkeypatch.delenv("NFP_VALID_OFF")
    out, gx, fv, bv = _device_run(x, go, cfg, "f32", "nchw")
    _assert_l1(R, fv, bv)
    _check(out, gx, ref_out, ref_gx, "f32", f"switch unset: {fv} {bv}")


@pytest.mark.parametrize("name", ["insert_default_2x12x9x9", "insert_r2_2x8x9x11"])
def test_insert_with_the_valid_layer_matches_the_fixture(name, monkeypatch):
    from neighbour_feature_pooling_amd import NFPInsert, _abi
    monkeypatch.setenv("NFP_CPROJ_TORCH", "0")      # (the projection on the cproj kernels, as test_gpu_insert.py)
    L = _abi.load()
    dev = torch.device("cuda:0")
    c = KI.INSERT_BY_NAME[name]
    g = load_golden(name)
    m = NFPInsert(c["shape"][1], valid_layer=True, **c["kw"])
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p:")}, strict=True)
    m.train(c["train"])
    m = m.to(dev)
    R = m.nfp.R
    # the layer's own launches, each way: exactly 1 + 1, the l1 variants
    x = torch.from_numpy(KI.make_input(c)).to(dev).requires_grad_(True)
    n0 = L.nfp_launch_count()
    maps = m._layer(x)
    n1, fv = L.nfp_launch_count(), L.nfp_last_variant().decode()
    torch.autograd.grad(maps, x, torch.ones_like(maps))
    torch.cuda.synchronize()
    n2, bv = L.nfp_launch_count(), L.nfp_last_variant().decode()
    assert (n1 - n0, n2 - n1) == (1, 1)
    _assert_l1(R, fv, bv)
    n0 = L.nfp_launch_count()
    got = run_insert(m, c, dev)
    torch.cuda.synchronize()
    assert L.nfp_launch_count() - n0 == 2 + 6        # ... plus the projection: 3 + 3 launches in training
    errs = fixture_errors(got, g)
    print(name, "fixture", errs)
    for k, e in errs.items():
        assert e <= F32, (k, e)


def _net_step(valid_layer, dev):
    """out and every parameter gradient of one seeded NFPInsertNet train step on `dev` (numpy)."""
    from neighbour_feature_pooling_amd.models import NFPInsertNet
    torch.manual_seed(0)
    m = NFPInsertNet(num_classes=5, nfp_insert_idx=1, valid_layer=valid_layer)
    x = torch.randn(2, 3, 64, 64)
    m, x = m.to(dev), x.to(dev)
    out = m(x)
    torch.nn.functional.cross_entropy(out, torch.tensor([1, 3], device=dev)).backward()
    res = {"out": out.detach().cpu().numpy()}
    res.update({"g:" + k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters()})
    return res


def test_insert_net_train_step_with_the_valid_layer():
    """One train step at [2,3,64,64], valid_layer=True on the device against its CPU run; the bar is 4x the error of the
    valid_layer=False arm against ITS CPU run (the largest over out and the parameter gradients), not below 1e-5.
    Measured on an MI355X: valid_layer=False 2.31, valid_layer=True 2.38, bar 9.2 — at this size the trunk behind the insert
    ends in 2x2 and 1x1 maps, so with B = 2 its train-mode BatchNorm layers normalise over 8 or 2 values per channel and
    neither arm is close to its CPU run.  The case shows that the keyword leaves the step finite and no worse than the
    default arm; the oracle and fixture cases above hold the layer itself."""
    dev = torch.device("cuda:0")
    cpu = _net_step(False, "cpu")
    cpu_on = _net_step(True, "cpu")
    assert all(np.array_equal(cpu[k], cpu_on[k]) for k in cpu)      # (on the CPU the keyword changes nothing)
    off = _net_step(False, dev)
    on = _net_step(True, dev)
    e_off = {k: rel_err(off[k], cpu[k]) for k in cpu}
    e_on = {k: rel_err(on[k], cpu[k]) for k in cpu}
    bar = max(1e-5, 4.0 * max(e_off.values()))
    print("NFPInsertNet step: valid_layer=False max err", max(e_off.values()), "valid_layer=True max err", max(e_on.values()),
          "bar", bar)
    assert all(np.isfinite(v).all() for v in on.values())
    for k, e in e_on.items():
        assert e <= bar, (k, e, bar)


def test_insert_net_valid_layer_launches_the_l1_kernels():
    from neighbour_feature_pooling_amd import _abi
    from neighbour_feature_pooling_amd.models import NFPInsertNet
    L = _abi.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = NFPInsertNet(num_classes=5, nfp_insert_idx=1, valid_layer=True).to(dev)
    x = torch.randn(2, 24, 16, 16, device=dev, requires_grad=True)      # what block 1 hands the insert at [2,3,64,64]
    n0 = L.nfp_launch_count()
    maps = m.insert._layer(x)
    fv = L.nfp_last_variant().decode()
    torch.autograd.grad(maps, x, torch.ones_like(maps))
    torch.cuda.synchronize()
    assert L.nfp_launch_count() - n0 == 2
    _assert_l1(1, fv, L.nfp_last_variant().decode())
