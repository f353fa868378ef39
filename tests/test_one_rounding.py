"""The power of tests/one_rounding.py::one_rounding_excess, pinned without a GPU: on the float64 formulation of cosine and
L2 (`_host.nfp_host`; x bf16-rounded, grad_out float32 — the values the map_f32 kernels see) the reference gradient, taken to
float32 and rounded to bf16 to nearest, passes the bar; the same gradient converted by truncation, computed with one tap's
grad_out 2 % off, or with one element per image left unstored (zero) fails it."""
import numpy as np
import pytest
import torch

from neighbour_feature_pooling_amd.functional import NfpConfig
from neighbour_feature_pooling_amd._host import nfp_host
from neighbour_feature_pooling_amd.synth import feature_map
from one_rounding import one_rounding_excess

TOL = 1e-5      # the float32 bar of the fixed hot-path cases (tests/test_gpu_parity.py)

#        shape, R, padding mode, input kind
SHAPES = [((3, 8, 5, 7), 1, "reflect", "normal"),
          ((2, 16, 6, 6), 2, "zeros", "normal"),
          ((4, 64, 7, 7), 1, "reflect", "relu"),
          ((2, 8, 24, 23), 1, "reflect", "normal"),
          ((2, 40, 24, 24), 1, "reflect", "relu"),
          ((1, 8, 25, 24), 2, "replicate", "normal")]


def _rne(a32):
    return torch.from_numpy(a32).bfloat16().float().numpy()


def _trunc(a32):
    return (np.ascontiguousarray(a32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _gradient(x, go, cfg):
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    gx, = torch.autograd.grad(nfp_host(x64, cfg), x64, torch.from_numpy(go).double())
    return gx.numpy()


@pytest.mark.parametrize("measure", ["cosine", "norm"])
@pytest.mark.parametrize("shape,R,mode,kind", SHAPES)
def test_round_to_nearest_passes_and_three_mutants_fail(shape, R, mode, kind, measure):
    cfg = NfpConfig(R=R, measure=measure, p=2, padding=R, padding_mode=mode, diff_weights=measure == "norm")
    x = _rne(feature_map(shape, 31, kind))
    go = feature_map((shape[0], cfg.out_channels) + shape[2:], 32)
    ref = _gradient(x, go, cfg)
    assert not np.isnan(ref).any()
    g32 = ref.astype(np.float32)
    honest = one_rounding_excess(_rne(g32), ref, TOL)
    truncated = one_rounding_excess(_trunc(g32), ref, TOL)
    go_off = go.copy()
    go_off[:, 3] *= 0.98                                        # one tap's weight 2 % off
    tap = one_rounding_excess(_rne(_gradient(x, go_off, cfg).astype(np.float32)), ref, TOL)
    holed = _rne(g32)
    for b in range(shape[0]):                                   # one element per image never stored: the one of median size
        flat = holed[b].reshape(-1)
        flat[np.argsort(np.abs(flat))[flat.size // 2]] = 0.0
    hole = one_rounding_excess(holed, ref, TOL)
    print(f"{shape} {measure}: honest {honest:.3f} truncation {truncated:.2f} tap {tap:.1f} hole {hole:.1f}")
    assert honest <= 1.0
    assert truncated > 1.0
    assert tap > 1.0
    assert hole > 1.0


def test_nan_patterns_and_degenerate_references():
    ref = np.array([1.0, np.nan, -2.0, 0.0])
    assert one_rounding_excess(ref.copy(), ref, TOL) == 0.0
    assert one_rounding_excess(np.array([1.0, 0.0, -2.0, 0.0]), ref, TOL) == float("inf")      # a number where NaN stands
    assert one_rounding_excess(np.array([1.0, np.nan, np.nan, 0.0]), ref, TOL) == float("inf")
    assert one_rounding_excess(np.array([1.0, np.nan, -2.0]), ref, TOL) == float("inf")        # shapes
    # an element at zero has the slack alone; one at the top of the range 2^-8 of itself beside it
    top = 2.0
    assert one_rounding_excess(np.array([1.0, np.nan, -2.0, 0.9 * TOL * top]), ref, TOL) <= 1.0
    assert one_rounding_excess(np.array([1.0, np.nan, -2.0, 1.1 * TOL * top]), ref, TOL) > 1.0
    assert one_rounding_excess(np.array([1.0, np.nan, -2.0 * (1 + 2.0 ** -8), 0.0]), ref, TOL) <= 1.0
    assert one_rounding_excess(np.array([1.0, np.nan, -2.0 * (1 + 2.0 ** -7), 0.0]), ref, TOL) > 1.0
    zeros = np.zeros(5)
    assert one_rounding_excess(zeros, zeros, TOL) == 0.0
    assert one_rounding_excess(np.array([0, 0, 1e-30, 0, 0]), zeros, TOL) == float("inf")
    assert one_rounding_excess(np.full(3, np.nan), np.full(3, np.nan), TOL) == 0.0
