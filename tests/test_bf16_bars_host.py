"""What tests/bf16_bars.py rests on and what it adds, pinned without a GPU on every geometry of tests/bf16_cases.py
(the two large batches — the smallest the plan query routes to bwd_fast<...,mfma2> and fwd_tile<...,dma> — cut to their first
images: the images of a batch are independent):

  * the helper's signed out / grad_x equal oracle.forward / oracle.backward to 1e-6 (rel_err): the bars rest on the pinned
    oracle, not on new code;
  * the honest emulation of the specified arithmetic — the float64 result taken to float32, rounded to bf16 to nearest, the
    backward evaluated from that ROUNDED out, taken to float32, rounded to nearest — has excess <= 1 for out and for grad_x
    under the plain bars (no Gram term, no matrix-core term): the reference alone stays inside the bar;
  * four mutants of it exceed 1 under the per-element bars: a store that truncates instead of rounding (out everywhere;
    grad_x of cosine and dot — every term of L2's S carries the error of the rounded out, which covers a second rounding
    error there), one tap's grad_out 2 % off (grad_x), the backward's per-pair coefficients rounded to bf16 (grad_x of
    cosine), and one tap dropped (its grad_out taken as zero: grad_x).  The first three pass the bars the families' own files
    use (1e-2 of the largest magnitude for out, 2e-2 for grad_x) — asserted beside, which is what the new bars add; a whole
    dropped tap does not pass them at R = 1 and is held to the new bar alone.
    The 2 % tap is asserted on every geometry and measure (1.15 to 335) except where L2's S hides it: L2 at R = 3 (one of 48
    taps; S allows every term of the gradient ULP once more: 0.58 to 1.15) and TAP_TOO_WEAK, the 30-pixel R = 2 L2 map
    (0.92); there its figure is printed."""
import functools

import numpy as np
import pytest
import torch

import bf16_bars as BB
import bf16_cases as G
from conftest import rel_err

SLACK = G.SLACK
TAP_TOO_WEAK = {"2x8x6x5-R2zero-s1d1p2-l2-normal"}      # beside L2 at R = 3 (module docstring)
OLD_OUT, OLD_GX = 1e-2, 2e-2        # test_gpu_valid.TOL_BF16_OUT / TOL_BF16_GX, test_gpu_poison.BF_OUT / BF_GRAD
IMAGES = 6


# (shape, R, padding mode, input kind) x cosine / L2 / dot: the probe shapes
TABLE = [((2, 8, 7, 7), 1, "reflect", "normal"), ((2, 8, 7, 7), 3, "reflect", "normal"), ((1, 192, 14, 14), 2, "zeros", "normal"),
         ((2, 16, 9, 10), 2, "replicate", "relu"), ((1, 64, 14, 14), 1, "zeros", "smooth")]


def _table():
    return [pytest.param((tuple(sorted(G._geo(shape, R=R, mode=mode).items())), m, kind),
                         id="table-%s-R%d%s-%s-%s" % ("x".join(map(str, shape)), R, mode[:4], m, kind))
            for shape, R, mode, kind in TABLE for m in ("cos", "l2", "dot")]


def _studies():
    seen, out = set(), []
    for cid, family, g, m, kind, lay, op, env, fwd, bwd, gram, mfma in G.CASES:
        key = (tuple(sorted(g.items())), m, kind)
        if key not in seen:
            seen.add(key)
            out.append(pytest.param(key, id="%s-R%d%s-s%dd%dp%d-%s-%s" % ("x".join(map(str, g["shape"])), g["R"], g["padding_mode"][:4],
                                                                         g["stride"], g["dilation"], g["padding"], m, kind)))
    return out


def _rne(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


def _trunc(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _coef_to_bf16(k):
    return k.float().bfloat16().double()


def _old(a, ref):
    return rel_err(np.nan_to_num(a), np.nan_to_num(ref))


@functools.lru_cache(maxsize=None)
def _study(key):
    gkey, m, kind = key
    g = dict(gkey)
    x, go = G.inputs_of(g, m, kind, images=min(IMAGES, g["shape"][0]))
    cfg, ctor = G.config_of(g, m), G.ctor_of(g, m)
    ref = BB.reference(x, go, cfg)
    assert not np.isnan(ref["out"]).any() and not np.isnan(ref["grad_x"]).any()     # (L2 at distance 0: MeasNorm<2>::coef's 0)
    res = dict(x=x, go=go, ctor=ctor, ref=ref)

    def stored_backward(store, go_used=go, hook=None):
        out_b = store(ref["out"]).astype(np.float64)
        return out_b, store(BB.reference(x, go_used, cfg, out_stored=out_b, coef_hook=hook)["grad_x"])

    def figures(out_b, gx_b):
        return (BB.out_excess(out_b, ref["out"], SLACK), _old(out_b, ref["out"]),
                BB.grad_x_excess(gx_b, ref["grad_x"], ref["S"], SLACK), _old(gx_b, ref["grad_x"]))

    res["honest"] = figures(*stored_backward(_rne))
    res["trunc"] = figures(*stored_backward(_trunc))
    tap = min(3, go.shape[1] - 1)
    go_off = go.copy()
    go_off[:, tap] *= 0.98
    res["tap"] = figures(*stored_backward(_rne, go_off))
    res["coef"] = figures(*stored_backward(_rne, hook=_coef_to_bf16))
    go_drop = go.copy()
    go_drop[:, tap] = 0.0
    res["drop"] = figures(*stored_backward(_rne, go_drop))
    return res


@pytest.mark.parametrize("key", _studies())
def test_the_helper_agrees_with_the_oracle(key, oracle_lib):
    s = _study(key)
    out = oracle_lib.forward(s["x"], **s["ctor"])
    gx = oracle_lib.backward(s["x"], s["go"], **s["ctor"])
    e_out, e_gx = rel_err(s["ref"]["out"], out), rel_err(s["ref"]["grad_x"], gx)
    print(f"out {e_out:.2e} grad_x {e_gx:.2e}")
    assert out.shape == s["ref"]["out"].shape and not np.isnan(out).any() and not np.isnan(gx).any()
    assert e_out <= 1e-6 and e_gx <= 1e-6
    assert (s["ref"]["S"] >= 0).all() and (s["ref"]["T"] >= 0).all() and (s["ref"]["S_gram"] >= s["ref"]["S"]).all()
    assert (s["ref"]["T"] >= np.abs(s["ref"]["grad_x"]) * (1 - 1e-12)).all()       # |sum| <= sum of the absolute values
    if key[1] == "dot":
        assert not s["ref"]["S"].any()


@pytest.mark.parametrize("key", _studies() + _table())
def test_the_honest_emulation_stays_inside_both_bars(key):
    e_out, old_out, e_gx, old_gx = _study(key)["honest"]
    print(f"honest: out {e_out:.3f} (rel_err {old_out:.1e}) grad_x {e_gx:.3f} (rel_err {old_gx:.1e})")
    assert e_out <= 1.0 and e_gx <= 1.0
    assert old_out <= OLD_OUT and old_gx <= OLD_GX


@pytest.mark.parametrize("key", _studies() + _table())
def test_four_mutants_fail_the_new_bars_and_three_pass_the_old(key, request):
    s = _study(key)
    (gkey, m, kind), R = key, dict(key[0])["R"]
    for name in ("trunc", "tap", "coef", "drop"):
        e_out, old_out, e_gx, old_gx = s[name]
        print(f"{name}: out {e_out:.3f} (rel_err {old_out:.1e}) grad_x {e_gx:.3f} (rel_err {old_gx:.1e})")
    e_out, old_out, e_gx, old_gx = s["trunc"]
    assert e_out > 1.0 and old_out <= OLD_OUT
    if m != "l2":
        assert e_gx > 1.0 and old_gx <= OLD_GX
    e_out, old_out, e_gx, old_gx = s["tap"]
    if not (m == "l2" and R == 3) and request.node.callspec.id not in TAP_TOO_WEAK:
        assert e_gx > 1.0 and old_gx <= OLD_GX
    e_out, old_out, e_gx, old_gx = s["coef"]
    if m in ("cos", "cos_dissim"):
        assert e_gx > 1.0 and old_gx <= OLD_GX
    assert s["drop"][2] > 1.0


def test_every_family_is_named_by_a_variant_pattern_of_the_cases():
    names = " ".join(c[8] + " " + c[9] for c in G.CASES)
    for kernel in ("fwd_band<", "bwd_fast<", "fwd_gram<", ",mfma>", ",mfma2>", "fwd_tile<R1", "bwd_tile<R1", "fwd_tile<R2", "bwd_tile<R2", ",dma>",
                   ",dense>", "fwd_tile<R3", "bwd_tile<R3", "fwd_valid<", "bwd_valid<", "fwd_strided<", "bwd_strided<", "fwd_pairs$",
                   "bwd_gather$", "bwd_gather_banded$", "fwd_direct$", "bwd_direct$", ",gap>"):
        assert kernel in names, kernel


def test_the_bars_terms_and_nan_patterns():
    ref = np.array([1.0, np.nan, -2.0, 0.0])
    S = np.array([0.0, 0.0, 4.0, 1.0])
    T = np.array([1.0, 0.0, 6.0, 1.0])
    U = BB.ULP
    assert BB.grad_x_excess(ref.copy(), ref, S, SLACK) == 0.0
    assert BB.grad_x_excess(np.array([1.0, 0.0, -2.0, 0.0]), ref, S, SLACK) == float("inf")          # a number where NaN stands
    assert BB.grad_x_excess(np.array([1.0, np.nan, np.nan, 0.0]), ref, S, SLACK) == float("inf")
    assert BB.grad_x_excess(np.array([1.0, np.nan, -2.0]), ref, S[:3], SLACK) == float("inf")        # shapes
    # S = 0: the plain one-rounding bar; S > 0 widens its own element alone, T only with eps_T
    assert BB.grad_x_excess(np.array([1.0 + 0.9 * U, np.nan, -2.0, 0.0]), ref, S, SLACK) <= 1.0
    assert BB.grad_x_excess(np.array([1.0 + 1.1 * U, np.nan, -2.0, 0.0]), ref, S, SLACK) > 1.0
    assert BB.grad_x_excess(np.array([1.0, np.nan, -2.0 - 2.9 * 2 * U, 0.0]), ref, S, SLACK) <= 1.0
    assert BB.grad_x_excess(np.array([1.0, np.nan, -2.0 - 3.1 * 2 * U, 0.0]), ref, S, SLACK) > 1.0
    assert BB.grad_x_excess(np.array([1.0, np.nan, -2.0, 0.9 * U]), ref, S, SLACK) <= 1.0
    assert BB.grad_x_excess(np.array([1.0, np.nan, -2.0, 1.1 * U]), ref, S, SLACK) > 1.0
    assert BB.grad_x_excess(np.array([1.0, np.nan, -2.0, 1.1 * U]), ref, S, SLACK, T, 0.2 * U) <= 1.0
    assert BB.grad_x_excess(np.array([1.0, np.nan, -2.0, 1.3 * U]), ref, S, SLACK, T, 0.2 * U) > 1.0
    # out: `extra` stands beside the slack, element by element
    extra = np.array([0.0, 0.0, 0.0, 1e-3])
    assert BB.out_excess(np.array([1.0, np.nan, -2.0, 0.9e-3]), ref, SLACK, extra) <= 1.0
    assert BB.out_excess(np.array([1.0, np.nan, -2.0, 0.9e-3]), ref, SLACK) > 1.0
    assert BB.out_excess(np.array([1.0 + 2 * U, np.nan, -2.0, 0.0]), ref, SLACK, extra) == BB.one_rounding_excess(
        np.array([1.0 + 2 * U, np.nan, -2.0, 0.0]), ref, SLACK) > 1.0
    assert BB.out_excess(ref.copy(), ref, SLACK, extra) == 0.0
