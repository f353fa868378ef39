"""The per-element bar for a bf16 gradient that is ONE round-to-nearest of a float32 value (nfp_desc.map_f32: grad_x is
computed in float32 from exactly representable inputs and a float32 `out`, then rounded once).

Derived, not measured.  bf16 keeps 8 significant bits, so round-to-nearest of a value v lands within 2^-8 |v| of it.  The
float32 value the kernel rounds is itself within slack * max|ref| of the reference (`slack`: the bar the suite holds the
same kernel family to in float32 storage), and rounding that neighbour instead of the reference moves the result by at most
another 2^-8 of the shift.  So for every element

    |got - ref| <= 2^-8 |ref| + (1 + 2^-8) slack max|ref|

and `one_rounding_excess` is the largest ratio of the left side to the right: a result passes at <= 1.  A conversion by
truncation sits near 2, a 2 % error in one tap's weight or one unstored element far above (tests/test_one_rounding.py)."""
import numpy as np

ULP = 2.0 ** -8


def one_rounding_excess(got, ref, slack):
    """max over elements of |got - ref| / (2^-8 |ref| + (1 + 2^-8) slack max|ref|); elements where `ref` is NaN are skipped;
    inf when the NaN patterns differ (or the shapes)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return float("inf")
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return float("inf")
    if nan.all():
        return 0.0
    g, r = got[~nan], ref[~nan]
    with np.errstate(invalid="ignore"):
        diff = np.where(g == r, 0.0, np.abs(g - r))      # (equal infinities agree)
    bar = ULP * np.abs(r) + (1.0 + ULP) * slack * float(np.max(np.abs(r)))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff == 0.0, 0.0, diff / bar)   # (an all-zero reference: any other value is infinitely far)
    return float(np.max(np.where(np.isnan(ratio), np.inf, ratio)))
