"""Golden-vector cases of radius-3 (7 x 7 window) "same" maps, which the row-band kernels serve (pure data;
make_golden_r3.py runs the real reference on them).  Inputs and gradients as cases.py describes: 7 x 7 is W = 2R + 1, the
heads' map; 14 x 14 takes three row bands.
"""
from cases import case

K7 = dict(R=3, padding=3)

R3_CASES = [
    case("r3_cos_reflect_2x8x7x7", (2, 8, 7, 7), dict(K7, measure="cosine"), 610),
    case("r3_l2_zeros_2x8x7x7", (2, 8, 7, 7), dict(K7, measure="norm", p=2, padding_mode="zeros"), 611),
    case("r3_cos_replicate_2x8x7x7", (2, 8, 7, 7), dict(K7, measure="cosine", padding_mode="replicate"), 612),
    case("r3_cos_reflect_1x8x14x14", (1, 8, 14, 14), dict(K7, measure="cosine"), 613),
]
R3_BY_NAME = {c["name"]: c for c in R3_CASES}
assert len(R3_BY_NAME) == len(R3_CASES)
