"""Golden-vector cases of stride 2 to 4 maps, which the strided row-band kernels serve (pure data; make_golden_strided.py
runs the real reference on them).  Inputs and gradients as cases.py describes.  No distance-zero pair among them (no rmse
under replicate: the reference spreads that NaN further than the oracle does).
"""
from cases import case

STRIDED_CASES = [
    case("strided_cos_r1_s2_p0_2x8x5x5", (2, 8, 5, 5), dict(R=1, measure="cosine", padding=0, stride=2), 620),
    case("strided_l2_r1_s2_reflect_2x8x8x8", (2, 8, 8, 8), dict(R=1, measure="norm", p=2, padding=1, stride=2), 621),
    case("strided_cos_r2_s3_zeros_2x8x9x9", (2, 8, 9, 9), dict(R=2, measure="cosine", padding=2, stride=3, padding_mode="zeros"), 622),
    case("strided_gfc_r1_s4_p0_2x8x7x7", (2, 8, 7, 7), dict(R=1, measure="gfc", padding=0, stride=4), 623),
    case("strided_dot_r2_s2_p0_2x8x7x7", (2, 8, 7, 7), dict(R=2, measure="dot", padding=0, stride=2), 624),
]
STRIDED_BY_NAME = {c["name"]: c for c in STRIDED_CASES}
assert len(STRIDED_BY_NAME) == len(STRIDED_CASES)
# fixtures of cases.py that lie inside the served set as well
EXISTING = ["geo_cos_stride2", "geo_l2_stride2_replicate"]
