"""Golden-vector cases of the trained heads at more than 32 NFP maps — NFPHead(R=3): 48 maps; MultiRadiusNFPHead with
R_list=(1, 2, 3): 8 + 24 + 48 = 80 (pure data; make_golden_heads_wide.py runs the real reference on them).  Inputs, gradients
and parameters as cases_heads.py describes.  With seed 510 the float64 pre-activations of the compress tail keep
min|a| >= 1e-5 max|a| in training and in eval (1.2e-4 / 6.4e-5 for the R = 3 head, 1.5e-4 / 5.1e-5 for the three radii).
"""
from cases_heads import hcase

HEAD_WIDE_CASES = [
    hcase("head_nfp_r3_4x16x7x7", "NFPHead", (4, 16, 7, 7), dict(bottleneck_dim=24, R=3), 510),
    hcase("head_nfp_r3_eval_4x16x7x7", "NFPHead", (4, 16, 7, 7), dict(bottleneck_dim=24, R=3), 510, train=False),
    hcase("head_three_radii_4x16x7x7", "MultiRadiusNFPHead", (4, 16, 7, 7), dict(bottleneck_dim=16, R_list=(1, 2, 3)), 510),
]
HEAD_WIDE_BY_NAME = {c["name"]: c for c in HEAD_WIDE_CASES}
assert len(HEAD_WIDE_BY_NAME) == len(HEAD_WIDE_CASES)
# maps the compress tail of each case sees
HEAD_WIDE_MAPS = {"head_nfp_r3_4x16x7x7": 48, "head_nfp_r3_eval_4x16x7x7": 48, "head_three_radii_4x16x7x7": 80}
