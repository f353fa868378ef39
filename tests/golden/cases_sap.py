"""Golden-vector cases of SimilarityAwarePooling (pure data; make_golden_sap.py runs the real reference on them).

The input is regenerated bit-exactly from (shape, seed, kind) with cases.make_input, the gradient of the pooled vector
with make_grad_pooled; att_proj's parameters are the ones the reference drew under torch.manual_seed(seed) and are
stored in the fixture.  ctor = keyword arguments of SimilarityAwarePooling(in_channels=C, **ctor).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cases import case  # noqa: E402

SAP_CASES = [
    case("sap_cos_r1_2x16x7x7", (2, 16, 7, 7), dict(R=1, measure="cosine"), 300),
    case("sap_l2_r2_3x8x9x8", (3, 8, 9, 8), dict(R=2, measure="norm", p=2), 301),          # N = 24, maps 5 x 4
    case("sap_norm_p1_default_2x8x7x7", (2, 8, 7, 7), dict(R=1, measure="norm"), 302),      # NFPPooling's default p = 1
    case("sap_cos_bias_2x8x7x6", (2, 8, 7, 6), dict(R=1, measure="cosine", bias=True), 303),
    case("sap_cos_one_pixel_2x8x3x3", (2, 8, 3, 3), dict(R=1, measure="cosine"), 304),      # P = 1: pooled is the map, gw = 0
]
SAP_BY_NAME = {c["name"]: c for c in SAP_CASES}
assert len(SAP_BY_NAME) == len(SAP_CASES)

# init-only fixtures: (name, C, ctor, seed) -> the att_proj parameters SimilarityAwarePooling(C, **ctor) draws under
# manual_seed(seed) — behind the 7 x 7 probe the constructor draws first
SAP_INIT_CASES = [
    ("sap_init_c5_r1_cosine", 5, dict(R=1, measure="cosine"), 9),
    ("sap_init_c4_r2_norm_bias", 4, dict(R=2, measure="norm", bias=True), 10),
]


def make_grad_pooled(c, n_maps):
    from neighbour_feature_pooling_amd.synth import feature_map
    return feature_map((c["shape"][0], n_maps), c["seed"] + 2000, "normal")
