"""Golden-vector cases of NFPPooling(bias=True) (pure data; make_golden_bias.py runs the real reference on them).

Inputs and output gradients are regenerated bit-exactly from (shape, seed, kind) with cases.make_input /
cases.make_grad_out; the biases are the ones the reference drew under torch.manual_seed(seed) and are stored in the
fixture.  ctor = keyword arguments of NFPPooling(in_channels=C, bias=True, **ctor).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cases import case  # noqa: E402

FULL = 16384   # out / grad_x stored in full up to this many elements, else a strided sample and per-image sums
SMALL = (2, 8, 6, 5)
MEASURES = ["norm", "cosine", "dot", "rmse", "geman", "attention", "emd", "canberra", "hellinger", "chisquared1",
            "chisquared2", "gfc", "pearson", "jeffrey", "squaredchord", "smith", "scs"]

BIAS_CASES = (
    [case(f"bias_m_{m}", SMALL, dict(R=1, measure=m, padding=1), 200 + i, full_limit=FULL) for i, m in enumerate(MEASURES)] +
    [
        case("bias_m_Norm_quirk", SMALL, dict(R=1, measure="Norm", padding=1), 230, full_limit=FULL),
        case("bias_zeros_cos", SMALL, dict(R=1, measure="cosine", padding=1, padding_mode="zeros"), 231, full_limit=FULL),
        case("bias_zeros_norm_p2", SMALL, dict(R=1, measure="norm", p=2, padding=1, padding_mode="zeros"), 232, full_limit=FULL),
        case("bias_zeros_pad2_pearson", SMALL, dict(R=1, measure="pearson", padding=2, padding_mode="zeros"), 233, full_limit=FULL),
        case("bias_pad0_default", (2, 8, 7, 7), dict(R=1), 234, full_limit=FULL),
        case("bias_pad0_cos", (2, 8, 7, 6), dict(R=1, measure="cosine", padding=0), 235, full_limit=FULL),
        case("bias_stride2_cos", (2, 8, 9, 9), dict(R=1, measure="cosine", padding=1, stride=2), 236, full_limit=FULL),
        case("bias_dil2_geman", (2, 8, 9, 8), dict(R=1, measure="geman", padding=2, dilation=2), 237, full_limit=FULL),
        case("bias_circular_smith", SMALL, dict(R=1, measure="smith", padding=1, padding_mode="circular"), 238, full_limit=FULL),
        case("bias_replicate_canberra", SMALL, dict(R=1, measure="canberra", padding=1, padding_mode="replicate"), 239,
             full_limit=FULL),
        case("bias_R2_gfc", (2, 8, 7, 6), dict(R=2, measure="gfc", padding=2), 240, full_limit=FULL),
        case("bias_R2_rmse", (2, 8, 7, 6), dict(R=2, measure="rmse", padding=2), 241, full_limit=FULL),
        case("bias_dissim_cos", SMALL, dict(R=1, measure="cosine", padding=1, similarity=False), 242, full_limit=FULL),
        case("bias_dissim_chisq2", SMALL, dict(R=1, measure="chisquared2", padding=1, similarity=False), 243, full_limit=FULL),
        case("bias_dissim_attention_zeros", SMALL, dict(R=1, measure="attention", padding=1, padding_mode="zeros",
                                                        similarity=False), 244, full_limit=FULL),
        case("bias_cos_4x64x14x14", (4, 64, 14, 14), dict(R=1, measure="cosine", padding=1), 245, full_limit=FULL),
        case("bias_norm_quirk_2x16x40x40", (2, 16, 40, 40), dict(R=1, measure="Norm", p=1, padding=1), 246, full_limit=FULL),
    ])
BIAS_BY_NAME = {c["name"]: c for c in BIAS_CASES}
assert len(BIAS_BY_NAME) == len(BIAS_CASES)

# init-only fixtures: (name, C, ctor, seed) -> the two biases NFPPooling(C, bias=True, **ctor) draws under manual_seed(seed)
INIT_CASES = [
    ("bias_init_c5_r1_cosine", 5, dict(R=1, measure="cosine", padding=1), 7),
    ("bias_init_c3_r2_norm", 3, dict(R=2, measure="Norm", padding=2), 8),
]
