"""Golden-vector cases of the three trained heads — NFPHead, MultiRadiusNFPHead, AdaptiveFusionNFP (pure data;
make_golden_heads.py runs the real reference on them).

The input is regenerated bit-exactly from (shape, seed) with synth.feature_map, the gradient of the head's output with
make_grad_out; the parameters are the ones the reference drew under torch.manual_seed(seed) and are stored in the fixture.
A case: <cls>(<in-channel keyword>=shape[1], **ctor) on an input [B, C, H, W], one step in train mode (or, train=False, in
eval()).  MultiRadiusNFPHead and AdaptiveFusionNFP add the compressed vector to GAP(x): bottleneck_dim == C there.
"""

# the keyword the class takes its input channels by (nfp_heads.py:16, 85, 287)
IN_KW = {"NFPHead": "in_c", "MultiRadiusNFPHead": "in_c", "AdaptiveFusionNFP": "in_channels"}


def hcase(name, cls, shape, ctor, seed, train=True):
    return dict(name=name, cls=cls, shape=tuple(shape), ctor=dict(ctor), seed=seed, train=train)


HEAD_CASES = [
    hcase("head_nfp_4x16x7x7", "NFPHead", (4, 16, 7, 7), dict(bottleneck_dim=24), 500),
    hcase("head_multi_radius_4x16x7x7", "MultiRadiusNFPHead", (4, 16, 7, 7), dict(bottleneck_dim=16), 501),
    hcase("head_adaptive_4x16x7x7", "AdaptiveFusionNFP", (4, 16, 7, 7), dict(bottleneck_dim=16, dropout_p=0.0), 502),
    hcase("head_nfp_eval_4x16x7x7", "NFPHead", (4, 16, 7, 7), dict(bottleneck_dim=24), 500, train=False),
]
HEAD_BY_NAME = {c["name"]: c for c in HEAD_CASES}
assert len(HEAD_BY_NAME) == len(HEAD_CASES)

# init-only fixtures: (name, class, in channels, ctor, seed) -> every parameter the class draws under manual_seed(seed)
HEAD_INIT_CASES = [
    ("head_init_nfp_c12", "NFPHead", 12, dict(bottleneck_dim=20), 31),
    ("head_init_multi_radius_c8", "MultiRadiusNFPHead", 8, dict(bottleneck_dim=8), 32),
    ("head_init_adaptive_c8_r2", "AdaptiveFusionNFP", 8, dict(bottleneck_dim=8, R=2), 33),
]


def make_input(c):
    from neighbour_feature_pooling_amd.synth import feature_map
    return feature_map(c["shape"], c["seed"], "normal")


def make_grad_out(c, out_shape):
    from neighbour_feature_pooling_amd.synth import feature_map
    return feature_map(tuple(out_shape), c["seed"] + 1000, "normal")
