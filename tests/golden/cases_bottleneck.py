"""Golden-vector cases of NFPBottleneck (pure data; make_golden_bottleneck.py runs the real reference on them).

The input is regenerated bit-exactly from (shape, seed) with synth.feature_map, the gradient of the block's output with
make_grad_out; the parameters are the ones the reference drew under torch.manual_seed(seed) and are stored in the fixture.
A case: NFPBottleneck(cin, cout, stride) on an input [B, cin, H, W], one step in train mode (or, train=False, in eval()).
"""


def bcase(name, shape, cout, stride, seed, train=True):
    return dict(name=name, shape=tuple(shape), cin=shape[1], cout=cout, stride=stride, seed=seed, train=train)


BNECK_CASES = [
    bcase("bneck_s1_down_4x16x9x9", (4, 16, 9, 9), 32, 1, 400),            # -> 7 x 7, downsample conv + BN
    bcase("bneck_s1_ident_2x32x7x7", (2, 32, 7, 7), 32, 1, 401),           # -> 5 x 5, downsample is Identity
    bcase("bneck_s2_4x16x12x12", (4, 16, 12, 12), 32, 2, 402),             # -> 4 x 4, _match with k = 9
    bcase("bneck_nonsquare_2x16x9x11", (2, 16, 9, 11), 32, 1, 403),        # -> 7 x 9
    bcase("bneck_probe_2x16x5x5", (2, 16, 5, 5), 32, 1, 404),              # the probe's own size -> 3 x 3
    bcase("bneck_eval_4x16x9x9", (4, 16, 9, 9), 32, 1, 400, train=False),  # eval() mode of the first case
]
BNECK_BY_NAME = {c["name"]: c for c in BNECK_CASES}
assert len(BNECK_BY_NAME) == len(BNECK_CASES)

# init-only fixtures: (name, in_channels, out_channels, stride, seed) -> every parameter NFPBottleneck draws under manual_seed(seed)
BNECK_INIT_CASES = [
    ("bneck_init_16_32_s1", 16, 32, 1, 21),
    ("bneck_init_24_24_s2", 24, 24, 2, 22),
]


def make_input(c):
    from neighbour_feature_pooling_amd.synth import feature_map
    return feature_map(c["shape"], c["seed"], "normal")


def make_grad_out(c, out_shape):
    from neighbour_feature_pooling_amd.synth import feature_map
    return feature_map(tuple(out_shape), c["seed"] + 1000, "normal")
