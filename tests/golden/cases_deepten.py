"""Golden-vector cases of DeepTENEncoding (pure data; make_golden_deepten.py runs the real reference on them).

The input and the gradient of the output are regenerated bit-exactly from (shape, seed) with make_x / make_grad_out.  The
parameters are the ones the reference drew under torch.manual_seed(seed) — or, params="synth", the ones make_synth_params
gives — and are stored in the fixture either way.
"""
import numpy as np


def dcase(name, shape, K, seed, x_scale=1.0, params="init"):
    return dict(name=name, shape=tuple(shape), K=K, seed=seed, x_scale=x_scale, params=params)


DEEPTEN_CASES = [
    dcase("deepten_3x20x3x3_k5", (3, 20, 3, 3), 5, 400),
    dcase("deepten_2x37x5x3_k7", (2, 37, 5, 3), 7, 401),
    dcase("deepten_2x64x5x5_k32", (2, 64, 5, 5), 32, 402, x_scale=0.3),
    dcase("deepten_2x192x4x4_k32_synth", (2, 192, 4, 4), 32, 403, params="synth"),   # spread assignments
    dcase("deepten_5x8x1x1_k3", (5, 8, 1, 1), 3, 404),                                # N = 1
]
DEEPTEN_BY_NAME = {c["name"]: c for c in DEEPTEN_CASES}
assert len(DEEPTEN_BY_NAME) == len(DEEPTEN_CASES)

# init-only fixtures: (name, D, K, seed) -> the parameters DeepTENEncoding(D, K) draws under manual_seed(seed)
DEEPTEN_INIT_CASES = [
    ("deepten_init_d512_k32", 512, 32, 9),
    ("deepten_init_d7_k3", 7, 3, 10),
]


def make_x(c):
    from neighbour_feature_pooling_amd.synth import feature_map
    return (feature_map(c["shape"], c["seed"], "normal") * np.float32(c["x_scale"])).astype(np.float32)


def make_grad_out(c):
    from neighbour_feature_pooling_amd.synth import feature_map
    return feature_map((c["shape"][0], c["K"] * c["shape"][1]), c["seed"] + 2000, "normal")


def make_synth_params(c):
    """codewords = 0.5 * N(0,1) [K,D], scale = -U(0,1) * 16 / D [K]: assignments spread over the codewords."""
    from neighbour_feature_pooling_amd.synth import feature_map
    D, K = c["shape"][1], c["K"]
    cw = (feature_map((K, D), c["seed"] + 3000, "normal") * np.float32(0.5)).astype(np.float32)
    u = (feature_map((K,), c["seed"] + 3001, "uniform").astype(np.float64) + 1.0) / 2.0
    return cw, (-u * 16.0 / D).astype(np.float32)
