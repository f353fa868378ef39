#!/usr/bin/env python3
"""The bits of the any-geometry backward (csrc/nfp_gather.h: bwd_gather, bwd_gather_banded) and of the biased backward
(csrc/nfp_bias.hip), which shares its coefficient tables' helpers: a fixed table of tiny cases made on the CPU from fixed
seeds, each run under NFP_FORCE_GENERIC=1 with no other switch and again under NFP_BWD_BANDS=3, a SHA-256 per gradient.
Two builds that claim to compute the same thing (a refactor of the kernels and its parent) are run once each and
compared: every sum of these kernels runs in a fixed order, so every digest must agree.

    python scripts/gather_bits.py --out new.json [--against parent.json]      (exit 1 on any difference)

Hashed per case and setting: grad_x, with bias=True also grad_centre_bias / grad_neighbour_bias; beside them the name of
the kernel that served the backward.  The cases: the four padding modes; stride 2 with pad = R*dil + 1 (pixels that are
the centre of no output or of several); dilation 2; a W = 1 map under replicate padding (2*pad + 1 padded coordinates fold
onto one); H = 7 on three bands (a short last band); C = 3, 5, 13 (ragged channel quads); channels-last; bf16, and bf16
with float32 maps (map_f32 = 1, the native autocast call); one measure per coefficient count (norm p = 3: 1, smith: 3,
pearson: 5); Attention on bf16; bias=True with cosine and pearson."""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

# (name, shape, layer arguments, flags: "nhwc", "bf16", "mix" = bf16 under autocast with float32 maps)
CASES = [
    ("reflect_cosine", (2, 8, 9, 8), dict(R=1, measure="cosine", padding=1, padding_mode="reflect"), ()),
    ("zeros_chisquared2", (2, 8, 9, 8), dict(R=1, measure="chisquared2", padding=1, padding_mode="zeros"), ()),
    ("replicate_norm1", (2, 8, 9, 8), dict(R=1, measure="norm", p=1, padding=1, padding_mode="replicate"), ()),
    ("circular_dot", (2, 8, 9, 8), dict(R=1, measure="dot", padding=1, padding_mode="circular"), ()),
    ("stride2_overpad", (2, 8, 9, 8), dict(R=1, measure="cosine", padding=2, stride=2, padding_mode="reflect"), ()),
    ("stride2_overpad_zeros_R2", (1, 4, 11, 10), dict(R=2, measure="canberra", padding=5, stride=2, dilation=2,
                                                      padding_mode="zeros"), ()),
    ("dilation2", (2, 8, 9, 8), dict(R=1, measure="gfc", padding=2, dilation=2, padding_mode="reflect"), ()),
    ("w1_replicate", (2, 8, 8, 1), dict(R=1, measure="cosine", padding=1, padding_mode="replicate"), ()),
    ("h7_three_bands", (2, 8, 7, 7), dict(R=1, measure="emd", padding=1), ()),
    ("pad0_norm1", (2, 8, 7, 7), dict(R=1, measure="norm", p=1, padding=0), ()),
    ("c3", (2, 3, 7, 6), dict(R=1, measure="cosine", padding=1), ()),
    ("c5", (2, 5, 7, 6), dict(R=1, measure="geman", padding=1, padding_mode="zeros"), ()),
    ("c13_two_quad_blocks", (1, 13, 6, 7), dict(R=2, measure="norm", p=2, padding=2), ()),
    ("c67_nhwc", (3, 67, 7, 9), dict(R=1, measure="cosine", padding=1), ("nhwc",)),
    ("nhwc_stride2", (2, 8, 9, 8), dict(R=1, measure="hellinger", padding=1, stride=2, padding_mode="replicate"), ("nhwc",)),
    ("bf16", (2, 8, 9, 8), dict(R=1, measure="cosine", padding=0), ("bf16",)),
    ("bf16_nhwc_c5", (2, 5, 9, 8), dict(R=1, measure="norm", p=1, padding=1, padding_mode="circular"), ("bf16", "nhwc")),
    ("bf16_map_f32", (2, 8, 9, 9), dict(R=1, measure="cosine", padding=1, stride=2), ("mix",)),
    ("bf16_map_f32_nhwc", (2, 6, 7, 7), dict(R=1, measure="canberra", padding=1), ("mix", "nhwc")),
    ("ncoef1_norm3", (2, 8, 9, 8), dict(R=1, measure="norm", p=3, padding=1), ()),
    ("ncoef3_smith", (2, 8, 9, 8), dict(R=1, measure="smith", padding=1), ()),
    ("ncoef5_pearson", (2, 8, 9, 8), dict(R=1, measure="pearson", padding=2, dilation=2), ()),
    ("attention_bf16", (2, 8, 9, 8), dict(R=1, measure="attention", padding=1), ("bf16",)),
    ("bias_cosine", (2, 6, 7, 8), dict(R=1, measure="cosine", padding=1, bias=True), ()),
    ("bias_pearson_stride2", (2, 5, 9, 8), dict(R=1, measure="pearson", padding=2, stride=2, padding_mode="zeros",
                                                bias=True), ("nhwc",)),
]
SETTINGS = ("", "NFP_BWD_BANDS=3")


def digest(t):
    t = t.detach().cpu().contiguous()
    raw = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
    return hashlib.sha256(raw.numpy().tobytes()).hexdigest()


def run_case(L, case, dev):
    from neighbour_feature_pooling_amd import NFPPooling
    name, shape, ctor, flags = case
    seed = int(hashlib.sha256(name.encode()).hexdigest()[:6], 16)
    torch.manual_seed(seed)        # (bias=True draws its biases from the global generator)
    layer = NFPPooling(shape[1], **ctor).to(dev)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(*shape, generator=g) + 0.25      # positive: valid for every measure
    low = "bf16" in flags or "mix" in flags
    x = x.to(dev).to(torch.bfloat16 if low else torch.float32)
    if "nhwc" in flags:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16, enabled="mix" in flags):
        out = layer(x)
    assert out.dtype == (torch.float32 if "mix" in flags else x.dtype), (name, out.dtype)
    go = torch.randn(out.shape, generator=g).to(dev).to(out.dtype)
    params = list(layer.parameters())
    grads = torch.autograd.grad(out, [x] + params, go)
    res = dict(grad_x=digest(grads[0]), variant=L.nfp_last_variant().decode())
    if ctor.get("bias"):
        named = dict(zip((n for n, _ in layer.named_parameters()), grads[1:]))
        res["grad_centre_bias"] = digest(named["center_value.bias"])
        res["grad_neighbour_bias"] = digest(named["comp_neighbors.bias"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--against")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gather_bits.py runs the kernels; it needs the GPU"
    from neighbour_feature_pooling_amd import _abi
    L = _abi.load()
    dev = torch.device("cuda:0")
    os.environ["NFP_FORCE_GENERIC"] = "1"
    os.environ["NFP_AMP_NATIVE"] = "1"     # (the map_f32 cases: the native autocast call is opt-in)
    got = {}
    for s in SETTINGS:
        os.environ.pop("NFP_BWD_BANDS", None)
        if s:
            os.environ.update([s.split("=", 1)])
        L.nfp_reload_env()
        for c in CASES:
            got["%s[%s]" % (c[0], s)] = run_case(L, c, dev)
    torch.cuda.synchronize()
    with open(a.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
    n = sum(len(v) for v in got.values())
    print("%d runs, %d entries -> %s" % (len(got), n, a.out))
    for v in sorted({r["variant"] for r in got.values()}):
        print("  %3d x %s" % (sum(r["variant"] == v for r in got.values()), v))
    if not a.against:
        return 0
    with open(a.against) as f:
        ref = json.load(f)
    bad = [(c, t) for c in sorted(set(got) | set(ref)) for t in sorted(set(got.get(c, {})) | set(ref.get(c, {})))
           if got.get(c, {}).get(t, "missing") != ref.get(c, {}).get(t, "missing")]
    for c, t in bad:
        print("DIFFERS %s %s" % (c, t))
    print("%d of %d entries differ from %s" % (len(bad), n, a.against))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
