#!/usr/bin/env python3
"""Radius-3 (7 x 7 window) "same" maps on the row-band kernels (NFP_TILE_R3=1: fwd_tile<R3,...> / bwd_tile<R3,...>) against
the any-geometry kernels that served them before (NFP_TILE_R3=0: fwd_pairs / bwd_gather) on the same GPU and build: forward +
backward of the layer, of nfp_with_gap, and of a whole NFPHead(R=3) / MultiRadiusNFPHead(R_list=(1, 2, 3)) step (rows 10 and
11 of scripts/bench_heads.py), each captured into a CUDA graph and replayed (bench_heads.graph_us: kernels alone).
Both arms run in one process, alternating, --runs times each.  One JSON line per row, microseconds: each arm's graph times,
their median and spread (max - min), the variants that ran, and `not_slower`: the row-band arm's median is not above the
other's by more than both spreads — the rule the default routing of csrc/nfp_launch.h::tile_r3_wanted follows.

    python scripts/bench_r3.py [--replays 50 --runs 3] [--rows 0,1,2,...]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import torch

from bench_heads import graph_us

#        what        shape               layer ctor                              dtype      channels-last
ROWS = [("layer", (64, 512, 7, 7), dict(measure="cosine"), "f32", False),
        ("layer", (256, 512, 7, 7), dict(measure="cosine"), "f32", False),
        ("layer", (64, 512, 7, 7), dict(measure="cosine"), "bf16", True),
        ("layer", (256, 192, 14, 14), dict(measure="norm", p=2), "f32", False),
        ("layer", (64, 40, 28, 28), dict(measure="cosine"), "f32", False),
        ("with_gap", (64, 512, 7, 7), dict(measure="cosine"), "f32", False),
        ("NFPHead", (64, 512, 7, 7), dict(R=3), "f32", False),
        ("MultiRadiusNFPHead", (64, 512, 7, 7), dict(R_list=(1, 2, 3)), "f32", False),
        # where the default routing's size rule lies (rows 8 to 13): between the B = 64 and B = 256 rows above
        ("layer", (128, 512, 7, 7), dict(measure="cosine"), "f32", False),
        ("layer", (192, 512, 7, 7), dict(measure="cosine"), "f32", False),
        ("layer", (64, 64, 7, 7), dict(measure="cosine"), "f32", False),
        ("layer", (64, 192, 14, 14), dict(measure="norm", p=2), "f32", False),
        ("layer", (16, 40, 28, 28), dict(measure="cosine"), "f32", False),
        ("with_gap", (256, 512, 7, 7), dict(measure="cosine"), "f32", False)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rows", default=",".join(str(i) for i in range(len(ROWS))))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_r3.py measures on the GPU; there is no CPU timing"
    import neighbour_feature_pooling_amd as pkg
    from neighbour_feature_pooling_amd import NFPPooling, _abi, functional, nfp_with_gap
    dev = torch.device("cuda:0")
    L = _abi.load()
    for i in (int(s) for s in a.rows.split(",")):
        what, shape, ctor, dt, cl = ROWS[i]
        torch.manual_seed(0)
        x = torch.randn(shape, device=dev).to(torch.bfloat16 if dt == "bf16" else torch.float32)
        if cl:
            x = x.contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        seen = {}
        if what in ("layer", "with_gap"):
            layer = NFPPooling(shape[1], R=3, padding=3, **ctor)
            go = torch.randn(shape[0], 48, shape[2], shape[3], device=dev).to(x.dtype)
            gg = torch.randn(shape[:2], device=dev)

            def step():
                if what == "layer":
                    out = layer(x)
                    seen["fwd"] = L.nfp_last_variant().decode()
                    r = torch.autograd.grad(out, x, go)
                else:
                    gap, maps = nfp_with_gap(x, layer.config)
                    seen["fwd"] = L.nfp_last_variant().decode()
                    r = torch.autograd.grad((gap, maps), x, (gg, go))
                seen["bwd"] = L.nfp_last_variant().decode()
                return r
        else:
            head = getattr(pkg, what)(in_c=shape[1], bottleneck_dim=512, **ctor).to(dev)
            go = torch.randn(shape[0], 512, device=dev)
            leaves = (x,) + tuple(p for p in head.parameters() if p.requires_grad)

            def step():
                return torch.autograd.grad(head(x), leaves, go)

        def arm(on):
            os.environ["NFP_TILE_R3"] = "1" if on else "0"
            L.nfp_reload_env()
            functional._PLANS.clear()      # (a cached plan carries what the library answered under the other arm)
            n0 = L.nfp_launch_count()
            step()
            torch.cuda.synchronize()
            launches = int(L.nfp_launch_count() - n0)
            return graph_us(step, a.replays), launches, dict(seen)

        res = {True: [], False: []}
        for _ in range(a.runs):
            for on in (True, False):
                res[on].append(arm(on))
        os.environ.pop("NFP_TILE_R3", None)
        L.nfp_reload_env()
        functional._PLANS.clear()
        med = lambda v: sorted(v)[len(v) // 2]     # noqa: E731
        row = dict(row=i, what=what, shape=list(shape), dtype=dt, channels_last=cl,
                   **{k: list(v) if isinstance(v, tuple) else v for k, v in ctor.items()})
        for on, name in ((True, "tile"), (False, "general")):
            ts = [round(t[0], 2) for t in res[on]]
            row.update({name + "_graph_us": ts, name + "_median_us": med(ts), name + "_spread_us": round(max(ts) - min(ts), 2),
                        name + "_nfp_launches": res[on][-1][1], name + "_variants": res[on][-1][2]})
        row.update(speedup=round(row["general_median_us"] / row["tile_median_us"], 3),
                   not_slower=bool(row["tile_median_us"] <= row["general_median_us"] + row["tile_spread_us"] + row["general_spread_us"]))
        print(json.dumps(row), flush=True)
        del x, go
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
