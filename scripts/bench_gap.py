#!/usr/bin/env python3
"""nfp_with_gap (GAP(x) and the NFP maps from one pass, one backward kernel for both gradients) against the composition
an NFP head otherwise runs — x.mean((2, 3)) + nfp(x), autograd merging the two gradients — forward + backward, same GPU.
One JSON line per shape, two figures each way (microseconds):
  eager   median of per-step device-event times over --iters steps after --warmup (host launch gaps included)
  graph   the step captured into a CUDA graph, replayed --replays times between two events, per replay (kernels alone)

    python scripts/bench_gap.py [--iters 20 --warmup 5 --replays 50] [--shapes 0,1,2,3,4,5,6]   (rows 4-6: radii (1, 2) together)
"""
import argparse
import dataclasses
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

SHAPES = [  # (B, C, H, W), NFPPooling kwargs, dtype, channels-last
    ((64, 512, 7, 7), dict(R=1, measure="cosine", padding=1), torch.float32, False),
    ((256, 512, 7, 7), dict(R=1, measure="cosine", padding=1), torch.float32, True),
    ((256, 192, 14, 14), dict(R=2, measure="norm", p=2, padding=2), torch.bfloat16, True),
    ((256, 24, 56, 56), dict(R=1, measure="cosine", padding=1), torch.float32, False),
    # radii (1, 2) from one pass (MultiRadiusNFPHead; kwargs of the R = 2 layer, run with inner_R = 1): `composed` is
    # x.mean + the fused two-radius nfp_op — the best there was before, not two separate layers
    ((64, 512, 7, 7), dict(R=2, measure="cosine", padding=2), torch.float32, False, 1),
    ((256, 512, 7, 7), dict(R=2, measure="cosine", padding=2), torch.float32, True, 1),
    ((256, 192, 14, 14), dict(R=2, measure="norm", p=2, padding=2), torch.bfloat16, True, 1),
]


def eager_us(step, iters, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def graph_us(step, replays):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / replays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--shapes", default="0,1,2,3,4,5,6")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gap.py measures on the GPU; there is no CPU timing"
    from neighbour_feature_pooling_amd import NFPPooling, _abi, nfp_op, nfp_with_gap
    dev = torch.device("cuda:0")
    L = _abi.load()
    for i in (int(s) for s in a.shapes.split(",")):
        shape, kw, dtype, cl = SHAPES[i][:4]
        inner_R = SHAPES[i][4] if len(SHAPES[i]) > 4 else 0
        torch.manual_seed(0)
        x = torch.randn(shape, device=dev).to(dtype)
        if cl:
            x = x.contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        cfg = dataclasses.replace(NFPPooling(shape[1], **kw).config, inner_R=inner_R)
        gg = torch.randn(shape[:2], device=dev)
        go = torch.randn(nfp_op(x.detach(), cfg).shape, device=dev).to(dtype)

        def fused():
            x.grad = None
            gap, maps = nfp_with_gap(x, cfg)
            torch.autograd.backward([gap, maps], [gg, go])

        def composed():
            x.grad = None
            gap, maps = x.mean((2, 3)).float(), nfp_op(x, cfg)
            torch.autograd.backward([gap, maps], [gg, go])

        row = dict(shape=list(shape), kw=kw, dtype=str(dtype).split(".")[-1], channels_last=cl)
        if inner_R:
            row["radii"] = [inner_R, kw["R"]]
        for name, fn in (("fused", fused), ("composed", composed)):
            row[name + "_eager_us"] = round(eager_us(fn, a.iters, a.warmup), 2)
            n0 = L.nfp_launch_count()
            fn()
            row[name + "_nfp_launches"] = int(L.nfp_launch_count() - n0)
            row[name + "_bwd_variant"] = L.nfp_last_variant().decode()
            row[name + "_graph_us"] = round(graph_us(fn, a.replays), 2)
        row["eager_speedup"] = round(row["composed_eager_us"] / row["fused_eager_us"], 3)
        row["graph_speedup"] = round(row["composed_graph_us"] / row["fused_graph_us"], 3)
        print(json.dumps(row), flush=True)
        del x, go, gg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
