#!/usr/bin/env python3
"""The heads' tail GAP(relu(bn(conv1x1(maps)))) on the HIP kernels (csrc/nfp_cpool.hip) against the torch composition of the
same call (NFP_CPOOL_TORCH=1, read at call time: conv2d, batch_norm, relu, mean — the parent's path; the HIP arm runs with
NFP_CPOOL_TORCH=0, the HIP tail wherever it can serve) on the same GPU and build, forward + backward in train mode; and a
whole NFPHead step on [64,512,7,7] features the same way.
Both arms run in one process, alternating, --runs times each.  One JSON line per row, microseconds:
  eager   median of per-step device-event times over --iters steps after --warmup (host launch gaps included)
  graph   the step captured into a CUDA graph, replayed --replays times between two events, per replay (kernels alone)
  peak    torch.cuda.max_memory_allocated over one step, above what was allocated before it (bytes)
`margin` is the spread (max - min) of the composition arm's graph runs; `faster` says whether the HIP arm's slowest graph
run beats the composition's fastest by more than it.
Rows 6 to 11 are the wide form of the tail (the cpw kernels, 33 to 96 maps: what NFP_CPOOL_TORCH=0 runs there): four tail
shapes, then an NFPHead(R=3) step and a MultiRadiusNFPHead(R_list=(1, 2, 3)) step on [64,512,7,7].  Rows 12 to 14 add a third
arm, `wide` (NFP_CPOOL_TORCH=0 with NFP_CPOOL_WIDE=1: the wide form at 16, 24 and 32 maps), beside the register form (`hip`) and
the composition; `wide_vs_hip` and `wide_vs_torch` are ratios of graph medians, `wide_spread_us` / `hip_spread_us` each arm's
max - min.

    python scripts/bench_heads.py [--iters 20 --warmup 5 --replays 50 --runs 3] [--rows 0,1,2,3,4,5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

D = 512
TAIL_SHAPES = [(64, 8, 7, 7), (256, 8, 7, 7), (256, 32, 7, 7), (256, 8, 14, 14), (64, 8, 56, 56)]   # maps [B,N,H,W]
HEAD_SHAPE = (64, 512, 7, 7)                                                                          # features, row 5
WIDE_TAIL_SHAPES = [(64, 48, 7, 7), (256, 48, 7, 7), (256, 80, 7, 7), (64, 48, 14, 14)]                # rows 6 to 9
WIDE_HEADS = [("NFPHead", dict(R=3)), ("MultiRadiusNFPHead", dict(R_list=(1, 2, 3)))]                  # rows 10, 11
WIDE_SWITCH_SHAPES = [(256, 16, 7, 7), (256, 24, 7, 7), (256, 32, 7, 7)]                               # rows 12 to 14
ROW_SHAPES = TAIL_SHAPES + [HEAD_SHAPE] + WIDE_TAIL_SHAPES + [HEAD_SHAPE] * len(WIDE_HEADS) + WIDE_SWITCH_SHAPES


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


def peak_bytes(step):
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rows", default="0,1,2,3,4,5")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_heads.py measures on the GPU; there is no CPU timing"
    import neighbour_feature_pooling_amd as pkg
    from neighbour_feature_pooling_amd import NFPHead, _abi, nfp_compress_pool
    dev = torch.device("cuda:0")
    L = _abi.load()
    for i in (int(s) for s in a.rows.split(",")):
        torch.manual_seed(0)
        first_wide_head = len(TAIL_SHAPES) + 1 + len(WIDE_TAIL_SHAPES)
        is_head = i == len(TAIL_SHAPES) or first_wide_head <= i < first_wide_head + len(WIDE_HEADS)
        if not is_head:
            shape = ROW_SHAPES[i]
            x = torch.randn(shape, device=dev, requires_grad=True)
            conv = torch.nn.Conv2d(shape[1], D, 1, bias=False).to(dev)
            bn = torch.nn.BatchNorm2d(D).to(dev)
            go = torch.randn(shape[0], D, device=dev)
            leaves = (x, conv.weight, bn.weight, bn.bias)
            row = dict(what="tail", maps=list(shape), D=D)

            def step():
                return torch.autograd.grad(nfp_compress_pool(x, conv.weight, bn), leaves, go)
        else:
            shape = HEAD_SHAPE
            x = torch.randn(shape, device=dev, requires_grad=True)
            cls, ctor = ("NFPHead", {}) if i == len(TAIL_SHAPES) else WIDE_HEADS[i - first_wide_head]
            head = getattr(pkg, cls)(in_c=shape[1], bottleneck_dim=D, **ctor).to(dev)
            go = torch.randn(shape[0], D, device=dev)
            leaves = (x,) + tuple(p for p in head.parameters() if p.requires_grad)
            row = dict(what=cls + " step", features=list(shape), D=D, **{k: list(v) if isinstance(v, tuple) else v
                                                                         for k, v in ctor.items()})

            def step():
                return torch.autograd.grad(head(x), leaves, go)

        def arm(composition, wide=False):
            os.environ["NFP_CPOOL_TORCH"] = "1" if composition else "0"     # ("0": the HIP tail also where the default routes away)
            os.environ["NFP_CPOOL_WIDE"] = "1" if wide else "0"
            n0 = L.nfp_launch_count()
            step()
            launches = int(L.nfp_launch_count() - n0)
            return eager_us(step, a.iters, a.warmup), graph_us(step, a.replays), peak_bytes(step), launches

        third = i >= len(ROW_SHAPES) - len(WIDE_SWITCH_SHAPES)     # the NFP_CPOOL_WIDE=1 arm
        res = {False: [], True: [], "wide": []}
        for _ in range(a.runs):
            if third:
                res["wide"].append(arm(False, True))
            for composition in (False, True):
                res[composition].append(arm(composition))
        os.environ.pop("NFP_CPOOL_TORCH", None)
        os.environ.pop("NFP_CPOOL_WIDE", None)
        if i > len(TAIL_SHAPES):
            row["variant_of_hip_arm"] = "wide" if not third else "register"
        for composition, name in ((False, "hip"), (True, "torch")):
            r = res[composition]
            row[name + "_eager_us"] = [round(t[0], 2) for t in r]
            row[name + "_graph_us"] = [round(t[1], 2) for t in r]
            row[name + "_peak_bytes"] = r[-1][2]
            row[name + "_nfp_launches"] = r[-1][3]
        med = lambda v: sorted(v)[len(v) // 2]     # noqa: E731
        margin = max(row["torch_graph_us"]) - min(row["torch_graph_us"])
        row.update(margin_us=round(margin, 2), faster=bool(min(row["torch_graph_us"]) - max(row["hip_graph_us"]) > margin),
                   graph_speedup=round(med(row["torch_graph_us"]) / med(row["hip_graph_us"]), 3),
                   eager_speedup=round(med(row["torch_eager_us"]) / med(row["hip_eager_us"]), 3),
                   one_activation_bytes=shape[0] * D * shape[2] * shape[3] * 4,
                   hip_spread_us=round(max(row["hip_graph_us"]) - min(row["hip_graph_us"]), 2))
        if third:
            r = res["wide"]
            row.update(wide_eager_us=[round(t[0], 2) for t in r], wide_graph_us=[round(t[1], 2) for t in r],
                       wide_peak_bytes=r[-1][2], wide_nfp_launches=r[-1][3])
            row.update(wide_spread_us=round(max(row["wide_graph_us"]) - min(row["wide_graph_us"]), 2),
                       wide_vs_hip=round(med(row["hip_graph_us"]) / med(row["wide_graph_us"]), 3),
                       wide_vs_torch=round(med(row["torch_graph_us"]) / med(row["wide_graph_us"]), 3))
        print(json.dumps(row), flush=True)
        del x, go, leaves
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
