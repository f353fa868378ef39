#!/usr/bin/env python3
"""SimilarityAwarePooling: forward + backward time of the module with the HIP softmax-pool tail (csrc/nfp_attpool.hip)
against the same module with the torch tail (NFP_SAP_TORCH=1, read at call time) on the same build.  Both arms run in one
process, alternating, --runs times each; a run is the median of per-iteration device-event times (milliseconds) over
--iters eager steps after --warmup, no graph capture.  A step is the module's forward and torch.autograd.grad of the pooled
vector with respect to x and att_proj's two parameters.  One JSON line per shape; `margin` is the spread (max - min) of the
torch arm's runs, and `faster` says whether the HIP arm's slowest run beats the torch arm's fastest by more than it.

    python scripts/bench_sap.py [--iters 20 --warmup 5 --runs 3] [--shapes 0,1,2,3]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

SHAPES = [  # (B, C, H, W), SimilarityAwarePooling kwargs, dtype, channels-last
    ((64, 512, 7, 7), dict(R=1, measure="cosine"), torch.float32, False),
    ((256, 192, 14, 14), dict(R=2, measure="norm", p=2), torch.bfloat16, True),
    ((256, 24, 56, 56), dict(R=1, measure="cosine"), torch.float32, False),
    ((4, 16, 112, 112), dict(R=1, measure="cosine"), torch.float32, False),   # few images, long rows
]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--shapes", default="0,1,2,3")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sap.py measures on the GPU; there is no CPU timing"
    from neighbour_feature_pooling_amd import SimilarityAwarePooling, _abi
    dev = torch.device("cuda:0")
    for i in (int(s) for s in a.shapes.split(",")):
        shape, kw, dtype, cl = SHAPES[i]
        torch.manual_seed(0)
        x = torch.randn(shape, device=dev).to(dtype)
        if cl:
            x = x.contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        m = SimilarityAwarePooling(shape[1], **kw).to(dev)
        leaves = (x, m.att_proj.weight, m.att_proj.bias)
        gp = torch.randn(shape[0], m.nfp_channels, device=dev).to(dtype)

        def step():
            return torch.autograd.grad(m(x), leaves, gp)

        def arm(torch_tail):
            if torch_tail:
                os.environ["NFP_SAP_TORCH"] = "1"
            else:
                os.environ.pop("NFP_SAP_TORCH", None)
            n0 = _abi.load().nfp_launch_count()
            step()
            launches = _abi.load().nfp_launch_count() - n0
            return timed(step, a.iters, a.warmup), launches

        hip, tail = [], []
        for _ in range(a.runs):
            t, hip_launches = arm(False)
            hip.append(round(t, 4))
            t, tail_launches = arm(True)
            tail.append(round(t, 4))
        os.environ.pop("NFP_SAP_TORCH", None)
        margin = max(tail) - min(tail)
        print(json.dumps(dict(shape=list(shape), kw=kw, dtype=str(dtype).split(".")[-1], channels_last=cl,
                              maps=list(m.nfp(x.detach()).shape), hip_tail_ms=hip, torch_tail_ms=tail,
                              hip_median_ms=sorted(hip)[len(hip) // 2], torch_median_ms=sorted(tail)[len(tail) // 2],
                              margin_ms=round(margin, 4), faster=bool(min(tail) - max(hip) > margin),
                              nfp_launches_hip_arm=int(hip_launches), nfp_launches_torch_arm=int(tail_launches))), flush=True)
        del x, gp, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
