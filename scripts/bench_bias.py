#!/usr/bin/env python3
"""NFPPooling(bias=True): forward + backward time of the biased HIP kernels (csrc/nfp_bias.hip) against
  * the unbiased HIP path of the same layer (bias=False: the hot-path kernels), and
  * the torch formulation with biases (_host.nfp_host, autograd) on the same GPU.
One JSON line per shape: median of per-iteration device-event times (milliseconds) over --iters calls after --warmup.

    python scripts/bench_bias.py [--iters 20 --warmup 5] [--shapes 0,1,2]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

SHAPES = [  # (B, C, H, W), NFPPooling kwargs, dtype, channels-last
    ((64, 512, 7, 7), dict(R=1, measure="cosine", padding=1), torch.float32, False),
    ((256, 64, 56, 56), dict(R=1, measure="Norm", p=1, padding=1), torch.float32, False),
    ((256, 192, 14, 14), dict(R=2, measure="norm", p=2, padding=2), torch.bfloat16, True),
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
    ap.add_argument("--shapes", default="0,1,2")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bias.py measures on the GPU; there is no CPU timing"
    from neighbour_feature_pooling_amd import NFPPooling, _abi
    from neighbour_feature_pooling_amd._host import nfp_host
    dev = torch.device("cuda:0")
    for i in (int(s) for s in a.shapes.split(",")):
        shape, kw, dtype, cl = SHAPES[i]
        torch.manual_seed(0)
        x = torch.randn(shape, device=dev).to(dtype)
        if cl:
            x = x.contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        biased = NFPPooling(shape[1], bias=True, **kw).to(dev)
        plain = NFPPooling(shape[1], **kw).to(dev)
        go = torch.randn(biased(x).shape, device=dev).to(dtype)

        def step(fn):
            def run():
                x.grad = None
                biased.zero_grad(set_to_none=True)
                fn().backward(go)
            return run

        cb, nb = biased.center_value.bias, biased.comp_neighbors.bias
        t_hip = timed(step(lambda: biased(x)), a.iters, a.warmup)
        fwd_v, = [_abi.load().nfp_last_variant().decode()]
        t_plain = timed(step(lambda: plain(x)), a.iters, a.warmup)
        plain_v = _abi.load().nfp_last_variant().decode()
        t_torch = timed(step(lambda: nfp_host(x, biased.config, cb, nb)), max(3, a.iters // 4), 2)
        print(json.dumps(dict(shape=list(shape), kw=kw, dtype=str(dtype).split(".")[-1], channels_last=cl,
                              biased_hip_ms=round(t_hip, 4), unbiased_hip_ms=round(t_plain, 4), torch_biased_ms=round(t_torch, 4),
                              vs_torch=round(t_torch / t_hip, 2), vs_unbiased=round(t_hip / t_plain, 2),
                              biased_variant=fwd_v, unbiased_variant=plain_v)), flush=True)
        del x, go, biased, plain
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
