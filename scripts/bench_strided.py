#!/usr/bin/env python3
"""Time forward + backward of a stride-2 NFP layer on the strided row-band kernels (functional.nfp_strided) against
  off    the same call with NFP_STRIDED_OFF=1: the any-geometry kernels (fwd_pairs / bwd_gather) — the route of this call
         before nfp_strided existed
as a captured graph of 20 steps; five runs per arm, alternating in one process, device events, after warm-up (10 eager
steps per arm, then one replay before every timed run of 10 replays).  One JSON line per (shape, R, padding, measure,
dtype, layout): per arm the five times in us per fwd+bwd step, their median and spread (max - min), the ratio off /
strided of the medians, and `beats_off` — the medians differ by more than the larger of the two spreads.  The shapes are the
maps a strided nfp_at_layer / nfp_insert layer sees.  Then one NFPInsertNet(nfp_insert_idx=1) train step at [64,3,224,224]
with a stride-2 cosine insert, strided_layer on and off.  The arms' outputs are compared on the timed inputs first.

    python scripts/bench_strided.py [--out FILE] [--quick]      (--quick: R = 1, float32 NCHW only)
"""
import argparse
import itertools
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neighbour_feature_pooling_amd import NFPPooling, _abi, nfp_strided  # noqa: E402

SHAPES = [(64, 64, 56, 56), (64, 128, 28, 28), (64, 256, 14, 14), (64, 512, 7, 7), (64, 16, 112, 112), (64, 40, 28, 28)]
ARMS = ("strided", "off")
GRAPH_STEPS, RUNS, REPLAYS = 20, 5, 10


class arm_env:
    def __init__(self, arm):
        self.off = arm == "off"

    def __enter__(self):
        if self.off:
            os.environ["NFP_STRIDED_OFF"] = "1"

    def __exit__(self, *a):
        os.environ.pop("NFP_STRIDED_OFF", None)


def time_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def summary(times):
    med = {a: statistics.median(t) for a, t in times.items()}
    spread = {a: max(t) - min(t) for a, t in times.items()}
    return dict(us={a: [round(v, 2) for v in t] for a, t in times.items()}, median_us={a: round(v, 2) for a, v in med.items()},
                spread_us={a: round(v, 2) for a, v in spread.items()}, ratio_off_over_strided=round(med["off"] / med["strided"], 3),
                beats_off=bool(med["off"] - med["strided"] > max(spread.values())),
                loses_to_off=bool(med["strided"] - med["off"] > max(spread.values())))


def bench_shape(shape, R, pad, measure, dtype, nhwc):
    dev = torch.device("cuda:0")
    kw = dict(R=R, measure=measure, padding=pad, stride=2)
    if measure == "norm":
        kw["p"] = 2
    cfg = NFPPooling(shape[1], **kw).config
    torch.manual_seed(1)
    x = torch.randn(shape, device=dev).to(dtype)
    if nhwc:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    L = _abi.load()

    def step():
        return torch.autograd.grad(nfp_strided(x, cfg), x, go)[0]
    with torch.no_grad():
        oshape = nfp_strided(x, cfg).shape
    go = torch.randn(oshape, device=dev).to(dtype)
    variants, graphs, results = {}, {}, {}
    for arm in ARMS:
        with arm_env(arm):
            for _ in range(10):
                results[arm] = step()
            torch.cuda.synchronize()
            variants[arm] = L.nfp_last_variant().decode()
    # the arms compute the same gradient (relative to the tensor's max; reordered sums differ in the last bits)
    ref = results["off"].float()
    diff = float((results["strided"].float() - ref).abs().max() / ref.abs().max())
    for arm in ARMS:
        g = torch.cuda.CUDAGraph()
        with arm_env(arm):
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                step()
            torch.cuda.current_stream().wait_stream(s)
            with torch.cuda.graph(g):
                for _ in range(GRAPH_STEPS):
                    step()
        graphs[arm] = g
    times = {a: [] for a in ARMS}
    for _ in range(RUNS):
        for arm in ARMS:
            graphs[arm].replay()
            times[arm].append(time_us(graphs[arm].replay, REPLAYS) / GRAPH_STEPS)
    return dict(shape=list(shape), R=R, padding=pad, measure="l2" if measure == "norm" else measure,
                dtype=str(dtype).split(".")[1], layout="nhwc" if nhwc else "nchw", mode="graph", bwd_variant=variants,
                grad_x_rel_diff=diff, **summary(times))


def bench_insert_net():
    """One NFPInsertNet train step at [64,3,224,224], a stride-2 cosine insert (R = 1, padding 1) behind block 1: the layer
    sees [64,24,56,56]; strided_layer on / off."""
    from neighbour_feature_pooling_amd.models import NFPInsertNet
    dev = torch.device("cuda:0")
    x = torch.randn(64, 3, 224, 224, device=dev)
    y = torch.randint(0, 10, (64,), device=dev)
    steps = {}
    for arm, on in (("strided", True), ("off", False)):
        torch.manual_seed(0)
        m = NFPInsertNet(num_classes=10, nfp_insert_idx=1, nfp_kwargs=dict(measure="cosine", stride=2, padding=1),
                         strided_layer=on).to(dev)
        opt = torch.optim.SGD(m.parameters(), lr=0.01)

        def step(m=m, opt=opt):
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.cross_entropy(m(x), y).backward()
            opt.step()
        steps[arm] = step
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    times = {a: [] for a in steps}
    for _ in range(RUNS):
        for arm in steps:
            times[arm].append(time_us(steps[arm], 5))
    return dict(block="NFPInsertNet(nfp_insert_idx=1, cosine stride 2 padding 1) train step [64,3,224,224] f32", mode="eager",
                **summary(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_strided.py: no GPU")
    recs = []

    def emit(r):      # (a line as soon as it is measured)
        print(json.dumps(r), flush=True)
        recs.append(r)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(json.dumps(q) for q in recs) + "\n")
    radii = (1,) if args.quick else (1, 2)
    stores = ((torch.float32, False),) if args.quick else tuple(itertools.product((torch.float32, torch.bfloat16), (False, True)))
    for shape in SHAPES:
        for R, padded, measure, (dtype, nhwc) in itertools.product(radii, (False, True), ("cosine", "norm"), stores):
            emit(bench_shape(shape, R, R if padded else 0, measure, dtype, nhwc))
    emit(bench_insert_net())


if __name__ == "__main__":
    main()
