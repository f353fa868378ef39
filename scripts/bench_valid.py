#!/usr/bin/env python3
"""Time forward + backward of an unpadded NFP layer on the valid-map kernels (functional.nfp_valid) against
  off    the same call with NFP_VALID_OFF=1: the any-geometry kernels (fwd_pairs / bwd_gather), the path before nfp_valid
  crop   the "same" kernels with the ring cropped, nfp(x, padding=R)[:, :, R:-R, R:-R] (cosine / L2 only: its gradient is
         wrong for rmse at R = 2)
eager and as a captured graph of 20 steps; three runs per arm, alternating in one process, device events, after warm-up.
One JSON line per (shape, mode): per arm the three times in us per fwd+bwd step, their median, and the margin — the
spread (max - min) of the `off` arm's three runs.  Then one NFPBottleneck(64, 256) train step at [64,64,56,56], both arms.

    python scripts/bench_valid.py [--out FILE] [--trace]      (--trace: a few steps per arm and shape, for a kernel trace)

--l1: the same for the L1 layer — NFPPooling's class defaults, Norm p = 1, which nfp_valid serves on fwd_valid<..l1..> /
bwd_valid<..l1..> — at the maps NFPInsertNet hands its insert, arms `valid` and `off` (NFP_VALID_OFF=1: fwd_pairs /
bwd_gather), then one NFPInsertNet train step at [64,3,224,224] with nfp_insert_idx 0 and 1, valid_layer on and off.
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neighbour_feature_pooling_amd import NFPBottleneck, NFPPooling, _abi, nfp_op, nfp_valid  # noqa: E402

SHAPES = [((256, 16, 56, 56), torch.float32, False), ((256, 32, 28, 28), torch.float32, False),
          ((256, 64, 14, 14), torch.float32, False), ((256, 128, 7, 7), torch.float32, False),
          ((256, 64, 14, 14), torch.bfloat16, True), ((64, 512, 7, 7), torch.float32, False)]
ARMS = ("valid", "off", "crop")
L1_SHAPES = [((64, 16, 112, 112), torch.float32, False), ((64, 24, 56, 56), torch.float32, False),
             ((64, 40, 28, 28), torch.float32, False), ((64, 80, 14, 14), torch.float32, False),
             ((64, 960, 7, 7), torch.float32, False), ((256, 16, 56, 56), torch.float32, False),
             ((64, 24, 56, 56), torch.bfloat16, True)]
L1_ARMS = ("valid", "off")
GRAPH_STEPS = 20


def step_fn(arm, x, go, cfg):
    R = cfg.R
    same = dataclasses.replace(cfg, padding=R)

    def step():
        if arm == "crop":
            out = nfp_op(x, same)[:, :, R:-R, R:-R]
        else:
            out = nfp_valid(x, cfg)
        return torch.autograd.grad(out, x, go)[0]
    return step


class arm_env:
    def __init__(self, arm):
        self.off = arm == "off"

    def __enter__(self):
        if self.off:
            os.environ["NFP_VALID_OFF"] = "1"

    def __exit__(self, *a):
        os.environ.pop("NFP_VALID_OFF", None)


def time_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def bench_shape(shape, dtype, nhwc, trace, measure="cosine", ARMS=ARMS):
    dev = torch.device("cuda:0")
    cfg = NFPPooling(shape[1], R=1, measure=measure, padding=0).config
    x = torch.randn(shape, device=dev).to(dtype)
    if nhwc:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    go = torch.randn(shape[0], 8, shape[2] - 2, shape[3] - 2, device=dev).to(dtype)
    L = _abi.load()
    steps, variants, graphs = {}, {}, {}
    for arm in ARMS:
        steps[arm] = step_fn(arm, x, go, cfg)
        with arm_env(arm):
            for _ in range(3 if trace else 10):
                steps[arm]()
            torch.cuda.synchronize()
            variants[arm] = L.nfp_last_variant().decode()
    if trace:
        return []
    for arm in ARMS:        # capture 20 steps per arm (each arm warmed up above)
        g = torch.cuda.CUDAGraph()
        with arm_env(arm):
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                steps[arm]()
            torch.cuda.current_stream().wait_stream(s)
            with torch.cuda.graph(g):
                for _ in range(GRAPH_STEPS):
                    steps[arm]()
        graphs[arm] = g
    recs = []
    for mode in ("eager", "graph"):
        times = {a: [] for a in ARMS}
        for _ in range(3):
            for arm in ARMS:
                with arm_env(arm):
                    if mode == "eager":
                        times[arm].append(time_us(steps[arm], 50))
                    else:
                        graphs[arm].replay()
                        times[arm].append(time_us(graphs[arm].replay, 10) / GRAPH_STEPS)
        margin = max(times["off"]) - min(times["off"])
        med = {a: statistics.median(t) for a, t in times.items()}
        recs.append(dict(shape=list(shape), dtype=str(dtype).split(".")[1], layout="nhwc" if nhwc else "nchw", mode=mode,
                         us={a: [round(v, 2) for v in t] for a, t in times.items()},
                         median_us={a: round(v, 2) for a, v in med.items()}, margin_us=round(margin, 2),
                         beats_off=bool(med["off"] - med["valid"] > margin),
                         beats_crop=bool(med["crop"] > med["valid"]) if "crop" in med else None, bwd_variant=variants))
        if measure != "cosine":
            recs[-1]["measure"] = measure
    return recs


def bench_block(trace):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = NFPBottleneck(64, 256).to(dev)
    opt = torch.optim.SGD(m.parameters(), lr=0.01)
    x = torch.randn(64, 64, 56, 56, device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        m(x).square().mean().backward()
        opt.step()
    times = {"valid": [], "off": []}
    for arm in times:
        with arm_env(arm):
            for _ in range(3):
                step()
    torch.cuda.synchronize()
    if trace:
        return []
    for _ in range(3):
        for arm in times:
            with arm_env(arm):
                times[arm].append(time_us(step, 10))
    return [dict(block="NFPBottleneck(64,256) train step [64,64,56,56] f32", mode="eager",
                 us={a: [round(v, 1) for v in t] for a, t in times.items()},
                 median_us={a: round(statistics.median(t), 1) for a, t in times.items()},
                 margin_us=round(max(times["off"]) - min(times["off"]), 1))]


def bench_insert_net(idx, trace):
    """One NFPInsertNet train step at [64,3,224,224] (the class-default L1 insert behind block `idx`): valid_layer on / off."""
    from neighbour_feature_pooling_amd.models import NFPInsertNet
    dev = torch.device("cuda:0")
    x = torch.randn(64, 3, 224, 224, device=dev)
    y = torch.randint(0, 10, (64,), device=dev)
    steps = {}
    for arm, on in (("valid", True), ("off", False)):
        torch.manual_seed(0)
        m = NFPInsertNet(num_classes=10, nfp_insert_idx=idx, valid_layer=on).to(dev)
        opt = torch.optim.SGD(m.parameters(), lr=0.01)

        def step(m=m, opt=opt):
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.cross_entropy(m(x), y).backward()
            opt.step()
        steps[arm] = step
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    if trace:
        return []
    times = {a: [] for a in steps}
    for _ in range(3):
        for arm in steps:
            times[arm].append(time_us(steps[arm], 5))
    med = {a: statistics.median(t) for a, t in times.items()}
    margin = max(times["off"]) - min(times["off"])
    return [dict(block=f"NFPInsertNet(nfp_insert_idx={idx}) train step [64,3,224,224] f32", mode="eager",
                 us={a: [round(v, 1) for v in t] for a, t in times.items()},
                 median_us={a: round(v, 1) for a, v in med.items()}, margin_us=round(margin, 1),
                 beats_off=bool(med["off"] - med["valid"] > margin))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--l1", action="store_true", help="the L1 layer (Norm p = 1) and the NFPInsertNet step instead")
    args = ap.parse_args()
    recs = []

    def emit(new):      # (a line as soon as it is measured)
        for r in new:
            print(json.dumps(r), flush=True)
        recs.extend(new)
    if args.l1:
        for shape, dtype, nhwc in L1_SHAPES:
            emit(bench_shape(shape, dtype, nhwc, args.trace, measure="norm", ARMS=L1_ARMS))
        for idx in (0, 1):
            emit(bench_insert_net(idx, args.trace))
    else:
        for shape, dtype, nhwc in SHAPES:
            emit(bench_shape(shape, dtype, nhwc, args.trace))
        emit(bench_block(args.trace))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in recs) + "\n")


if __name__ == "__main__":
    main()
