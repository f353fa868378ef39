#!/usr/bin/env python3
"""The projection [relu](bn(conv1x1(maps))) that keeps the map — NFPInsert's nfp_proj, NFPBottleneck's bn2(conv2(.)) — on the
HIP kernels (csrc/nfp_cpool.hip: cproj_*; NFP_CPROJ_TORCH=0, the kernels wherever they can serve) against the torch
composition of the same call (NFP_CPROJ_TORCH=1, read at call time: conv2d, batch_norm, relu) on the same GPU and build:
forward + backward in train mode, and the eval forward; and a whole NFPInsertNet step at a 224x224 input the same way.
Both arms run in one process, alternating, --runs times each.  One JSON line per row, microseconds:
  eager   median of per-step device-event times over --iters steps after --warmup (host launch gaps included)
  graph   the step captured into a CUDA graph, replayed --replays times between two events, per replay (kernels alone)
  eval    the eval-mode forward alone, graph-timed the same way
  peak    torch.cuda.max_memory_allocated over one train step, above what was allocated before it (bytes)
`margin` is the larger of the two arms' run-to-run spreads (max - min) of the graph times; `faster` says whether the HIP
arm's slowest graph run beats the composition's fastest by more than it, `slower` the reverse; neither: within the spread.

    python scripts/bench_insert.py [--iters 20 --warmup 5 --replays 50 --runs 3] [--rows 0,1,...,11] [--batch 64]

--channels-last: the same rows in a channels-last network — every arm ends in a channels-last `out` and receives a
channels-last grad_out — in float32 and bf16 (--dtypes; bf16: bf16 maps and conv weight, a float32 BatchNorm), three arms:
  nhwc    the channels-last kernels (memory_format=torch.channels_last, NFP_CPROJ_TORCH=0)
  torch   the composition asked for channels-last (NFP_CPROJ_TORCH=1)
  nchw    the NCHW kernels and the two conversions a channels-last network adds around them: the result converted to
          channels-last, the channels-last grad_out made NCHW-dense (what the package did before it had the keyword)
The whole-net rows (float32) run NFPInsertNet and its input in channels-last the same three ways.  `faster` / `slower`
compare nhwc with torch by the rule above; `vs_nchw_*` compare nhwc with nchw the same way.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from bench_heads import eager_us, graph_us, peak_bytes

# (maps [B,N,H,W], D, relu): the seven insert points of NFPInsertNet at a 224x224 input with the class defaults (the map
# behind each block, smaller by 2), two bottleneck tails, one 24-map case (R = 2 behind the /8 block)
PROJ_ROWS = [((64, 8, 110, 110), 16, True), ((64, 8, 54, 54), 24, True), ((64, 8, 26, 26), 40, True),
             ((64, 8, 12, 12), 80, True), ((64, 8, 12, 12), 112, True), ((64, 8, 5, 5), 160, True),
             ((64, 8, 5, 5), 960, True),
             ((64, 8, 54, 54), 64, False), ((256, 8, 12, 12), 256, False),
             ((64, 24, 24, 24), 40, True)]
NET_ROWS = [1, 3]            # nfp_insert_idx of the whole-net rows (10, 11)


class _ToChannelsLast(torch.autograd.Function):
    """The two copies of the `nchw` arm: the NCHW result made channels-last, the channels-last grad_out made NCHW-dense."""

    @staticmethod
    def forward(ctx, t):
        return t.contiguous(memory_format=torch.channels_last)

    @staticmethod
    def backward(ctx, g):
        return g.contiguous()


class _Converted(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return _ToChannelsLast.apply(self.inner(x))


def channels_last_rows(a):
    from neighbour_feature_pooling_amd import _abi, nfp_compress_map
    from neighbour_feature_pooling_amd.models import NFPInsertNet
    dev = torch.device("cuda:0")
    L = _abi.load()
    CL = torch.channels_last
    ARMS = ("nhwc", "torch", "nchw")
    for i in (int(s) for s in a.rows.split(",")):
        for dtype in (a.dtypes.split(",") if i < len(PROJ_ROWS) else ["f32"]):
            torch.manual_seed(0)
            td = dict(f32=torch.float32, bf16=torch.bfloat16)[dtype]
            if i < len(PROJ_ROWS):
                shape, D, relu = PROJ_ROWS[i]
                x = torch.randn(shape, device=dev).to(td).requires_grad_(True)
                conv = torch.nn.Conv2d(shape[1], D, 1, bias=False).to(dev).to(td)
                bn = torch.nn.BatchNorm2d(D).to(dev)
                go = torch.randn(shape[0], D, *shape[2:], device=dev).to(td).contiguous(memory_format=CL)
                leaves = (x, conv.weight, bn.weight, bn.bias)
                row = dict(what="projection, channels-last", dtype=dtype, maps=list(shape), D=D, relu=relu,
                           one_activation_bytes=shape[0] * D * shape[2] * shape[3] * (4 if dtype == "f32" else 2))

                def fwd(arm, training):
                    if arm == "nchw":
                        return _ToChannelsLast.apply(nfp_compress_map(x, conv.weight, bn, relu=relu, training=training))
                    return nfp_compress_map(x, conv.weight, bn, relu=relu, training=training, memory_format=CL)

                def make(arm):
                    def step():
                        return torch.autograd.grad(fwd(arm, True), leaves, go)

                    def eval_step():
                        with torch.no_grad():
                            return fwd(arm, False)
                    return step, eval_step
            else:
                idx = NET_ROWS[i - len(PROJ_ROWS)]
                nets = {}
                for arm in ARMS:
                    torch.manual_seed(0)
                    net = NFPInsertNet(num_classes=10, nfp_insert_idx=idx,
                                       memory_format=torch.contiguous_format if arm == "nchw" else CL)
                    if arm == "nchw":
                        net.insert = _Converted(net.insert)
                    nets[arm] = net.to(dev).to(memory_format=CL)
                x = torch.randn(a.batch, 3, 224, 224, device=dev).contiguous(memory_format=CL)
                go = torch.randn(a.batch, 10, device=dev)
                row = dict(what="NFPInsertNet step, channels-last", dtype=dtype, nfp_insert_idx=idx, input=list(x.shape))

                def make(arm):
                    net, params = nets[arm], tuple(nets[arm].parameters())

                    def step():
                        net.train()
                        return torch.autograd.grad(net(x), params, go)

                    def eval_step():
                        net.eval()
                        with torch.no_grad():
                            return net(x)
                    return step, eval_step

            def run(arm):
                os.environ["NFP_CPROJ_TORCH"] = "1" if arm == "torch" else "0"
                step, eval_step = make(arm)
                n0 = L.nfp_launch_count()
                step()
                launches = int(L.nfp_launch_count() - n0)
                return (eager_us(step, a.iters, a.warmup), graph_us(step, a.replays), graph_us(eval_step, a.replays),
                        peak_bytes(step), launches, L.nfp_last_variant().decode())

            res = {arm: [] for arm in ARMS}
            try:
                for _ in range(a.runs):
                    for arm in ARMS:
                        res[arm].append(run(arm))
            except RuntimeError as e:       # an arm torch refuses (a dtype pairing, say) is a row of its own; a device error ends it all
                if "HIP" in str(e) or "hip" in str(e) or "illegal" in str(e):
                    raise
                row["error"] = str(e).splitlines()[0][:200]
                print(json.dumps(row), flush=True)
                continue
            finally:
                os.environ.pop("NFP_CPROJ_TORCH", None)
            for arm in ARMS:
                r = res[arm]
                row[arm + "_eager_us"] = [round(t[0], 2) for t in r]
                row[arm + "_graph_us"] = [round(t[1], 2) for t in r]
                row[arm + "_eval_graph_us"] = [round(t[2], 2) for t in r]
                row[arm + "_peak_bytes"] = r[-1][3]
                row[arm + "_nfp_launches"] = r[-1][4]
                row[arm + "_last_variant"] = r[-1][5]
            med = lambda v: sorted(v)[len(v) // 2]     # noqa: E731
            spread = lambda v: max(v) - min(v)         # noqa: E731
            for key, tag in (("_graph_us", ""), ("_eval_graph_us", "eval_")):
                for other, pre in (("torch", ""), ("nchw", "vs_nchw_")):
                    h, t = row["nhwc" + key], row[other + key]
                    margin = max(spread(h), spread(t))
                    row[tag + pre + "margin_us"] = round(margin, 2)
                    row[tag + pre + "faster"] = bool(min(t) - max(h) > margin)
                    row[tag + pre + "slower"] = bool(min(h) - max(t) > margin)
                    row[tag + pre + "graph_speedup"] = round(med(t) / med(h), 3)
            print(json.dumps(row), flush=True)
            del x, go
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rows", default=",".join(str(i) for i in range(len(PROJ_ROWS) + len(NET_ROWS))))
    ap.add_argument("--batch", type=int, default=64, help="images of the whole-net rows")
    ap.add_argument("--channels-last", action="store_true", help="the rows in a channels-last network: three arms")
    ap.add_argument("--dtypes", default="f32,bf16", help="of the projection rows with --channels-last")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_insert.py measures on the GPU; there is no CPU timing"
    if a.channels_last:
        return channels_last_rows(a)
    from neighbour_feature_pooling_amd import _abi, nfp_compress_map
    from neighbour_feature_pooling_amd.models import NFPInsertNet
    dev = torch.device("cuda:0")
    L = _abi.load()
    for i in (int(s) for s in a.rows.split(",")):
        torch.manual_seed(0)
        if i < len(PROJ_ROWS):
            shape, D, relu = PROJ_ROWS[i]
            x = torch.randn(shape, device=dev, requires_grad=True)
            conv = torch.nn.Conv2d(shape[1], D, 1, bias=False).to(dev)
            bn = torch.nn.BatchNorm2d(D).to(dev)
            go = torch.randn(shape[0], D, *shape[2:], device=dev)
            leaves = (x, conv.weight, bn.weight, bn.bias)
            row = dict(what="projection", maps=list(shape), D=D, relu=relu,
                       one_activation_bytes=shape[0] * D * shape[2] * shape[3] * 4)

            def step():
                return torch.autograd.grad(nfp_compress_map(x, conv.weight, bn, relu=relu, training=True), leaves, go)

            def eval_step():
                with torch.no_grad():
                    return nfp_compress_map(x, conv.weight, bn, relu=relu, training=False)
        else:
            idx = NET_ROWS[i - len(PROJ_ROWS)]
            net = NFPInsertNet(num_classes=10, nfp_insert_idx=idx).to(dev)
            x = torch.randn(a.batch, 3, 224, 224, device=dev)
            go = torch.randn(a.batch, 10, device=dev)
            leaves = tuple(net.parameters())
            row = dict(what="NFPInsertNet step", nfp_insert_idx=idx, input=list(x.shape))

            def step():
                net.train()
                return torch.autograd.grad(net(x), leaves, go)

            def eval_step():
                net.eval()
                with torch.no_grad():
                    return net(x)

        def arm(composition):
            os.environ["NFP_CPROJ_TORCH"] = "1" if composition else "0"
            n0 = L.nfp_launch_count()
            step()
            launches = int(L.nfp_launch_count() - n0)
            return (eager_us(step, a.iters, a.warmup), graph_us(step, a.replays), graph_us(eval_step, a.replays), peak_bytes(step),
                    launches)

        res = {False: [], True: []}
        for _ in range(a.runs):
            for composition in (False, True):
                res[composition].append(arm(composition))
        os.environ.pop("NFP_CPROJ_TORCH", None)
        for composition, name in ((False, "hip"), (True, "torch")):
            r = res[composition]
            row[name + "_eager_us"] = [round(t[0], 2) for t in r]
            row[name + "_graph_us"] = [round(t[1], 2) for t in r]
            row[name + "_eval_graph_us"] = [round(t[2], 2) for t in r]
            row[name + "_peak_bytes"] = r[-1][3]
            row[name + "_nfp_launches"] = r[-1][4]
        med = lambda v: sorted(v)[len(v) // 2]     # noqa: E731
        spread = lambda v: max(v) - min(v)         # noqa: E731
        for key, tag in (("_graph_us", ""), ("_eval_graph_us", "eval_")):
            h, t = row["hip" + key], row["torch" + key]
            margin = max(spread(h), spread(t))
            row[tag + "margin_us"] = round(margin, 2)
            row[tag + "faster"] = bool(min(t) - max(h) > margin)
            row[tag + "slower"] = bool(min(h) - max(t) > margin)
            row[tag + "graph_speedup"] = round(med(t) / med(h), 3)
        row["eager_speedup"] = round(med(row["torch_eager_us"]) / med(row["hip_eager_us"]), 3)
        print(json.dumps(row), flush=True)
        del x, go, leaves
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
