#!/usr/bin/env python3
"""DeepTENEncoding: the HIP kernels (csrc/nfp_deepten.hip) against the torch composition (`_host.deepten_host`,
NFP_DEEPTEN_TORCH=1, read at call time) on the same GPU and build.  Per shape, dtype and layout two workloads — the
train-mode step (forward and torch.autograd.grad with respect to x, the codewords and the scale) and the no-grad forward —
each captured once per arm as a CUDA graph.  The arms alternate, --runs times each; a run is the time of --iters replays
between two device events, divided by --iters (milliseconds).  `spread` is max - min over an arm's runs.  Peak memory: what
one eager step allocates above what was allocated before it (MiB).  One JSON line per (shape, dtype, layout).

    python scripts/bench_deepten.py [--iters 20 --warmup 3 --runs 5] [--shapes 0,1,2,3] [--codes 32]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

SHAPES = [  # (B, D, H, W), the layouts measured
    ((64, 512, 7, 7), ("nchw", "nhwc")),         # ResNet18_DeepTENPooling
    ((64, 960, 7, 7), ("nchw", "nhwc")),         # MobileNetV3_DeepTENPooling
    ((64, 192, 14, 14), ("tok",)),               # ViTTiny_DeepTENPooling: the patch tokens behind the class token, in place
    ((32, 2048, 7, 7), ("nchw", "nhwc")),        # a ResNet50 map
]


def laid_out(x, layout):
    B, D, H, W = x.shape
    if layout == "nchw":
        return x.contiguous()
    if layout == "nhwc":
        return x.contiguous(memory_format=torch.channels_last)
    buf = torch.zeros(B, 1 + H * W, D, dtype=x.dtype, device=x.device)
    buf[:, 1:] = x.flatten(2).transpose(1, 2)
    return buf[:, 1:].transpose(1, 2).unflatten(2, (H, W))


def captured(fn, warmup):
    """fn as a CUDA graph (warmed up on a side stream first)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def replay_ms(graph, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    graph.replay()
    a.record()
    for _ in range(iters):
        graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--shapes", default="0,1,2,3")
    ap.add_argument("--codes", type=int, default=32)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_deepten.py measures on the GPU; there is no CPU timing"
    from neighbour_feature_pooling_amd import DeepTENEncoding, _abi
    dev = torch.device("cuda:0")
    L = _abi.load()
    for i in (int(s) for s in a.shapes.split(",")):
        shape, layouts = SHAPES[i]
        for dtype in (torch.float32, torch.bfloat16):
            for layout in layouts:
                torch.manual_seed(0)
                m = DeepTENEncoding(shape[1], a.codes).to(dev)
                x = laid_out(torch.relu(torch.randn(shape, device=dev)).to(dtype), layout).requires_grad_(True)
                go = torch.randn(shape[0], a.codes * shape[1], device=dev).to(dtype)
                leaves = (x, m.codewords, m.scale)

                def train():
                    return torch.autograd.grad(m(x), leaves, go)

                def infer():
                    with torch.no_grad():
                        return m(x)

                rec = dict(shape=list(shape), codes=a.codes, dtype=str(dtype).split(".")[-1], layout=layout)
                graphs = {}
                for arm in ("hip", "torch"):
                    if arm == "torch":
                        os.environ["NFP_DEEPTEN_TORCH"] = "1"
                    else:
                        os.environ.pop("NFP_DEEPTEN_TORCH", None)
                    n0 = L.nfp_launch_count()
                    train()
                    rec[f"launches_{arm}"] = int(L.nfp_launch_count() - n0)
                    rec[f"train_peak_mib_{arm}"] = peak_mib(train)
                    rec[f"infer_peak_mib_{arm}"] = peak_mib(infer)
                    graphs[arm] = (captured(train, a.warmup), captured(infer, a.warmup))
                os.environ.pop("NFP_DEEPTEN_TORCH", None)
                times = {(arm, w): [] for arm in graphs for w in (0, 1)}
                for _ in range(a.runs):
                    for arm in ("hip", "torch"):
                        for w in (0, 1):
                            times[(arm, w)].append(round(replay_ms(graphs[arm][w], a.iters), 4))
                for (arm, w), ts in times.items():
                    name = ("train", "infer")[w]
                    rec[f"{name}_ms_{arm}"] = ts
                    rec[f"{name}_median_ms_{arm}"] = sorted(ts)[len(ts) // 2]
                    rec[f"{name}_spread_ms_{arm}"] = round(max(ts) - min(ts), 4)
                for name in ("train", "infer"):
                    rec[f"{name}_speedup"] = round(rec[f"{name}_median_ms_torch"] / rec[f"{name}_median_ms_hip"], 2)
                    rec[f"{name}_faster"] = bool(min(rec[f"{name}_ms_torch"]) > max(rec[f"{name}_ms_hip"]))
                print(json.dumps(rec), flush=True)
                del graphs, x, go, m
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
