#!/usr/bin/env python3
"""Generate the insert fixtures tests/golden/insert_*.npz by running the REAL reference (cases_insert.py): the layer
models/mobilenetv3.py::MOBILENETV3_NFP_INSERT builds at its lines 345-350 — the reference's NFPPooling(in_channels=C, **kw)
and, after it, nn.Sequential(Conv2d(nfp.out_channels, C, 1, bias=False), BatchNorm2d(C), ReLU(inplace=True)) — and its
forward nfp_proj(nfp(x)) (352-353).  The net around it needs timm and pretrained weights, which are not needed for the
block: the two constructors below are torch's own and the reference's own, called in the reference's order.

Runs only where the reference is available (never on the GPU box); nothing of it is copied — a fixture holds the
parameters and BatchNorm buffers drawn under torch.manual_seed(seed) ("p:<state-dict key>"), the sorted names of the state
dict, and the OUTPUTS, all in full: out, grad_x, the gradient of every trainable parameter ("g:<name>") and the BatchNorm
buffers after the step ("after:<key>").  An eval-mode case first takes one train-mode forward of its input (so that the
running statistics it then reads are not the initial 0 / 1); its "p:" entries are the state behind that.

    MPLBACKEND=Agg python tests/golden/make_golden_insert.py
"""
import os
import sys

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = os.environ.get("NFP_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))   # (a checkout beside this one)
sys.path.insert(0, REF)

import numpy as np
import torch
import torch.nn as nn

import cases_insert as KI
from models.pooling.nfp import NFPPooling  # the real reference (models/pooling/nfp.py)


class Block(nn.Module):
    """The two attributes the reference net holds, under its names, built in its order."""

    def __init__(self, C, kw):
        super().__init__()
        self.nfp = NFPPooling(in_channels=C, **kw)
        self.nfp_proj = nn.Sequential(nn.Conv2d(self.nfp.out_channels, C, kernel_size=1, bias=False), nn.BatchNorm2d(C),
                                      nn.ReLU(inplace=True))

    def forward(self, x):
        return self.nfp_proj(self.nfp(x))


def _frozen(key):
    return key.endswith("comp_neighbors.weight") or key.endswith("center_value.weight")   # constants of (C, R, measure)


def _state(m, prefix):
    return {prefix + k: v.detach().numpy().copy() for k, v in m.state_dict().items() if not _frozen(k)}


def _init(C, kw, seed):
    torch.manual_seed(seed)
    m = Block(C, kw)
    rec = _state(m, "p:")
    rec["sd_keys"] = np.array(sorted(m.state_dict()))
    return m, rec


def run_case(c):
    m, rec = _init(c["shape"][1], c["kw"], c["seed"])
    x = torch.from_numpy(KI.make_input(c)).requires_grad_(True)
    if not c["train"]:
        with torch.no_grad():
            m(x)
        rec.update(_state(m, "p:"))
    m.train(c["train"])
    out = m(x)
    out.backward(torch.from_numpy(KI.make_grad_out(c, out.shape)))
    rec.update(out=out.detach().numpy().astype(np.float32), grad_x=x.grad.numpy().astype(np.float32))
    for k, p in m.named_parameters():
        if p.requires_grad and p.grad is not None:
            rec["g:" + k] = p.grad.numpy().astype(np.float32)
    rec.update({k: v for k, v in _state(m, "after:").items() if "running_" in k or "num_batches" in k})
    return rec


def main():
    total = 0
    for c in KI.INSERT_CASES:
        path = os.path.join(HERE, c["name"] + ".npz")
        np.savez_compressed(path, **run_case(c))
        total += os.path.getsize(path)
        print(path, os.path.getsize(path))
    for name, C, kw, seed in KI.INSERT_INIT_CASES:
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **_init(C, kw, seed)[1])
        total += os.path.getsize(path)
        print(path, os.path.getsize(path))
    print("total bytes", total)


if __name__ == "__main__":
    main()
