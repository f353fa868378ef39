#!/usr/bin/env python3
"""Generate the NFPPooling(bias=True) fixtures tests/golden/bias_*.npz by running the REAL reference (cases_bias.py).

Runs only where the reference is available (never on the GPU box); nothing of it is copied — a fixture holds the
biases the reference drew under torch.manual_seed(seed) and its OUTPUTS: out, grad_x and both bias gradients (or a
strided sample plus per-image sums for large maps).  gbc_none = 1 marks a centre-bias gradient that is None (Norm and
RMSE never call center_value).

    MPLBACKEND=Agg python tests/golden/make_golden_bias.py
"""
import os
import sys

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = os.environ.get("NFP_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import numpy as np
import torch

import cases as K
import cases_bias as KB
from models.pooling.nfp import NFPPooling  # the real reference (models/pooling/nfp.py)


def _store(rec, key, a, limit, axes):
    """The layout tests/conftest.py::assert_matches_golden reads: in full, or every 97th element plus sums over `axes`."""
    a = a.astype(np.float32)
    if a.size <= limit:
        rec[key] = a
    else:
        a64 = a.astype(np.float64)
        rec[key + "_shape"] = np.array(a.shape)
        rec[key + "_sample"] = a.reshape(-1)[K.gx_sample_index(a.size)]
        rec[key + "_sum"] = a64.sum(axis=axes)
        rec[key + "_abs_sum"] = np.abs(a64).sum(axis=axes)


def run_case(c):
    torch.manual_seed(c["seed"])
    m = NFPPooling(in_channels=c["shape"][1], bias=True, **c["ctor"])
    x = torch.from_numpy(K.make_input(c)).requires_grad_(True)
    out = m(x)
    go = torch.from_numpy(K.make_grad_out(c, tuple(out.shape)))
    out.backward(go)
    rec = {"bc": m.center_value.bias.detach().numpy().astype(np.float32),
           "nb": m.comp_neighbors.bias.detach().numpy().astype(np.float32),
           "gnb": m.comp_neighbors.bias.grad.numpy().astype(np.float32)}
    gbc = m.center_value.bias.grad
    rec["gbc_none"] = np.array(1 if gbc is None else 0)
    if gbc is not None:
        rec["gbc"] = gbc.numpy().astype(np.float32)
    _store(rec, "out", out.detach().numpy(), c["full_limit"], (2, 3))
    _store(rec, "gx", x.grad.numpy(), c["full_limit"], (1, 2, 3))
    return rec


def init_case(C, ctor, seed):
    torch.manual_seed(seed)
    m = NFPPooling(in_channels=C, bias=True, **ctor)
    return {"bc": m.center_value.bias.detach().numpy(), "nb": m.comp_neighbors.bias.detach().numpy()}


def main():
    total = 0
    for c in KB.BIAS_CASES:
        path = os.path.join(HERE, c["name"] + ".npz")
        np.savez_compressed(path, **run_case(c))
        total += os.path.getsize(path)
        print(path, os.path.getsize(path))
    for name, C, ctor, seed in KB.INIT_CASES:
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **init_case(C, ctor, seed))
        total += os.path.getsize(path)
    print("total bytes", total)


if __name__ == "__main__":
    main()
