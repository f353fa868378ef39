#!/usr/bin/env python3
"""Generate the NFPBottleneck fixtures tests/golden/bneck_*.npz by running the REAL reference (cases_bottleneck.py).

Runs only where the reference is available (never on the GPU box); nothing of it is copied — a fixture holds the
parameters and BatchNorm buffers the reference drew under torch.manual_seed(seed) ("p:<state-dict key>"), the sorted names
of its state dict, and its OUTPUTS, all in full: out, grad_x, the gradient of every trainable parameter ("g:<name>") and
the BatchNorm buffers after the step ("after:<key>").

The reference imports models.pooling.enhanced_nfp.EnhancedNFPPooling, which it does not ship: a stand-in module is
registered before models.nfp_heads is imported, as make_golden_sap.py does.

    MPLBACKEND=Agg python tests/golden/make_golden_bottleneck.py
"""
import os
import sys
import types

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

import cases_bottleneck as KB
from models.pooling.nfp import NFPPooling  # the real reference (models/pooling/nfp.py)


class EnhancedNFPPooling(NFPPooling):
    def __init__(self, in_channels, R=1, measure="cosine", padding=0, **kw):
        super().__init__(in_channels, R=R, measure=measure, padding=padding, **kw)


_standin = types.ModuleType("models.pooling.enhanced_nfp")
_standin.EnhancedNFPPooling = EnhancedNFPPooling
sys.modules["models.pooling.enhanced_nfp"] = _standin

from models.nfp_heads import NFPBottleneck  # noqa: E402  (the real reference, models/nfp_heads.py:234-278)

FROZEN = ("nfp.comp_neighbors.weight", "nfp.center_value.weight")     # constants of (C, R, measure): not stored


def _state(m, prefix):
    return {prefix + k: v.detach().numpy().copy() for k, v in m.state_dict().items() if k not in FROZEN}


def _init(cin, cout, stride, seed):
    torch.manual_seed(seed)
    m = NFPBottleneck(cin, cout, stride)
    rec = _state(m, "p:")
    rec["sd_keys"] = np.array(sorted(m.state_dict()))
    return m, rec


def run_case(c):
    m, rec = _init(c["cin"], c["cout"], c["stride"], c["seed"])
    m.train(c["train"])
    x = torch.from_numpy(KB.make_input(c)).requires_grad_(True)
    out = m(x)
    out.backward(torch.from_numpy(KB.make_grad_out(c, out.shape)))
    rec.update(out=out.detach().numpy().astype(np.float32), grad_x=x.grad.numpy().astype(np.float32))
    for k, p in m.named_parameters():
        if p.requires_grad and p.grad is not None:
            rec["g:" + k] = p.grad.numpy().astype(np.float32)
    rec.update({k: v for k, v in _state(m, "after:").items() if "running_" in k or "num_batches" in k})
    return rec


def main():
    total = 0
    for c in KB.BNECK_CASES:
        path = os.path.join(HERE, c["name"] + ".npz")
        np.savez_compressed(path, **run_case(c))
        total += os.path.getsize(path)
        print(path, os.path.getsize(path))
    for name, cin, cout, stride, seed in KB.BNECK_INIT_CASES:
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **_init(cin, cout, stride, seed)[1])
        total += os.path.getsize(path)
        print(path, os.path.getsize(path))
    print("total bytes", total)


if __name__ == "__main__":
    main()
