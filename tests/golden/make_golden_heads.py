#!/usr/bin/env python3
"""Generate the head fixtures tests/golden/head_*.npz by running the REAL reference (cases_heads.py): NFPHead,
MultiRadiusNFPHead and AdaptiveFusionNFP of models/nfp_heads.py.

Runs only where the reference is available (never on the GPU box); nothing of it is copied — a fixture holds the
parameters and BatchNorm buffers the reference drew under torch.manual_seed(seed) ("p:<state-dict key>"), the sorted names
of its state dict, and its OUTPUTS, all in full: out, grad_x, the gradient of every trainable parameter ("g:<name>") and
the BatchNorm buffers after the step ("after:<key>").  An eval-mode case first takes one train-mode forward of its input
(so that the running statistics it then reads are not the initial 0 / 1); its "p:" entries are the state behind that.

The reference imports models.pooling.enhanced_nfp.EnhancedNFPPooling, which it does not ship: a stand-in module is
registered before models.nfp_heads is imported, as make_golden_sap.py does.

    MPLBACKEND=Agg python tests/golden/make_golden_heads.py
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

import cases_heads as KH
from models.pooling.nfp import NFPPooling  # the real reference (models/pooling/nfp.py)


class EnhancedNFPPooling(NFPPooling):
    def __init__(self, in_channels, R=1, measure="cosine", padding=0, **kw):
        super().__init__(in_channels, R=R, measure=measure, padding=padding, **kw)


_standin = types.ModuleType("models.pooling.enhanced_nfp")
_standin.EnhancedNFPPooling = EnhancedNFPPooling
sys.modules["models.pooling.enhanced_nfp"] = _standin

import models.nfp_heads as ref_heads  # noqa: E402  (the real reference, models/nfp_heads.py)


def _frozen(key):
    return key.endswith("comp_neighbors.weight") or key.endswith("center_value.weight")   # constants of (C, R, measure)


def _state(m, prefix):
    return {prefix + k: v.detach().numpy().copy() for k, v in m.state_dict().items() if not _frozen(k)}


def _init(cls, C, ctor, seed):
    torch.manual_seed(seed)
    m = getattr(ref_heads, cls)(**{KH.IN_KW[cls]: C}, **ctor)
    rec = _state(m, "p:")
    rec["sd_keys"] = np.array(sorted(m.state_dict()))
    return m, rec


def run_case(c):
    m, rec = _init(c["cls"], c["shape"][1], c["ctor"], c["seed"])
    x = torch.from_numpy(KH.make_input(c)).requires_grad_(True)
    if not c["train"]:
        with torch.no_grad():
            m(x)
        rec.update(_state(m, "p:"))
    m.train(c["train"])
    out = m(x)
    out.backward(torch.from_numpy(KH.make_grad_out(c, out.shape)))
    rec.update(out=out.detach().numpy().astype(np.float32), grad_x=x.grad.numpy().astype(np.float32))
    for k, p in m.named_parameters():
        if p.requires_grad and p.grad is not None:
            rec["g:" + k] = p.grad.numpy().astype(np.float32)
    rec.update({k: v for k, v in _state(m, "after:").items() if "running_" in k or "num_batches" in k})
    return rec


def main():
    total = 0
    for c in KH.HEAD_CASES:
        path = os.path.join(HERE, c["name"] + ".npz")
        np.savez_compressed(path, **run_case(c))
        total += os.path.getsize(path)
        print(path, os.path.getsize(path))
    for name, cls, C, ctor, seed in KH.HEAD_INIT_CASES:
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **_init(cls, C, ctor, seed)[1])
        total += os.path.getsize(path)
        print(path, os.path.getsize(path))
    print("total bytes", total)


if __name__ == "__main__":
    main()
