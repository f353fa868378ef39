#!/usr/bin/env python3
"""Generate the SimilarityAwarePooling fixtures tests/golden/sap_*.npz by running the REAL reference (cases_sap.py).

Runs only where the reference is available (never on the GPU box); nothing of it is copied — a fixture holds the
att_proj parameters (and, with bias=True, the layer's biases) the reference drew under torch.manual_seed(seed), the names
of its state dict, and its OUTPUTS: pooled, grad_x and the gradients of att_proj, all in full.

The reference imports models.pooling.enhanced_nfp.EnhancedNFPPooling, which it does not ship: a stand-in module is
registered before models.nfp_heads is imported, whose EnhancedNFPPooling is the reference's own NFPPooling behind the
(in_channels, R, measure, padding, **kw) signature of the call sites.

    MPLBACKEND=Agg python tests/golden/make_golden_sap.py
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

import cases as K
import cases_sap as KS
from models.pooling.nfp import NFPPooling  # the real reference (models/pooling/nfp.py)


class EnhancedNFPPooling(NFPPooling):
    def __init__(self, in_channels, R=1, measure="cosine", padding=0, **kw):
        super().__init__(in_channels, R=R, measure=measure, padding=padding, **kw)


_standin = types.ModuleType("models.pooling.enhanced_nfp")
_standin.EnhancedNFPPooling = EnhancedNFPPooling
sys.modules["models.pooling.enhanced_nfp"] = _standin

from models.nfp_heads import SimilarityAwarePooling  # noqa: E402  (the real reference, models/nfp_heads.py:204-232)


def _params(m):
    rec = {"w": m.att_proj.weight.detach().numpy().astype(np.float32),
           "b": m.att_proj.bias.detach().numpy().astype(np.float32),
           "sd_keys": np.array(sorted(m.state_dict()))}
    if m.nfp.bias:
        rec["nfp_bc"] = m.nfp.center_value.bias.detach().numpy().astype(np.float32)
        rec["nfp_nb"] = m.nfp.comp_neighbors.bias.detach().numpy().astype(np.float32)
    return rec


def run_case(c):
    torch.manual_seed(c["seed"])
    m = SimilarityAwarePooling(in_channels=c["shape"][1], **c["ctor"])
    x = torch.from_numpy(K.make_input(c)).requires_grad_(True)
    pooled = m(x)
    pooled.backward(torch.from_numpy(KS.make_grad_pooled(c, pooled.shape[1])))
    rec = _params(m)
    rec.update(pooled=pooled.detach().numpy().astype(np.float32), grad_x=x.grad.numpy().astype(np.float32),
               grad_w=m.att_proj.weight.grad.numpy().astype(np.float32),
               grad_b=m.att_proj.bias.grad.numpy().astype(np.float32))
    return rec


def init_case(C, ctor, seed):
    torch.manual_seed(seed)
    return _params(SimilarityAwarePooling(in_channels=C, **ctor))


def main():
    total = 0
    for c in KS.SAP_CASES:
        path = os.path.join(HERE, c["name"] + ".npz")
        np.savez_compressed(path, **run_case(c))
        total += os.path.getsize(path)
        print(path, os.path.getsize(path))
    for name, C, ctor, seed in KS.SAP_INIT_CASES:
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **init_case(C, ctor, seed))
        total += os.path.getsize(path)
    print("total bytes", total)


if __name__ == "__main__":
    main()
