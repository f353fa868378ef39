#!/usr/bin/env python3
"""Generate the DeepTENEncoding fixtures tests/golden/deepten_*.npz by running the REAL reference (cases_deepten.py).

Runs only where the reference is available (never on the GPU box); nothing of it is copied — a fixture holds the parameters
the reference drew under torch.manual_seed(seed) (or cases_deepten.make_synth_params), the names of its state dict, and its
OUTPUTS in full: out, grad_x, grad_codewords, grad_scale from the float32 module, and the same four ("*_64") from the
module under .double() on the same float32 inputs and parameters.

    python tests/golden/make_golden_deepten.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = os.environ.get("NFP_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))   # (a checkout beside this one)
sys.path.insert(0, REF)

import numpy as np
import torch

import cases_deepten as KD

from models.deepten import DeepTENEncoding  # noqa: E402  (the real reference, models/deepten.py)


def _run(m, x, go, dtype):
    m = m.to(dtype)
    m.zero_grad(set_to_none=True)
    xi = x.detach().clone().to(dtype).requires_grad_(True)
    out = m(xi)
    out.backward(go.to(dtype))
    return [t.detach().numpy() for t in (out, xi.grad, m.codewords.grad, m.scale.grad)]


def run_case(c):
    torch.manual_seed(c["seed"])
    m = DeepTENEncoding(in_channels=c["shape"][1], num_codes=c["K"])
    if c["params"] == "synth":
        cw, sc = KD.make_synth_params(c)
        with torch.no_grad():
            m.codewords.copy_(torch.from_numpy(cw))
            m.scale.copy_(torch.from_numpy(sc))
    rec = {"codewords": m.codewords.detach().numpy().astype(np.float32).copy(),
           "scale": m.scale.detach().numpy().astype(np.float32).copy(), "sd_keys": np.array(sorted(m.state_dict()))}
    x, go = torch.from_numpy(KD.make_x(c)), torch.from_numpy(KD.make_grad_out(c))
    names = ("out", "grad_x", "grad_codewords", "grad_scale")
    rec.update({n: v.astype(np.float32) for n, v in zip(names, _run(m, x, go, torch.float32))})
    rec.update({n + "_64": v.astype(np.float64) for n, v in zip(names, _run(m, x, go, torch.float64))})
    return rec


def init_case(D, K, seed):
    torch.manual_seed(seed)
    m = DeepTENEncoding(in_channels=D, num_codes=K)
    return {"codewords": m.codewords.detach().numpy().astype(np.float32), "scale": m.scale.detach().numpy().astype(np.float32),
            "sd_keys": np.array(sorted(m.state_dict()))}


def main():
    total = 0
    for c in KD.DEEPTEN_CASES:
        path = os.path.join(HERE, c["name"] + ".npz")
        np.savez_compressed(path, **run_case(c))
        total += os.path.getsize(path)
        print(path, os.path.getsize(path))
    for name, D, K, seed in KD.DEEPTEN_INIT_CASES:
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **init_case(D, K, seed))
        total += os.path.getsize(path)
        print(path, os.path.getsize(path))
    print("total bytes", total)


if __name__ == "__main__":
    main()
