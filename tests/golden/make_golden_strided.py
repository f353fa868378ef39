#!/usr/bin/env python3
"""Generate the fixtures of cases_strided.py by running the REAL reference (as make_golden.py does: its run_case, on the
CPU, where the reference lies; nothing of it is copied — a fixture holds the reference's out and grad_x).

    MPLBACKEND=Agg python tests/golden/make_golden_strided.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

from make_golden import run_case   # (imports the reference)
from cases_strided import STRIDED_CASES


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    for c in STRIDED_CASES:
        rec = run_case(c)
        path = os.path.join(HERE, c["name"] + ".npz")
        np.savez_compressed(path, **rec)
        print(f"{c['name']:36s} out{tuple(rec['out'].shape)} gx{tuple(rec['gx'].shape)} {os.path.getsize(path) / 1024:.0f} KiB")
    print(f"torch {torch.__version__}")


if __name__ == "__main__":
    main()
