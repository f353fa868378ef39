#!/usr/bin/env python3
"""Generate the fixtures of cases_heads_wide.py — the heads at 48 and 80 NFP maps — by running the REAL reference, with
make_golden_heads.py's run_case (which see: where it runs, what a fixture holds).  Nothing of the reference is copied.

    MPLBACKEND=Agg python tests/golden/make_golden_heads_wide.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np

from make_golden_heads import run_case  # (registers the stand-in module and imports the reference)
import cases_heads_wide as KW


def main():
    for c in KW.HEAD_WIDE_CASES:
        path = os.path.join(HERE, c["name"] + ".npz")
        np.savez_compressed(path, **run_case(c))
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
