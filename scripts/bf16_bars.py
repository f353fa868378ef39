#!/usr/bin/env python3
"""The per-element bf16 bars (tests/bf16_bars.py) on the GPU: every case of tests/bf16_cases.py once — each kernel family that
stores bf16 maps, its variant strings and both bars asserted — and the largest excess per family (DESIGN §2 records them).

    python scripts/bf16_bars.py [substring of the case ids]      (exit 1 when a bar or a variant fails)

A failed bar is recorded and the run goes on; any other error (a HIP error) ends it at once."""
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import pytest
import torch

import bf16_cases as G


def main():
    assert torch.cuda.is_available(), "bf16_bars.py runs the kernels; it needs the GPU"
    from neighbour_feature_pooling_amd import _abi, functional
    L = _abi.load()
    only = sys.argv[1] if len(sys.argv) > 1 else ""
    worst, bad = {}, 0
    for case in G.CASES:
        if only not in case[0]:
            continue
        mp = pytest.MonkeyPatch()
        functional._PLANS.clear()
        L.nfp_reload_env()
        try:
            e = G.run_case(case, mp)
            w = worst.setdefault(case[1], [0.0, 0.0])
            w[0], w[1] = max(w[0], e[0]), max(w[1], e[1])
        except AssertionError as err:
            bad += 1
            print("FAIL", case[0], str(err)[:300], flush=True)
        except BaseException:
            traceback.print_exc()
            print("STOP at", case[0], flush=True)
            return 3
        finally:
            mp.undo()
            functional._PLANS.clear()
            L.nfp_reload_env()
    for fam, (o, g) in worst.items():
        print("%-10s largest excess: out %.3f grad_x %.3f" % (fam, o, g))
    print("failed cases:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
