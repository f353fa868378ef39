#!/usr/bin/env python3
"""Registers / scratch / LDS / occupancy of every kernel of one translation unit, from hipcc's resource-usage remarks.
A row per kernel, keyed by its full demangled name without the argument list.
usage: python tools/kernel_resources.py csrc/nfp_tile_fwd.hip [name-filter]"""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neighbour_feature_pooling_amd import build


def kernel_name(demangled):
    """`void ns::(anonymous namespace)::k<8, true>(ns::CpK, int)` -> `k<8, true>`: the argument list is the last
    top-level (...) group; the return type of a template's instantiation and the anonymous namespace's prefix go too."""
    s = demangled.strip()
    if s.endswith(")"):
        depth = 0
        for i in range(len(s) - 1, -1, -1):
            depth += s[i] == ")"
            depth -= s[i] == "("
            if depth == 0:
                s = s[:i]
                break
    s = s[5:] if s.startswith("void ") else s
    return re.sub(r"\b(\w+::)*\(anonymous namespace\)::", "", s)      # (`nfp::(anonymous namespace)::`: every kernel has it)


def main():
    src = sys.argv[1]
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    out = subprocess.run([build.hipcc_path()] + build.HIPCC_FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", src],
                         capture_output=True, text=True).stderr
    cur = None
    rows = {}
    for line in out.splitlines():
        m = re.search(r"remark: (?:\s*)Function Name: (\S+)", line)
        if m:
            cur = kernel_name(subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout)
            rows[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            rows[cur][m.group(1).split(" ")[0]] = int(m.group(2))
        if "error" in line:
            print(line)
    for k, v in sorted(rows.items()):
        if flt in k:
            print(f"{k:48s} VGPR {v.get('VGPRs', -1):4d}  scratch {v.get('ScratchSize', -1):4d}  LDS {v.get('LDS', -1):6d}  "
                  f"waves/SIMD {v.get('Occupancy', -1)}  SGPR {v.get('TotalSGPRs', -1)}")
    print(f"{sum(flt in k for k in rows)} kernels")


if __name__ == "__main__":
    main()
