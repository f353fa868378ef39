#!/usr/bin/env python3
"""What does the dispatcher of ONE build of libnfp_hip.so decide?  Host only: no GPU, nothing launches.

  python scripts/plan_sweep.py --lib PATH [--set NAME=VALUE ...]     one line per descriptor
  python scripts/plan_sweep.py --lib PATH --summary                  line count and sha256 of the sweep under no switch
                                                                     and under each of SETTINGS, a fresh process each

Two builds decide alike when their outputs are equal byte for byte (a change to the host-side selection code is
checked that way: the parent's library and the new one, every setting).  A line holds the descriptor, nfp_plan in both
directions (return code, text, nfp_last_error() where refused), nfp_saved_floats / nfp_workspace_bytes /
nfp_output_shape, the pool / gap / valid / valid_abs queries (with the stand-in workspace the descriptor is entitled to) and the
biased path's two sizes.

Descriptors: the 3000 draws of tests/test_dispatch_plan.py's sweep (same generator and seed), the tables of
test_dispatch_plan.py, test_mixed_plan.py and test_nchw_row_staging_plan.py; every bf16 one again with map_f32 = 1; every
R = 2, pad = 2 one again with inner_R = 1.
"""
import argparse
import ctypes
import hashlib
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from neighbour_feature_pooling_amd import _abi

SETTINGS = ["", "NFP_MFMA=0", "NFP_GEMM3=0", "NFP_GEMM3=2", "NFP_TILE_FIRST=1", "NFP_FORCE_GENERIC=1", "NFP_STAGE_BLOCKS=1",
            "NFP_POOL_TICKET=1", "NFP_BWD_BANDS=3", "NFP_FWD_SCALAR=1 NFP_BWD_ATOMIC=1", "NFP_TILE_DMA=1",
            "NFP_TILE_MAX_GRID=64"]
FIELDS = ("B", "C", "H", "W", "R", "pad", "stride", "dilation", "pad_mode", "measure", "dtype", "p", "sxC", "inner_R", "map_f32")


def descriptors():
    import test_dispatch_plan as tdp
    import test_mixed_plan as tmp_
    import test_nchw_row_staging_plan as trs
    desc = tdp.desc
    rnd = random.Random(20260)   # test_every_accepted_descriptor_launches_within_device_limits, draw for draw
    measures = [m for m in _abi.MEASURES if m != "scs"]
    out = []
    for _ in range(3000):
        H, W = rnd.choice([1, 2, 3, 5, 7, 9, 14, 16, 28, 33, 56, 64, 100, 150]), rnd.choice([1, 2, 4, 7, 8, 14, 28, 37, 56, 112, 200])
        R, stride, dil = rnd.choice([1, 1, 1, 2, 2, 3, 5]), rnd.choice([1, 1, 1, 2, 3]), rnd.choice([1, 1, 1, 2, 3])
        out.append(desc((rnd.choice([1, 3, 16, 64, 256, 1024]), rnd.choice([1, 3, 4, 16, 63, 192, 512, 960, 2048]), H, W), R=R,
                        pad=rnd.choice([0, 1, R, R * dil, R * dil + 2]), stride=stride, dil=dil,
                        mode=rnd.choice(_abi.PAD_MODES), measure=rnd.choice(measures), p=rnd.choice([1.0, 2.0, 3.0]),
                        dtype=rnd.choice([_abi.F32, _abi.BF16]), channels_last=rnd.random() < 0.3))
    (table,) = [m.args[1] for m in tdp.test_which_kernel_serves_which_call.pytestmark if m.name == "parametrize"]
    out += [desc(**kw) for kw, _, _ in table]
    mixed_kw = [h[0] for h in tmp_.HOT] + tmp_.GENERAL + [u[0] for u in tmp_.UNCHANGED]
    out += [tmp_.mixed(**kw) for kw in mixed_kw] + [desc(dtype=_abi.BF16, **kw) for kw in mixed_kw]
    out += [desc(**c[0]) for c in trs.CLASS]
    extra = []
    for d in out:
        if d.dtype == _abi.BF16 and d.map_f32 == 0:
            e = _abi.NfpDesc.from_buffer_copy(d)
            e.map_f32 = 1
            extra.append(e)
        if d.R == 2 and d.pad == 2 and d.inner_R == 0:
            e = _abi.NfpDesc.from_buffer_copy(d)
            e.inner_R = 1
            extra.append(e)
    return out + extra


def line(L, d):
    buf = ctypes.create_string_buffer(1024)
    ref = ctypes.byref(d)
    cols = [",".join(f"{getattr(d, f):g}" for f in FIELDS)]
    d.ws = None
    for backward in (0, 1):
        rc = L.nfp_plan(ref, backward, buf, len(buf))
        cols.append(f"{'bwd' if backward else 'fwd'}[{rc}] {buf.value.decode() if rc == 0 else L.nfp_last_error().decode()}")
    n, ho, wo = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = L.nfp_output_shape(ref, ctypes.byref(n), ctypes.byref(ho), ctypes.byref(wo))
    wsb = L.nfp_workspace_bytes(ref)
    cols.append(f"saved={L.nfp_saved_floats(ref)} ws={wsb} shape={rc}:{n.value},{ho.value},{wo.value}")
    d.ws = 0x1000 if wsb > 0 else None
    cols.append(f"pool={L.nfp_pool_supported(ref)}/{L.nfp_pool_saved_floats(ref)} gap={L.nfp_gap_supported(ref)}/"
                f"{L.nfp_gap_saved_floats(ref)} valid={L.nfp_valid_supported(ref)}/{L.nfp_valid_saved_floats(ref)} "
                f"valid_abs={L.nfp_valid_abs_supported(ref)}")
    cols.append(f"bias={L.nfp_bias_saved_floats(ref)}/{L.nfp_bias_scratch_floats(ref)}")
    return " | ".join(cols)


def sweep(lib, settings):
    for s in settings:
        name, value = s.split("=", 1)
        os.environ[name] = value
    _abi.LIB_PATH = os.path.abspath(lib)
    L = _abi.load()
    L.nfp_reload_env()
    for d in descriptors():
        print(line(L, d))


def summary(lib):
    for s in SETTINGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--lib", lib] + [a for kv in s.split() for a in ("--set", kv)]
        out = subprocess.run(cmd, check=True, capture_output=True).stdout
        lines = out.decode().splitlines()
        accepted = sum(ln.count(" fwd[0] ") + ln.count(" bwd[0] ") for ln in lines)
        print(f"{s or '(no switch)':36s} lines {len(lines)}  accepted plans {accepted}  sha256 {hashlib.sha256(out).hexdigest()}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", required=True)
    ap.add_argument("--set", action="append", default=[], metavar="NAME=VALUE")
    ap.add_argument("--summary", action="store_true")
    a = ap.parse_args()
    summary(a.lib) if a.summary else sweep(a.lib, a.set)
