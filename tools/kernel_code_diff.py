#!/usr/bin/env python3
"""Is the device code of two source trees the same, kernel by kernel, whatever unit a kernel is compiled in?
usage: python tools/kernel_code_diff.py PARENT_CSRC THIS_CSRC [extra hipcc flags]

Every *.hip of both directories is compiled to a bare gfx950 code object (build.HIPCC_FLAGS + the extra flags +
--cuda-device-only --no-gpu-bundle-output -c), the kernel symbols are read with llvm-readelf -s (a kernel is a FUNC
with a <name>.kd descriptor beside it), each kernel's bytes are cut out of .text by symbol value and size, and hashed.
Reported: kernels on one side only, kernels that more than one unit of a tree defines, kernels whose bytes differ, and
which units of the same name are identical as whole objects.  Exit status 1 if any of the three lists is non-empty.
Bytes are hashed and nothing else: no disassembly."""
import concurrent.futures as cf
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neighbour_feature_pooling_amd import build


def readelf():
    beside = os.path.join(os.path.dirname(os.path.realpath(build.hipcc_path())), "..", "lib", "llvm", "bin", "llvm-readelf")
    return shutil.which("llvm-readelf") or beside


def compile_unit(src, obj, flags):
    unit = os.path.splitext(os.path.basename(src))[0]
    subprocess.check_call([build.hipcc_path()] + build.HIPCC_FLAGS + flags +
                          ["--cuda-device-only", "--no-gpu-bundle-output", "-cuid=" + unit, "-c", "-o", obj, src])
    return obj


def kernels_of(obj):
    """{kernel name: sha256 of its bytes} of one code object"""
    text = None
    for line in subprocess.check_output([readelf(), "-S", "-W", obj], text=True).splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) > 5 and f[1] == ".text":
            text = (int(f[0]), int(f[3], 16), int(f[4], 16))   # section index, address, file offset
    funcs, descriptors = {}, set()
    for line in subprocess.check_output([readelf(), "-s", "-W", obj], text=True).splitlines():
        f = line.split()
        if len(f) < 8 or not f[0].endswith(":") or not f[0][:-1].isdigit():
            continue
        if f[3] == "OBJECT" and f[7].endswith(".kd"):
            descriptors.add(f[7][:-3])
        elif f[3] == "FUNC" and text and f[6] == str(text[0]):
            funcs[f[7]] = (int(f[1], 16), int(f[2], 0))   # (sizes of six digits and more are printed in hex, with 0x)
    with open(obj, "rb") as fh:
        blob = fh.read()
    out = {}
    for name in descriptors:
        value, size = funcs[name]
        off = value - text[1] + text[2]
        out[name] = hashlib.sha256(blob[off:off + size]).hexdigest()
    return out


def tree(csrc, flags, tmp, tag):
    """({unit: {kernel: hash}}, {unit: hash of the whole object}) of one csrc directory"""
    units = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    with cf.ThreadPoolExecutor(max_workers=build.MAX_JOBS) as ex:
        objs = list(ex.map(lambda u: compile_unit(os.path.join(csrc, u), os.path.join(tmp, tag + "_" + u + ".co"), flags), units))
    whole = {}
    for u, o in zip(units, objs):
        with open(o, "rb") as fh:
            whole[u] = hashlib.sha256(fh.read()).hexdigest()
    return {u: kernels_of(o) for u, o in zip(units, objs)}, whole


def merged(per_unit, side):
    """{kernel: hash} of a tree, and the kernels that more than one of its units defines"""
    first, twice = {}, []
    for unit, ks in per_unit.items():
        for k, h in ks.items():
            if k in first:
                twice.append("%s: %s (%s and %s)" % (side, k, first[k][1], unit))
            else:
                first[k] = (h, unit)
    return first, twice


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    flags = sys.argv[3:]
    with tempfile.TemporaryDirectory(prefix="nfp_code_diff_") as tmp:
        pa, pa_whole = tree(sys.argv[1], flags, tmp, "parent")
        th, th_whole = tree(sys.argv[2], flags, tmp, "this")
    a, twice_a = merged(pa, "parent")
    b, twice_b = merged(th, "this")
    for side, per_unit in (("parent", pa), ("this", th)):
        print("%s: %d kernels in %d units  (%s)" % (side, sum(len(k) for k in per_unit.values()), len(per_unit),
                                                   ", ".join("%s %d" % (u, len(k)) for u, k in sorted(per_unit.items()))))
    only = ["parent only: %s (%s)" % (k, a[k][1]) for k in sorted(set(a) - set(b))] + \
           ["this only: %s (%s)" % (k, b[k][1]) for k in sorted(set(b) - set(a))]
    differ = ["%s (%s -> %s)" % (k, a[k][1], b[k][1]) for k in sorted(set(a) & set(b)) if a[k][0] != b[k][0]]
    same_units = sorted(set(pa_whole) & set(th_whole))
    print("units of the same name identical as whole objects: %s" %
          ", ".join("%s %s" % (u, pa_whole[u] == th_whole[u]) for u in same_units))
    for title, rows in (("kernels on one side only", only), ("kernels defined by more than one unit", twice_a + twice_b),
                        ("kernels whose bytes differ", differ)):
        print("%s: %d" % (title, len(rows)))
        for r in rows:
            print("  " + r)
    return 1 if only or twice_a or twice_b or differ else 0


if __name__ == "__main__":
    sys.exit(main())
