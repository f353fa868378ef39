#!/usr/bin/env python3
"""Randomised stress of the native torch.autocast call (nfp_desc.map_f32: bf16 x in, float32 maps out, a bf16 grad_x back)
against the float64 torch formulation on the bf16-rounded x with a float32 grad_out.  Three families of draws:

  table    maps of 4 .. 512 pixels on fwd_band / bwd_fast <...,mix,...>
  band     maps of 513 .. ~2400 pixels on fwd_tile / bwd_tile <...,mix,...>
  general  what the hot kernels do not serve (stride, dilation, pad != R, circular padding, C % 4 != 0, the other
           measures): fwd_pairs / fwd_direct, bwd_gather / bwd_gather_banded / bwd_direct reading a float32 `out` beside bf16 x

Every case draws the input kind (normal / relu with whole pixels zeroed in one image / smooth; positive inputs for the
measures that are not smooth at 0), the layout (NCHW, channels-last, ViT tokens behind a class token) and `similarity`.
Checks: the maps within 2e-5 of the tensor's magnitude (the stress scripts' float32 bar), NaN patterns equal; grad_x
within ONE bf16 rounding of the reference per element (tests/one_rounding.py, slack 2e-5); grad_x against the same build's
NFP_AMP_UPCAST=1 result (2^-7 max|ref| + 1e-5 max|ref|: two roundings of float32 values that agree to 1e-5); types, two
launches, `mix` in both variants (table, band).  A case the library does not plan natively fails.

usage: python scripts/stress_mixed.py [n per family] [seed] [family ...]"""
import ctypes, os, sys, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import dataclasses
import numpy as np, torch
from neighbour_feature_pooling_amd import NFPPooling, _abi
from neighbour_feature_pooling_amd import functional as F
from neighbour_feature_pooling_amd._host import nfp_host
from neighbour_feature_pooling_amd.synth import feature_map
from one_rounding import one_rounding_excess
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from stress_tile import rel_err

FAMILIES = ("table", "band", "general")
SLACK = 2e-5                    # the stress scripts' float32 bar (stress_tile.py, stress_big_batch.py)
HOT = ["cosine", "norm", "dot", "gfc", "rmse"]
# every measure the library takes with map_f32 (all but Attention and SharpenedCosine)
ALL = HOT + ["geman", "emd", "canberra", "hellinger", "squaredchord", "chisquared1", "chisquared2", "pearson", "jeffrey", "smith"]
POSITIVE = set(ALL) - set(HOT) - {"pearson"}      # |.|, sqrt, log or a quotient by |a| + |b|: inputs in [0.25, 1.25)
ELEMS = 1_500_000               # B C H W at most: the float64 reference stays well under a second


def _batch(rnd, choices, per_image):
    return max(1, min(rnd.choice(choices), ELEMS // per_image))


def draw(rnd, family):
    """One case as plain values (no GPU): dict(shape, ctor, kind, layout, seeds)."""
    mode = rnd.choice(["reflect", "zeros", "replicate"])
    stride = dil = 1
    if family == "table":
        R = rnd.choice([1, 1, 2])
        meas = rnd.choice(["cosine"] + HOT)
        H, W = rnd.randint(R + 1, 22), rnd.randint(R + 1, 22)
        if H * W < 4:
            H = W = 3
        # k = 5 with two values per pair (the cosine form and its riders): bwd_fast's pair values, 400 B of LDS per pixel,
        # hold 409 pixels; above, the row-band backward serves the map — those shapes belong to no family here
        while R == 2 and meas in ("cosine", "dot", "gfc") and H * W > 409:
            H, W = rnd.randint(R + 1, 22), rnd.randint(R + 1, 22)
        # a k = 5 reflect border on a 3-pixel side: the table kernels decline it (nfp_plan: the row-band or the any-geometry
        # kernels) — the 3-pixel side stays, under another padding mode
        if R == 2 and mode == "reflect" and min(H, W) == 3:
            mode = rnd.choice(["zeros", "replicate"])
        C = 4 * rnd.randint(1, 16)
        if rnd.random() < 0.1:
            C, H, W = 512, 7, 7
        B = _batch(rnd, [1, 2, 3, 7, 40, 130, 300], C * H * W)
        pad = R
    elif family == "band":
        R = rnd.choice([1, 1, 2])
        meas = rnd.choice(["cosine"] + HOT)
        W = rnd.randint(2 * R + 2, 60)
        H = rnd.randint(513 // W + 1, min(160, max(513 // W + 1, 2400 // W)))
        C = rnd.choice([4 * rnd.randint(1, 16)] * 4 + [64, 128])
        B = _batch(rnd, [1, 2, 3, 7], C * H * W)
        pad = R
    else:
        R = rnd.choice([1, 1, 2])
        meas = rnd.choice(ALL)
        H, W = rnd.randint(2 * R + 1, 12), rnd.randint(2 * R + 1, 12)
        C = 4 * rnd.randint(1, 8)
        pad = R
        why = rnd.choice(["stride", "dilation", "pad", "circular", "channels"] + (["measure"] if meas not in HOT else []))
        if why == "stride":
            stride = rnd.choice([2, 3])
        elif why == "dilation":
            dil, pad = 2, rnd.choice([R, 2 * R])
        elif why == "pad":
            pad = rnd.choice([p for p in (0, 1, 2, 3) if p != R])
        elif why == "circular":
            mode = "circular"
        elif why == "channels":
            C = rnd.choice([3, 5, 6, 18, 67])
        if rnd.random() < 0.25:       # ... and sometimes two of them
            stride = max(stride, rnd.choice([1, 2]))
            C += rnd.choice([0, 1])
        span = dil * 2 * R + 1
        H, W = max(H, span), max(W, span)
        if mode == "reflect":
            pad = min(pad, H - 1, W - 1)
        if meas == "hellinger" and mode != "reflect":
            # a pixel against its own padded copy has distance 0 and no subgradient (NaN): how far the NaN travels is the
            # reference's business, not the storage type's — zeros padding, as the other stress scripts do
            mode = "zeros"
        if meas == "hellinger" and R == 2:
            mode = "zeros"
        B = rnd.choice([1, 2, 3, 5])
    ctor = dict(R=R, measure=meas, padding=pad, stride=stride, dilation=dil, padding_mode=mode,
                similarity=rnd.random() < 0.7)
    if meas == "norm":
        ctor["p"] = 2 if family != "general" else rnd.choice([1, 2])
    kind = "positive" if meas in POSITIVE else rnd.choice(["normal", "relu", "smooth"])
    return dict(shape=(B, C, H, W), ctor=ctor, kind=kind, layout=rnd.choice(["nchw", "nhwc", "tokens"]),
                seeds=(rnd.randint(0, 1 << 20), rnd.randint(0, 1 << 20)))


def describe(case):
    B, C, H, W = case["shape"]
    c = case["ctor"]
    return (f"B{B} C{C} {H}x{W} R{c['R']} {c['measure']}{'/p%d' % c['p'] if 'p' in c else ''} pad{c['padding']} s{c['stride']} "
            f"d{c['dilation']} {c['padding_mode']} sim={c['similarity']} {case['kind']} {case['layout']}")


def planned(case):
    """(forward, backward) plan texts of the case's map_f32 descriptor, or the library's refusal — host only (nfp_plan)."""
    L = _abi.load()
    B, C, H, W = case["shape"]
    cfg = dataclasses.replace(NFPPooling(C, **case["ctor"]).config, map_f32=1)
    sB = {"nchw": C * H * W, "nhwc": C * H * W, "tokens": (1 + H * W) * C}[case["layout"]]
    layout = "nchw" if case["layout"] == "nchw" else "nhwc"
    d = F.build_desc(case["shape"], F._canon(case["shape"], layout, sB), torch.bfloat16, cfg)
    if int(L.nfp_workspace_bytes(ctypes.byref(d))) > 0:
        d.ws = 0x1000       # (never dereferenced: nfp_plan launches nothing)
    texts = []
    buf = ctypes.create_string_buffer(1024)
    for back in (0, 1):
        rc = L.nfp_plan(ctypes.byref(d), back, buf, len(buf))
        texts.append(buf.value.decode().split(" |")[0] if rc == 0 else "refused: " + L.nfp_last_error().decode())
    return tuple(texts)


def in_family(family, fwd, bwd):
    if family == "table":
        return fwd.startswith("fwd_band<") and bwd.startswith("bwd_fast<") and ",mix," in fwd and ",mix," in bwd
    if family == "band":
        return fwd.startswith("fwd_tile<") and bwd.startswith("bwd_tile<") and ",mix," in fwd and ",mix," in bwd
    return fwd in ("fwd_pairs", "fwd_direct") and bwd in ("bwd_gather", "bwd_gather_banded", "bwd_direct")


def host_input(case):
    """x of the case, float32 on the bf16 grid (numpy)."""
    shape = case["shape"]
    if case["kind"] == "positive":
        xh = 0.75 + 0.5 * feature_map(shape, case["seeds"][0], "uniform")
    else:
        xh = feature_map(shape, case["seeds"][0], case["kind"]).copy()
    if case["kind"] == "relu":          # ... and whole pixels at zero in one image: every third
        b = case["seeds"][0] % shape[0]
        flat = xh[b].reshape(shape[1], -1)
        flat[:, case["seeds"][1] % 3::3] = 0.0
    return torch.from_numpy(np.ascontiguousarray(xh, np.float32)).bfloat16().float().numpy()


def as_layout(xh, layout, dev):
    B, C, H, W = xh.shape
    xt = torch.from_numpy(xh).to(dev, torch.bfloat16)
    if layout == "nhwc":
        return xt.contiguous(memory_format=torch.channels_last)
    if layout == "tokens":      # [B, 1 + HW, C] tokens behind a class token, viewed as [B,C,H,W]
        buf = torch.zeros(B, 1 + H * W, C, device=dev, dtype=torch.bfloat16)
        buf[:, 1:] = xt.flatten(2).transpose(1, 2)
        return buf[:, 1:].transpose(1, 2).unflatten(2, (H, W))
    return xt


def run(layer, x, go):
    """(maps, grad_x, forward variant, backward variant, launches, native?) of one fwd + bwd under torch.autocast."""
    L = _abi.load()
    x = x.detach().requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16):
        native = F._autocast_native(x, layer.config) is not None
        n0 = L.nfp_launch_count()
        out = layer(x)
    fwd = L.nfp_last_variant().decode()
    gx, = torch.autograd.grad(out, x, go)
    bwd = L.nfp_last_variant().decode()
    return out.detach(), gx, fwd, bwd, L.nfp_launch_count() - n0, native


def one_case(rnd, dev, family):
    case = draw(rnd, family)
    shape = case["shape"]
    layer = NFPPooling(shape[1], **case["ctor"])
    xh = host_input(case)
    x64 = torch.from_numpy(xh).double().requires_grad_(True)
    ref = nfp_host(x64, layer.config)
    goh = feature_map(tuple(ref.shape), case["seeds"][1])
    gref, = torch.autograd.grad(ref, x64, torch.from_numpy(goh).double())
    ref, gref = ref.detach().numpy(), gref.numpy()
    go = torch.from_numpy(goh).to(dev)
    out, gx, fwd, bwd, launches, native = run(layer, as_layout(xh, case["layout"], dev), go)
    before = os.environ.get("NFP_AMP_UPCAST")
    os.environ["NFP_AMP_UPCAST"] = "1"          # (read at call time)
    try:
        out_u, gx_u, fwd_u, bwd_u, _, native_u = run(layer, as_layout(xh, case["layout"], dev), go)
    finally:
        if before is None:
            del os.environ["NFP_AMP_UPCAST"]
        else:
            os.environ["NFP_AMP_UPCAST"] = before
    gxh, gxu = gx.float().cpu().numpy(), gx_u.float().cpu().numpy()
    e_map = rel_err(out.float().cpu().numpy(), ref)
    e_gx = one_rounding_excess(gxh, gref, SLACK)
    nan = np.isnan(gref)
    top = float(np.max(np.abs(gref[~nan]))) if not nan.all() else 0.0
    bound = 2.0 ** -7 * top + 1e-5 * top
    if not np.array_equal(np.isnan(gxh), np.isnan(gxu)):
        e_up = float("inf")
    else:
        d_up = float(np.max(np.abs(gxh[~nan] - gxu[~nan]))) if not nan.all() else 0.0
        e_up = d_up / bound if bound > 0 else (0.0 if d_up == 0 else float("inf"))
    ok = (native and not native_u and "mix" not in fwd_u and "mix" not in bwd_u and in_family(family, fwd, bwd)
          and out.dtype == torch.float32 and gx.dtype == torch.bfloat16 and tuple(gx.shape) == tuple(shape)
          and out_u.dtype == torch.float32 and gx_u.dtype == torch.bfloat16 and launches == 2
          and e_map <= SLACK and e_gx <= 1.0 and e_up <= 1.0)
    return ok, describe(case), (e_map, e_gx, e_up), (fwd, bwd)


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 2027
    os.environ["NFP_AMP_NATIVE"] = "1"          # the native call is opt-in (functional._autocast_native)
    dev = torch.device("cuda:0")
    total_bad = 0
    for k, family in enumerate(sys.argv[3:] or FAMILIES):
        rnd = random.Random(seed + k)
        bad, seen, worst = 0, {}, [0.0, 0.0, 0.0]
        for i in range(n):
            ok, desc, errs, vs = one_case(rnd, dev, family)
            key = vs[0].split("<")[0] + "/" + vs[1].split("<")[0] + (",dense" if ",dense>" in vs[1] else "")
            seen[key] = seen.get(key, 0) + 1
            worst = [max(a, b) for a, b in zip(worst, errs)]
            if not ok:
                bad += 1
                print("FAIL", desc, ["%.2e" % e for e in errs], vs, flush=True)
            torch.cuda.empty_cache()
        total_bad += bad
        print(f"{family}: {n} cases (seed {seed + k}), kernels {seen}, worst maps {worst[0]:.2e} (bar {SLACK:.0e}), "
              f"grad_x {worst[1]:.3f} of the one-rounding bar, {worst[2]:.3f} of the bound against the upcast, {bad} failed", flush=True)
    sys.exit(1 if total_bad else 0)
