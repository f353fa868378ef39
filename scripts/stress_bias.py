#!/usr/bin/env python3
"""Randomised stress of the biased kernels (NFPPooling(bias=True), csrc/nfp_bias.hip) at the sizes they run at: batches up
to 300, channels up to 512, radii up to 4, any geometry and padding mode, NCHW / channels-last / batch-strided views, f32
and bf16, against the float64 torch formulation (_host.nfp_host) on the GPU — out, grad_x and both bias gradients, the
neighbour bias's also per neighbour.  The draws reach every neighbours-per-workgroup count of bias_fwd (NB = 1, between,
N, N % NB != 0), which the forward's variant reports as bias_fwd<M,layout>x<NB>.
usage: python scripts/stress_bias.py [n] [seed]"""
import os, re, sys, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from neighbour_feature_pooling_amd import NFPPooling, _abi
from neighbour_feature_pooling_amd._host import nfp_host

MEASURES = ["norm", "cosine", "dot", "rmse", "geman", "attention", "emd", "canberra", "hellinger", "chisquared1",
            "chisquared2", "gfc", "pearson", "jeffrey", "squaredchord", "smith", "Norm"]   # (all but SCS; 'Norm': the p-quirk)
# float32-vs-float32 conditioning of a few measures (eps-sized denominators, near-cancelling sums): tests/test_gpu_bias.py
LOOSE = ("geman", "pearson", "hellinger", "squaredchord", "jeffrey", "smith", "canberra", "chisquared1", "chisquared2")
CHANNELS = [3, 5, 13, 64, 65, 130, 192, 512]
MAX_X = 10_000_000          # elements of x per case
MAX_TAPS = 120_000_000      # elements of the float64 reference's [B,C,N,Ho,Wo] tap stack per case

GRID = 2.0 ** -16           # inputs and biases on this grid: see exact()

_FWD = re.compile(r"bias_fwd<(-?\d+),(nchw|nhwc)>x(\d+)")


def fwd_nb(variant):
    """(layout, NB) from a forward variant bias_fwd<M,layout>x<NB>[+...]."""
    m = _FWD.match(variant)
    assert m, variant
    return m.group(2), int(m.group(3))


def exact(t):
    """t rounded to multiples of GRID.  With inputs and biases on the grid, every x + bias and x_c - x_n + bias the kernels
    form in float32 is exact, so their signs, zeros and ties are those of the float64 reference: the measures with
    sign(.) / min(.) in their gradient (Norm p = 1, EMD, Canberra, Hellinger, Smith, ...) would otherwise flip a few
    gradient terms wherever |a| or |v| is within float32 rounding of 0 — at these sizes, in nearly every case."""
    return (t * (1.0 / GRID)).round() * GRID


def quantize_biases(m):
    with torch.no_grad():
        m.center_value.bias.copy_(exact(m.center_value.bias))
        m.comp_neighbors.bias.copy_(exact(m.comp_neighbors.bias))
    return m


def rel(a, ref):
    """max|a - ref| / max|ref| in float64 on the device, NaNs as zero (their pattern is compared on its own)."""
    a, ref = torch.nan_to_num(a.double()), torch.nan_to_num(ref.double())
    den = ref.abs().max().item() if ref.numel() else 0.0
    return (a - ref).abs().max().item() / (den if den > 0 else 1.0) if a.numel() else 0.0


def same_nans(a, ref):
    return torch.equal(torch.isnan(a), torch.isnan(ref))


def run(m, x, go):
    """out, grad_x, grad_centre_bias (None for Norm / RMSE), grad_neighbour_bias, forward variant, backward variant."""
    L = _abi.load()
    m.zero_grad(set_to_none=True)
    x = x.detach().requires_grad_(True)
    out = m(x)
    fv = L.nfp_last_variant().decode()
    out.backward(go)
    bv = L.nfp_last_variant().decode()
    gbc = m.center_value.bias.grad
    return out.detach(), x.grad, gbc, m.comp_neighbors.bias.grad, fv, bv


def ref64(m, x, go):
    """The float64 formulation on x's device, on the same (already rounded) input and biases."""
    x64 = x.detach().double().requires_grad_(True)
    bc = m.center_value.bias.detach().double().requires_grad_(True)
    nb = m.comp_neighbors.bias.detach().double().requires_grad_(True)
    ref = nfp_host(x64, m.config, bc, nb)
    ref.backward(go.double())
    return ref.detach(), x64.grad, bc.grad, nb.grad


def compare(got, want, bf16, loose, per_neighbour=True):
    """(ok, errors) of run() against ref64(): out, grad_x, grad of the centre bias, grad of the neighbour bias (whole and
    worst neighbour slice gnb.view(C, N)[:, n])."""
    out, gx, gbc, gnb = got[:4]
    r_out, r_gx, r_gbc, r_gnb = want
    to, tg = (1e-2, 2e-2) if bf16 else ((5e-4, 5e-4) if loose else (1e-4, 1e-4))
    ok = same_nans(out.float(), r_out) and (gbc is None) == (r_gbc is None)
    eo, eg, en = rel(out, r_out), rel(gx, r_gx), rel(gnb, r_gnb)
    ec = rel(gbc, r_gbc) if gbc is not None and r_gbc is not None else 0.0
    es = 0.0
    if per_neighbour:
        a, b = gnb.view(gx.shape[1], -1), r_gnb.view(gx.shape[1], -1)
        es = max(rel(a[:, n], b[:, n]) for n in range(a.shape[1]))
    ok = ok and eo <= to and eg <= tg and en <= tg and ec <= tg and es <= tg
    return ok, (eo, eg, ec, en, es)


def _geometry(rnd):
    while True:
        R = rnd.choice([1, 1, 2, 3, 4])
        stride, dil = rnd.choice([1, 2, 3]), rnd.choice([1, 2])
        pad = rnd.randint(0, R * dil + 2)
        mode = rnd.choice(["reflect", "zeros", "replicate", "circular"])
        H, W = rnd.randint(2, 40), rnd.randint(2, 40)
        k = 2 * R + 1
        if H + 2 * pad < dil * (k - 1) + 1 or W + 2 * pad < dil * (k - 1) + 1:
            continue   # (the validity filter of tests/test_gpu_bias.py::test_random_geometries)
        if (mode == "reflect" and (pad >= H or pad >= W)) or (mode == "circular" and (pad > H or pad > W)):
            continue
        Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
        Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
        return R, stride, dil, pad, mode, H, W, k * k - 1, Ho * Wo


def batch_strided(x):
    """x's values as a [B,C,H,W] view of a [B, 1+H*W, C] buffer (patch tokens behind a class token): channels-last images,
    batch stride C*(1+H*W)."""
    B, C, H, W = x.shape
    buf = torch.zeros(B, 1 + H * W, C, dtype=x.dtype, device=x.device)
    v = buf[:, 1:].view(B, H, W, C).permute(0, 3, 1, 2)
    v.copy_(x)
    return v


def draw(rnd):
    """One case's parameters (python-random draws only: the data come from a device generator seeded with `seed`)."""
    R, stride, dil, pad, mode, H, W, N, O = _geometry(rnd)
    meas = rnd.choice(MEASURES)
    C = rnd.choice(CHANNELS)
    B = rnd.randint(1, 300)
    B = max(1, min(B, MAX_X // (C * H * W), MAX_TAPS // (C * N * O)))
    layout = rnd.choice(["nchw", "nhwc", "bstrided"])
    bf = rnd.random() < 0.25
    ctor = dict(R=R, measure=meas, padding=pad, stride=stride, dilation=dil, padding_mode=mode,
                similarity=rnd.random() < 0.5)
    if meas.lower() == "norm":
        ctor["p"] = rnd.choice([1, 2, 3])
    return dict(shape=(B, C, H, W), ctor=ctor, layout=layout, bf16=bf, N=N, O=O, seed=rnd.randint(0, 1 << 30))


def one_case(rnd, dev):
    c = draw(rnd)
    (B, C, H, W), ctor, layout, bf, N, seed = c["shape"], c["ctor"], c["layout"], c["bf16"], c["N"], c["seed"]
    R, pad, stride, dil = ctor["R"], ctor["padding"], ctor["stride"], ctor["dilation"]
    torch.manual_seed(seed)
    m = quantize_biases(NFPPooling(C, bias=True, **ctor).to(dev))    # (the conv's default init: random, non-zero biases)
    g = torch.Generator(device=dev).manual_seed(seed)
    dt = torch.bfloat16 if bf else torch.float32
    x = exact(torch.rand(B, C, H, W, generator=g, device=dev) + 0.25).to(dt)
    go = torch.randn(B, N, (H + 2 * pad - dil * 2 * R - 1) // stride + 1, (W + 2 * pad - dil * 2 * R - 1) // stride + 1,
                     generator=g, device=dev).to(dt)
    xr = x.contiguous(memory_format=torch.channels_last) if layout == "nhwc" else (batch_strided(x) if layout == "bstrided" else x)
    got = run(m, xr, go)
    want = ref64(m, x, go)
    ok, errs = compare(got, want, bf, ctor["measure"].lower() in LOOSE)
    fv, bv = got[4], got[5]
    del got, want
    desc = (f"B{B} C{C} {H}x{W} R{R} N={N} s{stride} d{dil} p{pad} {ctor['padding_mode']} {ctor['measure']}"
            f"{' p=%d' % ctor['p'] if 'p' in ctor else ''} sim={int(ctor['similarity'])} {layout} {'bf16' if bf else 'f32'}")
    return ok, desc, errs, (fv, bv)


def coverage(fv, desc):
    """(layout, 'NB=1' / '1<NB<N' / 'NB=N', N % NB != 0) of a case: NB from the forward's own variant, N from desc."""
    lay, nb = fwd_nb(fv)
    N = int(re.search(r"N=(\d+)", desc).group(1))
    return lay, ("NB=1" if nb == 1 else ("NB=N" if nb == N else "1<NB<N")), N % nb != 0


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    rnd = random.Random(seed)
    dev = torch.device("cuda:0")
    bad = 0
    seen = {}
    for i in range(n):
        ok, desc, errs, vs = one_case(rnd, dev)
        lay, kind, partial = coverage(vs[0], desc)
        key = f"{lay} {kind}" + (" N%NB" if partial else "")
        seen[key] = seen.get(key, 0) + 1
        if not ok:
            bad += 1
            print("FAIL", desc, ["%.2e" % e for e in errs], vs, flush=True)
        torch.cuda.empty_cache()
    print(f"{n} cases, forwards {dict(sorted(seen.items()))}, {bad} failed")


if __name__ == "__main__":
    main()
