#!/usr/bin/env python3
"""The bits of the compress-BN family (csrc/nfp_cpool.hip): every launching entry — nfp_cpool_*, nfp_cpool_wide_*,
nfp_cproj_*_fmt and the four nfp_cpsync_* stages — on tiny inputs made on the CPU from fixed seeds, a SHA-256 per output
tensor.  Two builds that claim to compute the same thing (a refactor of the kernels and its parent) are run once each and
compared: every sum of the family runs in a fixed order, so every digest must agree.

    python scripts/cp_bits.py --out new.json [--against parent.json]      (exit 1 on any difference)

Hashed per case: out, saved, running_mean, running_var; grad_maps, grad_w, grad_gamma, grad_beta of a full backward, of one
asked for grad_maps alone and of one asked for the parameters alone; for the staged calls also every rank's record and row
of k, Q.  The register form's cases cover the values below pairwise (N: the four template widths, 32 the 256-thread part
kernels; P: 289 is two chunks at 32 maps, 1100 two at 8, 35 a ragged quad; D: 130 is two 128-tiles with a last one of 2,
67 two 64-tiles of an odd D, 48 in bf16 NHWC the paired stores); then the paired stores whose span starts on an odd
element and an out at an address of 2 mod 4, the wide form at 33, 48 and 96 maps, and two emulated ranks, one without an
image."""
import argparse
import contextlib
import hashlib
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

MOM, EPS = 0.1, 1e-5
HW = {1: (1, 1), 35: (5, 7), 49: (7, 7), 256: (16, 16), 289: (17, 17), 1100: (25, 44)}
NS, PS, DS, BS = (3, 12, 17, 32), (1, 35, 49, 289, 1100), (5, 48, 67, 130), (1, 3)
FLAGS = (False, True)


def pairwise(dims, valid):
    """Rows of the product of `dims` that cover every pair of values of two dimensions some valid row holds, chosen
    greedily in product order (deterministic)."""
    rows = [r for r in itertools.product(*dims) if valid(r)]
    pairs = lambda r: {(i, r[i], j, r[j]) for i in range(len(r)) for j in range(i + 1, len(r))}     # noqa: E731
    todo = set().union(*map(pairs, rows))
    picked = []
    while todo:
        best = max(rows, key=lambda r: len(pairs(r) & todo))
        picked.append(best)
        todo -= pairs(best)
    return picked


def cases():
    """(name, kind, B, N, P, D, bf16, train, relu, nhwc, out at 2 mod 4)"""
    ok = lambda r: not (r[5] and r[3] * r[1] < 2)     # noqa: E731   (train-mode statistics need two values)
    out = []
    for N, P, D, B, bf16, train in pairwise((NS, PS, DS, BS, FLAGS, FLAGS), ok):
        out.append(("pool", B, N, P, D, bf16, train, True, False, False))
    for N, P, D, B, bf16, train, relu, nhwc in pairwise((NS, PS, DS, BS, FLAGS, FLAGS, FLAGS, FLAGS), ok):
        out.append(("proj", B, N, P, D, bf16, train, relu, nhwc, False))
    for N, train in itertools.product(NS, FLAGS):
        out.append(("proj", 3, N, 49, 5, True, train, True, True, False))       # pairs across the pixel rows, odd spans
        out.append(("proj", 2, N, 35, 48, True, train, False, True, True))      # one tile, out at 2 mod 4
    for N, P, bf16, train in itertools.product((33, 48, 96), (49, 256), FLAGS, FLAGS):
        out.append(("wide", 2, N, P, 70, bf16, train, True, False, False))
    return [("%s_B%d_N%d_P%d_D%d_%s_%s_%s_%s%s" % (c[0], c[1], c[2], c[3], c[4], "bf16" if c[5] else "f32",
                                                    "train" if c[6] else "eval", "relu" if c[7] else "lin",
                                                    "nhwc" if c[8] else "nchw", "_odd" if c[9] else ""),) + c for c in out]


# (name, images per rank, kind, N, P, D, bf16, relu, nhwc[, out at 2 mod 4]): the staged calls by emulated ranks, as tests/test_gpu_cp_sync.py
SYNC_CASES = [("sync_pool_empty", (3, 0), "pool", 3, 49, 130, False, True, False),
              ("sync_pool_bf16", (2, 1), "pool", 17, 35, 48, True, True, False),
              ("sync_pool_chunked", (0, 2), "pool", 32, 289, 5, False, True, False),
              ("sync_proj_relu_nhwc_bf16", (3, 0), "proj", 12, 49, 48, True, True, True),
              ("sync_proj_lin", (2, 1), "proj", 32, 289, 67, False, False, False),
              ("sync_proj_relu_chunked", (0, 1), "proj", 3, 1100, 130, False, True, False),
              ("sync_proj_lin_nhwc", (1, 2), "proj", 17, 35, 67, True, False, True),
              ("sync_proj_relu_nhwc_bf16_odd", (2, 1), "proj", 12, 35, 48, True, True, True, True)]


def inputs(seed, kind, B, N, P, D):
    """float32 CPU tensors: maps [B,N,H,W], w [D,N], gamma, beta, running_mean, running_var [D], grad_out"""
    g = torch.Generator().manual_seed(7919 * seed + 1)
    hw = HW[P]
    maps = torch.randn(B, N, *hw, generator=g) + 0.25
    w = torch.randn(D, N, generator=g) * 0.5
    gamma = torch.rand(D, generator=g) + 0.5
    beta = torch.randn(D, generator=g) * 0.5
    rm = torch.randn(D, generator=g) * 0.3
    rv = torch.rand(D, generator=g) + 0.5
    go = torch.randn(*((B, D, *hw) if kind == "proj" else (B, D)), generator=g)
    return maps, w, gamma, beta, rm, rv, go


def digest(t):
    if t is None:
        return None
    t = t.detach().cpu().contiguous()
    raw = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
    return hashlib.sha256(raw.numpy().tobytes()).hexdigest()


def on_device(ins, kind, bf16, nhwc, dev):
    maps, w, gamma, beta, rm, rv, go = ins
    dt = torch.bfloat16 if bf16 else torch.float32
    go = go.to(dev).to(dt if kind == "proj" else torch.float32)
    if nhwc:
        go = go.contiguous(memory_format=torch.channels_last)
    return maps.to(dev).to(dt).contiguous(), w.to(dev), gamma.to(dev), beta.to(dev), rm.to(dev), rv.to(dev), go


@contextlib.contextmanager
def shifted_out(C, on):
    """Inside, the binding's results start one element into their allocation (bf16: an address of 2 mod 4).  The binding
    has no argument for that, so its allocator `_cp_out` is replaced; a binding without that name fails here, loudly."""
    cp_out = C._cp_out
    if on:
        def shifted(kind, maps, D, channels_last=False):
            like = cp_out(kind, maps, D, channels_last)
            flat = torch.empty(like.numel() + 1, dtype=like.dtype, device=like.device)
            return flat[1:].as_strided(like.shape, like.stride())
        C._cp_out = shifted
    try:
        yield
    finally:
        C._cp_out = cp_out


def run_case(C, case, dev):
    _, kind, B, N, P, D, bf16, train, relu, nhwc, odd = case
    seed = int(hashlib.sha256(case[0].encode()).hexdigest()[:6], 16)
    maps, w, gamma, beta, rm, rv, go = on_device(inputs(seed, kind, B, N, P, D), kind, bf16, nhwc, dev)
    with shifted_out(C, odd):
        out, saved = C._cp_forward_call(kind, maps, w, gamma, beta, rm, rv, train, MOM, EPS, relu, nhwc)
    assert not odd or out.data_ptr() % 4 == 2
    res = dict(out=digest(out), saved=digest(saved), rm=digest(rm), rv=digest(rv))
    for tag, want in (("", (True, True, True, True)), ("maps_only.", (True, False, False, False)),
                      ("params_only.", (False, True, True, True))):
        grads = C._cp_backward_call(kind, maps, w, gamma, beta, rm, rv, saved, train, EPS, go, want, relu)
        for name, t in zip(("grad_maps", "grad_w", "grad_gamma", "grad_beta"), grads):
            if t is not None:
                res[tag + name] = digest(t)
    return res


def run_sync(C, case, dev):
    name, shards, kind, N, P, D, bf16, relu, nhwc = case[:9]
    odd = len(case) > 9 and case[9]
    seed = int(hashlib.sha256(name.encode()).hexdigest()[:6], 16)
    maps, w, gamma, beta, rm, rv, go = on_device(inputs(seed, kind, sum(shards), N, P, D), kind, bf16, False, dev)
    ms = [m.contiguous() for m in torch.split(maps, shards)]
    gos = [g.contiguous(memory_format=torch.channels_last) if nhwc else g.contiguous() for g in torch.split(go, shards)]
    records = torch.cat([C.cp_sync_moments_call(m)[None] for m in ms])
    res = dict(records=digest(records))
    saved, parts = [], []
    for r, m in enumerate(ms):
        rm_r, rv_r = rm.clone(), rv.clone()
        with shifted_out(C, odd):
            out, sv = C.cp_sync_forward_call(kind, m, w, gamma, beta, rm_r, rv_r, MOM, EPS, records, relu, nhwc)
        assert not odd or out.data_ptr() % 4 == 2
        saved.append(sv)
        res.update({"rank%d.out" % r: digest(out), "rank%d.saved" % r: digest(sv), "rank%d.rm" % r: digest(rm_r),
                    "rank%d.rv" % r: digest(rv_r)})
    for r, m in enumerate(ms):
        parts.append(C.cp_sync_reduce_call(kind, m, w, gamma, beta, saved[r], EPS, gos[r], (True, True, True), relu))
        for key, t in zip(("grad_w", "grad_gamma", "grad_beta", "kq_row"), parts[r]):
            res["rank%d.%s" % (r, key)] = digest(t)
    rows = torch.cat([p[3][None] for p in parts])
    for r, m in enumerate(ms):
        res["rank%d.grad_maps" % r] = digest(C.cp_sync_maps_call(kind, m, w, gamma, beta, saved[r], EPS, gos[r], rows, relu))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--against")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cp_bits.py runs the kernels; it needs the GPU"
    from neighbour_feature_pooling_amd import _abi, compress as C
    _abi.load()
    dev = torch.device("cuda:0")
    got = {c[0]: run_case(C, c, dev) for c in cases()}
    got.update({c[0]: run_sync(C, c, dev) for c in SYNC_CASES})
    torch.cuda.synchronize()
    with open(a.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
    n = sum(len(v) for v in got.values())
    print("%d cases, %d digests -> %s" % (len(got), n, a.out))
    if not a.against:
        return 0
    with open(a.against) as f:
        ref = json.load(f)
    bad = [(c, t) for c in sorted(set(got) | set(ref)) for t in sorted(set(got.get(c, {})) | set(ref.get(c, {})))
           if got.get(c, {}).get(t, "missing") != ref.get(c, {}).get(t, "missing")]
    for c, t in bad:
        print("DIFFERS %s %s" % (c, t))
    print("%d of %d digests differ from %s" % (len(bad), n, a.against))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
