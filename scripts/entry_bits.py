#!/usr/bin/env python3
"""The bits behind the C entry points of csrc/nfp_hip.hip, one tiny case per route of the dispatcher: plain nfp, the fused
pooled tail (nfp_pool), GAP beside the maps (nfp_with_gap), the valid maps and their L1 family, the biased calls, and one
empty batch per family.  Inputs are made on the CPU from fixed seeds.  Two builds that claim to decide and compute the
same thing (a refactor of the dispatcher and its parent) are run once each and compared; every field must agree.

    python scripts/entry_bits.py --out new.json [--against parent.json] [--root OTHER_CHECKOUT]
                                        (exit 1 on any difference, 2 on a route that is not the one the case is there for)

Recorded per case: a SHA-256 of every output and of every gradient, nfp_last_variant() behind the forward and behind the
backward, and by how much nfp_launch_count() moved (or the exception a case ends in).  Each case names a piece of the
variant string it expects either way: the route is read from there, not from the shape.  Cases marked NFP_POOL_TICKET=1 run under that switch (and a plan
cache of their own: the scratch size belongs to the arm)."""
import argparse
import hashlib
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--against")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the tree whose package is imported (default: this script's own): the same script runs another checkout")
ARGS = ap.parse_args() if __name__ == "__main__" else None
sys.path.insert(0, os.path.abspath(ARGS.root) if ARGS else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def cfg(measure, R=1, padding=None, **kw):
    from neighbour_feature_pooling_amd import NfpConfig
    return NfpConfig(R=R, measure=measure, padding=R if padding is None else padding,
                     diff_weights=measure in ("norm", "rmse"), **kw)


def _nfp(x, c):
    from neighbour_feature_pooling_amd.functional import nfp
    return (nfp(x, c),)


def _pool(want_gap):
    def call(x, c):
        from neighbour_feature_pooling_amd.functional import nfp_pool
        return nfp_pool(x, c, want_gap=want_gap)
    return call


def _gap(x, c):
    from neighbour_feature_pooling_amd.functional import nfp_with_gap
    return nfp_with_gap(x, c)


def _valid(x, c):
    from neighbour_feature_pooling_amd.functional import nfp_valid
    return (nfp_valid(x, c),)


# (name, op, shape, configuration, flags, (piece of the forward variant, piece of the backward variant))
# flags: "bf16", "nhwc", "nograd" (forward alone, nothing kept for a backward), "ticket" (NFP_POOL_TICKET=1), "bias",
#        "only0" / "only1" (the backward gets the gradient of that output alone)
CASES = [
    ("nfp_cosine_tables", _nfp, (2, 8, 7, 7), ("cosine",), (), ("fwd_band<R1,cos,f32,nchw>", "bwd_fast<R1,cos,f32,nchw>")),
    ("nfp_cosine_bf16_nhwc_mfma", _nfp, (2, 32, 7, 7), ("cosine",), ("bf16", "nhwc"), ("fwd_gram<", ",mfma")),
    ("nfp_cosine_row_bands", _nfp, (2, 8, 24, 24), ("cosine",), (), ("fwd_tile<", "bwd_tile<")),
    ("nfp_l2_k5_table_fwd_band_bwd", _nfp, (2, 8, 14, 14), ("norm", 2, None, dict(p=2)), (), ("fwd_band<R2,l2", "bwd_tile<R2,l2")),
    ("nfp_canberra_7", _nfp, (2, 8, 7, 7), ("canberra",), (), ("fwd_band<R1,canberra", "bwd_fast<R1,canberra")),
    ("nfp_canberra_14", _nfp, (2, 8, 14, 14), ("canberra",), (), ("fwd_band<R1,canberra", "bwd_tile<R1,canberra")),
    ("nfp_attention_f32", _nfp, (2, 8, 7, 7), ("attention",), (), ("fwd_band<R1,dot,f32,nchw>x7+attn_softmax", "bwd_fast<R1,dot")),
    ("nfp_attention_bf16", _nfp, (2, 8, 7, 7), ("attention",), ("bf16",), ("fwd_pairs+attn_softmax", "bwd_gather")),
    ("nfp_two_radii", _nfp, (2, 8, 7, 7), ("cosine", 2, None, dict(inner_R=1)), (), ("fwd_band<R1+2,cos", "bwd_fast<R1+2,cos")),
    ("nfp_pearson", _nfp, (2, 8, 7, 7), ("pearson",), (), ("fwd_pairs", "bwd_gather")),
    ("nfp_stride2", _nfp, (2, 8, 8, 8), ("cosine", 1, 1, dict(stride=2)), (), ("fwd_pairs", "bwd_gather")),
    ("pool_gap_grad", _pool(True), (2, 8, 7, 7), ("cosine",), (), ("fwd_band<R1,cos,f32,nchw,pool>x1", "bwd_fast<R1,cos,f32,nchw,pool>")),
    ("pool_gap_nograd", _pool(True), (2, 8, 7, 7), ("cosine",), ("nograd",), ("fwd_band<R1,cos,f32,nchw,pool>x1", None)),
    ("pool_nogap_grad", _pool(False), (2, 8, 7, 7), ("cosine",), (), ("fwd_band<R1,cos,f32,nchw,pool>x1", "bwd_fast<R1,cos,f32,nchw,pool>")),
    ("pool_nogap_nograd", _pool(False), (2, 8, 7, 7), ("cosine",), ("nograd",), ("fwd_band<R1,cos,f32,nchw,pool>x1", None)),
    ("pool_row_bands_fold", _pool(True), (2, 8, 24, 24), ("cosine",), (), (",pool>x", "bwd_tile<R1,cos,f32,nchw,pool>")),
    ("pool_bf16_nhwc_gram", _pool(True), (2, 16, 7, 7), ("cosine",), ("bf16", "nhwc"), ("fwd_gram<R1,cos,bf16,nhwc,pool>", ",pool>")),
    ("pool_gap_grad_ticket", _pool(True), (2, 8, 7, 7), ("cosine",), ("ticket",), ("fwd_band<R1,cos,f32,nchw,pool>x", "bwd_fast<R1,cos,f32,nchw,pool>")),
    ("pool_row_bands_ticket", _pool(True), (2, 8, 24, 24), ("cosine",), ("ticket",), ("fwd_tile<R1,cos,f32,nchw,pool>x", "bwd_tile<R1,cos,f32,nchw,pool>")),
    ("gap_tables", _gap, (2, 8, 7, 7), ("cosine",), (), ("fwd_band<R1,cos,f32,nchw,gap>x1", "bwd_fast<R1,cos,f32,nchw,gap>")),
    ("gap_row_bands_fold", _gap, (2, 8, 24, 24), ("cosine",), (), (",gap>x", "bwd_tile<R1,cos,f32,nchw,gap>")),
    ("gap_two_radii", _gap, (2, 8, 7, 7), ("cosine", 2, None, dict(inner_R=1)), (), ("fwd_band<R1+2,cos,f32,nchw,gap>x1", "bwd_fast<R1+2,cos,f32,nchw,gap>")),
    ("gap_bf16_nhwc", _gap, (2, 32, 7, 7), ("cosine",), ("bf16", "nhwc"), ("fwd_gram<R1,cos,bf16,nhwc,gap>", ",gap>")),
    ("gap_maps_gradient_alone", _gap, (2, 8, 7, 7), ("norm", 1, None, dict(p=2)), ("only1",), (",gap>", ",gap>")),
    ("gap_gap_gradient_alone", _gap, (2, 8, 7, 7), ("norm", 1, None, dict(p=2)), ("only0",), (",gap>", None)),
    ("valid_cosine", _valid, (2, 8, 7, 7), ("cosine", 1, 0), (), ("fwd_valid<", "bwd_valid<")),
    ("valid_l2", _valid, (2, 8, 7, 7), ("norm", 1, 0, dict(p=2)), (), ("fwd_valid<", "bwd_valid<")),
    ("valid_abs_norm1", _valid, (2, 8, 7, 7), ("norm", 1, 0, dict(p=1)), (), ("fwd_valid<1,l1", "bwd_valid<1,l1")),
    ("valid_abs_emd", _valid, (2, 8, 7, 7), ("emd", 1, 0), (), ("fwd_valid<1,l1", "bwd_valid<1,l1")),
    ("bias_cosine", None, (2, 8, 7, 7), ("cosine",), ("bias",), ("bias_fwd<", "bias_bwd<")),
    ("bias_attention", None, (2, 8, 7, 7), ("attention",), ("bias",), ("+attn_softmax", "+attn_softmax")),
    ("empty_nfp", _nfp, (0, 8, 7, 7), ("cosine",), (), (None, None)),
    ("empty_pool", _pool(True), (0, 8, 7, 7), ("cosine",), (), (None, None)),
    ("empty_gap", _gap, (0, 8, 7, 7), ("cosine",), (), (None, None)),
    ("empty_valid", _valid, (0, 8, 7, 7), ("cosine", 1, 0), (), (None, None)),
    ("empty_valid_abs", _valid, (0, 8, 7, 7), ("norm", 1, 0, dict(p=1)), (), (None, None)),
    ("empty_bias", None, (0, 8, 7, 7), ("cosine",), ("bias",), (None, None)),
]


def digest(t):
    if t is None:
        return "none"
    t = t.detach().cpu().contiguous()
    raw = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
    return "%s%s:%s" % (str(t.dtype).replace("torch.", ""), list(t.shape), hashlib.sha256(raw.numpy().tobytes()).hexdigest())


def run_case(L, case, dev):
    name, op, shape, cargs, flags, _ = case
    measure, R, padding, kw = list(cargs) + [1, None, None][len(cargs) - 1:]      # (measure[, R[, padding[, more]]])
    c = cfg(measure, R, padding, **(kw or {}))
    g = torch.Generator().manual_seed(int(hashlib.sha256(name.encode()).hexdigest()[:6], 16))
    x = torch.rand(*shape, generator=g) + 0.25      # positive: valid for every measure
    x = x.to(dev).to(torch.bfloat16 if "bf16" in flags else torch.float32)
    if "nhwc" in flags:
        x = x.contiguous(memory_format=torch.channels_last)
    leaves = [x]
    if "bias" in flags:
        from neighbour_feature_pooling_amd.functional import nfp_biased
        C, N = shape[1], c.out_channels
        leaves += [(torch.rand(C, generator=g) - 0.5).to(dev), (torch.rand(C * N, generator=g) - 0.5).to(dev)]
        op = lambda x_, c_: (nfp_biased(x_, c_, leaves[1], leaves[2]),)
    if "nograd" not in flags:
        for t in leaves:
            t.requires_grad_(True)
    torch.cuda.synchronize()
    n0 = L.nfp_launch_count()
    res = {}
    with torch.set_grad_enabled("nograd" not in flags):
        outs = op(x, c)
    torch.cuda.synchronize()
    res["variant_fwd"] = L.nfp_last_variant().decode()
    for i, o in enumerate(outs):
        res["out%d" % i] = digest(o)
    if "nograd" not in flags:
        keep = [i for i, o in enumerate(outs) if o is not None and not ("only0" in flags and i != 0) and not ("only1" in flags and i != 1)]
        gos = [torch.randn(outs[i].shape, generator=g).to(dev).to(outs[i].dtype) for i in keep]
        grads = torch.autograd.grad([outs[i] for i in keep], leaves, gos, allow_unused=True)
        torch.cuda.synchronize()
        res["variant_bwd"] = L.nfp_last_variant().decode()
        for i, gr in enumerate(grads):
            res["grad%d" % i] = digest(gr)
    res["launches"] = L.nfp_launch_count() - n0
    return res


def main():
    a = ARGS
    assert torch.cuda.is_available(), "entry_bits.py runs the kernels; it needs the GPU"
    from neighbour_feature_pooling_amd import _abi, functional
    L = _abi.load()
    dev = torch.device("cuda:0")
    got, off_route = {}, []
    for ticket in (False, True):
        os.environ.pop("NFP_POOL_TICKET", None)
        if ticket:
            os.environ["NFP_POOL_TICKET"] = "1"
        L.nfp_reload_env()
        functional._PLANS.clear()
        for case in CASES:
            if ("ticket" in case[4]) != ticket:
                continue
            try:
                r = run_case(L, case, dev)
            except Exception as e:      # (a refusal is an answer too: an empty batch of plain nfp has null tensors)
                r = dict(error="%s: %s" % (type(e).__name__, e), launches=-1)
            got[case[0]] = r
            print("%-30s %2d launches  %s | %s" % (case[0], r["launches"], r.get("variant_fwd", r.get("error")), r.get("variant_bwd", "-")))
            for want, key in zip(case[5], ("variant_fwd", "variant_bwd")):
                if want is not None and want not in r.get(key, ""):
                    off_route.append("%s %s: expected '%s' in '%s'" % (case[0], key, want, r.get(key)))
    os.environ.pop("NFP_POOL_TICKET", None)
    L.nfp_reload_env()
    functional._PLANS.clear()
    with open(a.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
    n = sum(len(v) for v in got.values())
    print("%d cases, %d fields -> %s" % (len(got), n, a.out))
    for line in off_route:
        print("OFF ROUTE " + line)
    if not a.against:
        return 2 if off_route else 0
    with open(a.against) as f:
        ref = json.load(f)
    bad = [(c, t) for c in sorted(set(got) | set(ref)) for t in sorted(set(got.get(c, {})) | set(ref.get(c, {})))
           if got.get(c, {}).get(t, "missing") != ref.get(c, {}).get(t, "missing")]
    for c, t in bad:
        print("DIFFERS %s %s: %s (was %s)" % (c, t, got.get(c, {}).get(t, "missing"), ref.get(c, {}).get(t, "missing")))
    print("%d of %d fields differ from %s" % (len(bad), n, a.against))
    return 1 if bad else (2 if off_route else 0)


if __name__ == "__main__":
    sys.exit(main())
