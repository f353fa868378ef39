#!/usr/bin/env python3
"""Where does the eager host time of one NFP forward + backward go?  (cProfile over 3000 steps.)

--op     which call: nfp (the default: NFPPooling, cosine, padding 1), valid / valid_abs (functional.nfp_valid, padding 0:
         cosine / Norm p = 1) or with_gap (functional.nfp_with_gap, cosine, padding 1) — all on a [64, 512, 7, 7] input
--root   the tree whose package is imported (default: this script's own): the same script times another checkout
NFP_PY_NODES=1 in the environment selects the Python autograd nodes."""
import argparse, cProfile, pstats, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--op", choices=["nfp", "valid", "valid_abs", "with_gap"], default="nfp")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch
from neighbour_feature_pooling_amd import NFPPooling, NfpConfig, nfp_valid, nfp_with_gap
x = torch.randn(64, 512, 7, 7, device="cuda", requires_grad=True)
if args.op == "nfp":
    m = NFPPooling(512, R=1, measure="cosine", padding=1)
elif args.op == "with_gap":
    cfg = NfpConfig(R=1, measure="cosine", padding=1, diff_weights=False)
    m = lambda t: nfp_with_gap(t, cfg)[1]
else:
    cfg = NfpConfig(R=1, measure="cosine", padding=0, diff_weights=False) if args.op == "valid" else \
        NfpConfig(R=1, measure="norm", p=1, padding=0, diff_weights=True)
    m = lambda t: nfp_valid(t, cfg)
with torch.no_grad():
    go = torch.randn_like(m(x))


def step():
    out = m(x)
    torch.autograd.grad(out, x, go)


for _ in range(200):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(3000):
    step()
torch.cuda.synchronize()
print(f"eager: {(time.perf_counter() - t0) / 3000 * 1e6:.1f} us per fwd+bwd")
t0 = time.perf_counter()
with torch.no_grad():
    for _ in range(3000):
        m(x)
torch.cuda.synchronize()
print(f"eager forward only (no grad): {(time.perf_counter() - t0) / 3000 * 1e6:.1f} us")
pr = cProfile.Profile()
pr.enable()
for _ in range(3000):
    step()
pr.disable()
torch.cuda.synchronize()
st = pstats.Stats(pr)
st.sort_stats("tottime").print_stats(18)
