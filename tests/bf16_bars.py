"""The per-element bars for maps and grad_x in plain bf16 storage, and the float64 formulation they are taken against.

Derived, not measured.  ULP = 2^-8 (one_rounding.ULP): round-to-nearest to bf16 lands within ULP |v| of v.  `ref` is the
float64 result on the bf16-rounded inputs; `slack` the bar the suite holds the same kernel family to in float32 storage.

Maps.  `out` is ONE round-to-nearest of a float32 value: `one_rounding_excess(out, ref_out, slack) <= 1`, as in
tests/one_rounding.py (`out_excess` with extra=None).

grad_x.  The backward computes in float32 from exactly representable x and grad_out and from the ROUNDED `out`
(Meas<M>::coef, csrc/nfp_measures.h), and rounds once at the store.  A relative error of ULP in `out` moves every sub-term of
the gradient that contains `out` by at most ULP (1 + 2 ULP) of itself (1 / out: ULP + ULP^2 + ...), so per element e

    |got[e] - ref[e]| <= ULP |ref[e]| + ULP (1 + 2 ULP) S[e] + (1 + ULP) slack max|ref|

S[e]: the sum, over every (centre, neighbour) pair e takes part in, of the absolute values of those sub-terms —
  L2 (norm p = 2), RMSE   the whole term, |go| |a_c - b_c| / d (RMSE: / C), for both pixels of the pair;
  cosine                  the two self terms, |go| |outv| |a_c| / (|a| max(|a|, eps)) and the same for b (`outv` the value as
                          stored: 1 - s under similarity=False);
  GFC                     the two self terms as Meas<NFP_GFC>::coef has them, |go| |outv| |b| |a_c| / ((|a||b| + eps) |a|);
  DotProduct              none: S = 0, the plain one-rounding bar.
Contributions through the padding fold onto their source pixel as the gradient does: autograd of F.pad folds them.

Two families have one further derived term each:
  fwd_gram, L2 maps (csrc/nfp_mfma.h)   d^2 = G_pp + G_qq - 2 G_pq from three float32 sums of C exact products:
      |delta d| <= C 2^-24 (G_pp + G_qq + 2 |G_pq|) / (2 d)  — `gram_out`, the `extra` of `out_excess`; through S it reaches
      grad_x: a pair's relative error in `out` is ULP + (1 + ULP) gram_out / d instead of ULP — `S_gram`, in units of ULP.
  bwd_fast<...,mfma> / <...,mfma2> (csrc/nfp_fast.h, wd_put_at)   every GEMM weight is two truncated bf16 halves, 16
      significand bits: + 2^-15 T[e] (`MFMA_EPS`), T the backward with every product replaced by its absolute value.

`reference` is a float64 torch formulation from F.pad and strided slices with the backward written out per pair (the
kernels' coef / grad split), so that it can also be evaluated from a STORED out (`out_stored`: the emulation of the specified
arithmetic, tests/test_bf16_bars_host.py) — any R, stride, padding, dilation, the four padding modes, either `similarity`;
tests/test_bf16_bars_host.py holds its signed out / grad_x to the pinned oracle."""
import numpy as np
import torch
import torch.nn.functional as F

from one_rounding import ULP, one_rounding_excess      # noqa: F401  (re-exported)

MFMA_EPS = 2.0 ** -15
MEASURES = ("cosine", "dot", "gfc", "norm", "rmse")
_PAD = {"zeros": "constant", "reflect": "reflect", "replicate": "replicate", "circular": "circular"}
_CHUNK = 1 << 22        # elements of one [b,C,N,Ho,Wo] piece: the batch is walked in pieces (images are independent)


def _taps(x, cfg):
    R, pad, s, d = cfg.R, cfg.padding, cfg.stride, cfg.dilation
    k = 2 * R + 1
    xp = F.pad(x, (pad,) * 4, mode=_PAD[cfg.padding_mode]) if pad > 0 else x
    Ho, Wo = ((v - d * (k - 1) - 1) // s + 1 for v in xp.shape[-2:])
    assert Ho >= 1 and Wo >= 1, (tuple(x.shape), Ho, Wo)
    tap = lambda ky, kx: xp[:, :, ky * d: ky * d + (Ho - 1) * s + 1: s, kx * d: kx * d + (Wo - 1) * s + 1: s]   # noqa: E731
    b = torch.stack([tap(t // k, t % k) for t in range(k * k) if t != (k * k) // 2], dim=2)
    return tap(R, R).unsqueeze(2), b          # [b,C,1,Ho,Wo], [b,C,N,Ho,Wo]


def _safe_inv(v):
    return torch.where(v > 0, 1.0 / torch.where(v > 0, v, torch.ones_like(v)), torch.zeros_like(v))


def _piece(x, go, cfg, out_stored, coef_hook):
    """One piece of the batch: float64 tensors in, (out, grad_x, S, T, gram_out, S_gram) out."""
    m, sim, eps, C = cfg.measure, bool(cfg.similarity), float(cfg.eps), x.shape[1]
    assert m in MEASURES and (m != "norm" or (cfg.p == 2 and cfg.diff_weights)), cfg
    x = x.clone().requires_grad_(True)
    a, b = _taps(x, cfg)
    with torch.no_grad():
        ad, bd = a.detach(), b.detach()
        dot = (ad * bd).sum(1, keepdim=True)                       # [b,1,N,Ho,Wo]
        na, nb = ad.square().sum(1, keepdim=True).sqrt(), bd.square().sum(1, keepdim=True).sqrt()
        g = go.unsqueeze(1)
        hook = coef_hook or (lambda k: k)
        gram_out = None
        if m in ("norm", "rmse"):
            d = (ad - bd).square().sum(1, keepdim=True).sqrt()
            if m == "rmse":
                d = d / np.sqrt(C)
            out = -d if sim else d
            outv = out if out_stored is None else out_stored.unsqueeze(1)
            sg = -g if sim else g
            if m == "norm":                                         # MeasNorm<2>::coef: 0 at d == 0
                k0 = torch.where(outv.abs() == 0, torch.zeros_like(g), sg / torch.where(outv.abs() == 0, torch.ones_like(outv), outv.abs()))
                E = C * 2.0 ** -24 * (na.square() + nb.square() + 2 * dot.abs())
                gram_out = torch.where(d > 0, E / (2 * torch.where(d > 0, d, torch.ones_like(d))), E.sqrt())
                rho = torch.where(d > 0, 1.0 + (1 + ULP) * gram_out / (ULP * torch.where(d > 0, d, torch.ones_like(d))), torch.ones_like(d))
            else:                                                   # Meas<NFP_RMSE>::coef: inf at d == 0, NaN below, as torch
                k0 = sg / (outv.abs() * C)
            k0 = hook(k0)
            da = k0 * (ad - bd)
            db = -da
            Sa = Sb = Ta = Tb = da.abs()
        elif m == "dot":
            out = dot if sim else -dot
            k0 = hook(g if sim else -g)
            da, db = k0 * bd, k0 * ad
            Ta, Tb = da.abs(), db.abs()
            Sa = Sb = torch.zeros_like(da)
        elif m == "cosine":
            ia, ib = 1.0 / na.clamp_min(eps), 1.0 / nb.clamp_min(eps)
            s = dot * ia * ib
            out = s if sim else 1 - s
            outv = out if out_stored is None else out_stored.unsqueeze(1)
            sv = outv if sim else 1 - outv
            sg = g if sim else -g
            k0, k1, k2 = hook(sg * ia * ib), hook(sg * sv * _safe_inv(na) * ia), hook(sg * sv * _safe_inv(nb) * ib)
            da, db = k0 * bd - k1 * ad, k0 * ad - k2 * bd
            Sa, Sb = (g * outv * _safe_inv(na) * ia * ad).abs(), (g * outv * _safe_inv(nb) * ib * bd).abs()
            Ta, Tb = (k0 * bd).abs() + (k1 * ad).abs(), (k0 * ad).abs() + (k2 * bd).abs()
        else:                                                       # gfc
            den = na * nb + eps
            f = dot / den
            out = f if sim else -f
            outv = out if out_stored is None else out_stored.unsqueeze(1)
            sgn = 1.0 if sim else -1.0
            num = sgn * outv * den
            k0 = hook(g * sgn / den)
            k1, k2 = hook(g * sgn * num * nb * _safe_inv(na) / den.square()), hook(g * sgn * num * na * _safe_inv(nb) / den.square())
            da, db = k0 * bd - k1 * ad, k0 * ad - k2 * bd
            Sa, Sb = (k1 * ad).abs(), (k2 * bd).abs()
            Ta, Tb = (k0 * bd).abs() + Sa, (k0 * ad).abs() + Sb
    # the fold through the padding, the stride and the window: autograd of F.pad and of the slices
    fold = lambda wa, wb: torch.autograd.grad((wa * a).sum() + (wb * b).sum(), x, retain_graph=True)[0]     # noqa: E731
    res = [out.squeeze(1), fold(da, db), fold(Sa, Sb), fold(Ta, Tb)]
    if gram_out is not None:
        res += [gram_out.squeeze(1), fold(Sa * rho, Sb * rho)]
    else:
        res += [torch.zeros_like(res[0]), res[2]]
    return res


def reference(x, go, cfg, out_stored=None, coef_hook=None):
    """x [B,C,H,W], go [B,N,Ho,Wo] (numpy, the values the kernels read) and a configuration (functional.NfpConfig, or
    anything with its fields) -> dict of float64 numpy arrays: out, grad_x, S, T, gram_out, S_gram (module docstring).
    `out_stored`: the backward reads this `out` in place of its own (the arithmetic of bf16 storage); `coef_hook`: applied to
    every per-pair coefficient of the backward (a mutant of tests/test_bf16_bars_host.py rounds them to bf16)."""
    xt, got = torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(go, np.float64))
    ost = None if out_stored is None else torch.from_numpy(np.asarray(out_stored, np.float64))
    B, C = xt.shape[:2]
    per_image = max(1, C * got[0].numel())
    step = max(1, _CHUNK // per_image)
    pieces = [_piece(xt[i:i + step], got[i:i + step], cfg, None if ost is None else ost[i:i + step], coef_hook)
              for i in range(0, B, step)]
    names = ("out", "grad_x", "S", "T", "gram_out", "S_gram")
    return {n: torch.cat([p[j] for p in pieces]).numpy() for j, n in enumerate(names)}


def _excess(got, ref, bar_of):
    """max |got - ref| / bar over the elements where `ref` is a number; inf when the shapes or the NaN patterns differ
    (one_rounding_excess's handling)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return float("inf")
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return float("inf")
    if nan.all():
        return 0.0
    g, r = got[~nan], ref[~nan]
    with np.errstate(invalid="ignore"):
        diff = np.where(g == r, 0.0, np.abs(g - r))
    bar = bar_of(r, ~nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff == 0.0, 0.0, diff / bar)
    return float(np.max(np.where(np.isnan(ratio), np.inf, ratio)))


def out_excess(got, ref, slack, extra=None):
    """one_rounding_excess with a per-element term `extra` beside the slack (fwd_gram's `gram_out`): the float32 value that
    is rounded lies within slack max|ref| + extra[e] of the reference."""
    if extra is None:
        return one_rounding_excess(got, ref, slack)
    ex = np.asarray(extra, np.float64)
    return _excess(got, ref, lambda r, keep: ULP * np.abs(r) + (1.0 + ULP) * (slack * float(np.max(np.abs(r))) + ex[keep]))


def grad_x_excess(got, ref, S, slack, T=None, eps_T=0.0):
    """max over elements of |got - ref| / (ULP |ref| + ULP (1 + 2 ULP) S + (1 + ULP) slack max|ref| [+ eps_T T]); a result
    passes at <= 1.  NaN patterns as one_rounding_excess takes them."""
    S = np.asarray(S, np.float64)
    T = None if T is None else np.asarray(T, np.float64)

    def bar_of(r, keep):
        bar = ULP * np.abs(r) + ULP * (1.0 + 2.0 * ULP) * S[keep] + (1.0 + ULP) * slack * float(np.max(np.abs(r)))
        return bar if T is None else bar + eps_T * T[keep]

    return _excess(got, ref, bar_of)
