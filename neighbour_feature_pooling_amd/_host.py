"""NFP on HOST (CPU) tensors, in plain torch ops.

Why this exists: the reference's heads call their NFP layer on a CPU dummy inside
__init__ to probe the output channels (models/nfp_heads.py:24-27,95-97,166-167,
models/resnet18.py:22-25), so a drop-in module must accept CPU tensors.  It is
NOT a fallback: a CUDA tensor never reaches this file (functional.nfp raises if
the HIP library cannot serve it), and nothing here touches oracle/.

Formulation: pad once, then every kernel tap is a strided slice of the padded
map (no depthwise one-hot convolutions as in nfp.py:42-82); the measures follow
nfp.py:141-374 on the stacked [B,C,N,Ho,Wo] neighbours; autograd differentiates.
"""
import torch
import torch.nn.functional as F

_PAD = {"zeros": "constant", "reflect": "reflect", "replicate": "replicate", "circular": "circular"}


def _taps(x, cfg):
    R, pad, s, d = cfg.R, cfg.padding, cfg.stride, cfg.dilation
    k = 2 * R + 1
    xp = F.pad(x, (pad, pad, pad, pad), mode=_PAD[cfg.padding_mode]) if pad > 0 else x
    Hp, Wp = xp.shape[-2:]
    span = d * (k - 1) + 1
    Ho, Wo = (Hp - span) // s + 1, (Wp - span) // s + 1
    if Ho < 1 or Wo < 1:
        raise RuntimeError(f"Kernel size can't be greater than actual input size ({Hp}x{Wp} padded, span {span})")

    def tap(ky, kx):
        return xp[:, :, ky * d: ky * d + (Ho - 1) * s + 1: s, kx * d: kx * d + (Wo - 1) * s + 1: s]

    centre = tap(R, R)
    neigh = torch.stack([tap(t // k, t % k) for t in range(k * k) if t != (k * k) // 2], dim=2)
    return centre.unsqueeze(2), neigh  # [B,C,1,Ho,Wo], [B,C,N,Ho,Wo]


def nfp_host(x, cfg, centre_bias=None, neighbour_bias=None):
    """centre_bias [C] / neighbour_bias [C*N] (NFPPooling(bias=True)): the biases of the reference's two convs, added
    after padding (a zero-padded tap reads 0 + bias); neighbour_bias in the reshape order of nfp.py:136-139."""
    a, b = _taps(x, cfg)
    m, sim, eps = cfg.measure, cfg.similarity, cfg.eps
    v = (a - b) if cfg.diff_weights else b  # what the reference's comp_neighbors conv yields
    if neighbour_bias is not None:
        beta = neighbour_bias.to(x.dtype).reshape(1, b.shape[1], b.shape[2], 1, 1)
        v, b = v + beta, b + beta
    if centre_bias is not None and m not in ("norm", "rmse"):   # (Norm and RMSE never call center_value: nfp.py:141-148,172-179)
        a = a + centre_bias.to(x.dtype).reshape(1, a.shape[1], 1, 1, 1)
    if m == "norm":
        r = torch.linalg.norm(v, ord=cfg.p, dim=1)
        return -r if sim else r
    if m == "rmse":
        r = torch.sqrt(torch.mean(v ** 2, dim=1))
        return -r if sim else r
    if m == "cosine":
        r = F.cosine_similarity(a, b, dim=1, eps=eps)
        return r if sim else 1 - r
    if m == "dot":
        r = (a * b).sum(1)
        return r if sim else -r
    if m == "attention":
        r = F.softmax((a * b).sum(1), dim=1)
        return r if sim else -r
    if m == "geman":
        q = (a - b) ** 2
        r = (q / (q + eps)).mean(1)
        return r if sim else 1 - r
    if m == "emd":
        r = (a - b).abs().sum(1)
        return -r if sim else r
    if m == "canberra":
        r = ((a - b).abs() / (a.abs() + b.abs() + eps)).sum(1)
        return -r if sim else r
    if m in ("hellinger", "squaredchord"):
        q = ((a.abs() + eps).sqrt() - (b.abs() + eps).sqrt()) ** 2
        r = torch.sqrt(0.5 * q.sum(1)) if m == "hellinger" else q.sum(1)
        return -r if sim else r
    if m == "chisquared1":
        r = ((a - b) ** 2 / (a.abs() + b.abs() + eps)).sum(1)
        return -r if sim else r
    if m == "chisquared2":
        r = ((a - b) ** 2 / (a.abs() + eps)).sum(1)
        return -r if sim else r
    if m == "gfc":
        r = (a * b).sum(1) / (torch.norm(a, dim=1) * torch.norm(b, dim=1) + eps)
        return r if sim else -r
    if m == "pearson":
        ac, bc = a - a.mean(1, keepdim=True), b - b.mean(1, keepdim=True)
        r = (ac * bc).sum(1) / torch.sqrt((ac ** 2).sum(1) * (bc ** 2).sum(1) + eps)
        return r if sim else -r
    if m == "jeffrey":
        ca, cb = a.abs() + eps, b.abs() + eps
        r = (ca * torch.log(ca / cb) + cb * torch.log(cb / ca)).sum(1)
        return -r if sim else r
    if m == "smith":
        A, Bn = a.abs(), b.abs()
        r = 1 - torch.minimum(A, Bn).sum(1) / (torch.minimum(A.sum(1), Bn.sum(1)) + eps)
        return r if sim else -r
    if m == "scs":
        # nfp.py:359-374 — the (B,N,H,W)/(B,1,N,H,W) division broadcasts to (B,B,N,H,W) and
        # mean(dim=1) then averages over the batch; reproduced as written in the reference.
        na = torch.norm(a, dim=1, keepdim=True) + cfg.q_scs
        nb = torch.norm(b, dim=1, keepdim=True) + cfg.q_scs
        c = (a * b).sum(1) / (na * nb)
        r = torch.nan_to_num(torch.sign(c) * c.abs() ** cfg.p, nan=0.0, posinf=0.0, neginf=0.0)
        if not sim:
            r = 1 - r
        return r.mean(dim=1)
    raise RuntimeError(f"Similarity measure {m} not implemented")


def attention_pool_host(maps, w, b):
    """The tail of SimilarityAwarePooling.forward (models/nfp_heads.py:224-232) in plain torch ops, any dtype and device:
    maps [B,N,...] -> [B,N], att = softmax over the pixels of the 1x1 conv (w [N] or [1,N,1,1], b [1]) of the maps, the
    maps summed under it.  Autograd differentiates."""
    B, N = maps.shape[:2]
    m = maps.reshape(B, N, -1)
    logits = (m * w.reshape(1, N, 1).to(m.dtype)).sum(1) + b.reshape(1, 1).to(m.dtype)
    att = torch.softmax(logits, dim=-1)
    return (m * att.unsqueeze(1)).sum(-1)


def deepten_host(x, codewords, scale):
    """The Deep-TEN encoding layer (models/deepten.py::DeepTENEncoding.forward) in plain torch ops, any dtype, device and
    strides: x [B,D,H,W], codewords [K,D], scale [K] -> [B, K*D].  The residuals pixel - codeword [B,N,K,D] are formed
    twice, as the reference forms them — for the squared distances behind the softmax over the codewords, and for the
    sum over the pixels under it.  Mixed dtypes promote as torch promotes them; outside torch.autocast the result is cast
    to x's dtype.  Autograd differentiates."""
    B, D = x.shape[:2]
    K = codewords.shape[0]
    pix = x.flatten(2).transpose(1, 2)                                              # [B,N,D]
    dist = (pix.unsqueeze(2) - codewords.reshape(1, 1, K, D)).pow(2).sum(dim=3)      # [B,N,K]
    assign = torch.softmax(-scale.reshape(1, 1, K) * dist, dim=2)
    resid = pix.unsqueeze(1) - codewords.reshape(1, K, 1, D)                        # [B,K,N,D]
    enc = (assign.transpose(1, 2).unsqueeze(3) * resid).sum(dim=2).reshape(B, K * D)
    return enc if torch.is_autocast_enabled(x.device.type) else enc.to(x.dtype)


def compress_conv(maps, weight):
    """The 1x1 conv of the two compositions below: maps [B,N,H,W] (or [B,N,P], taken as [B,N,P,1]) under weight [D,N,1,1] or
    [D,N] -> [B,D,H,W] ([B,D,P,1])."""
    B, N = maps.shape[:2]
    return F.conv2d(maps if maps.dim() == 4 else maps.reshape(B, N, -1, 1), weight.reshape(weight.shape[0], N, 1, 1))


def compress_finish(y, maps, relu, pool):
    """... and what follows their BatchNorm on its output y: the ReLU where asked, then GAP -> [B,D] (pool), or the map in
    the shape of `maps`."""
    y = F.relu(y) if relu else y
    if pool:
        return y.mean((2, 3))
    return y if maps.dim() == 4 else y.reshape(maps.shape[0], y.shape[1], *maps.shape[2:])


def compress_pool_host(maps, weight, gamma, beta, running_mean, running_var, use_batch_stats, momentum, eps):
    """The tail the heads of models/nfp_heads.py share (NFPHead nfp_heads.py:28-32,42-43): GAP(relu(batch_norm(conv1x1(maps))))
    as the four ATen ops — conv2d, batch_norm, relu, mean — any dtype and device, under torch.compile and torch.autocast:
    maps [B,N,H,W] (or [B,N,P]) -> [B,D].  weight [D,N,1,1] or [D,N]; gamma / beta may be None (affine=False); the running
    statistics, where given, are updated in place by batch_norm when use_batch_stats (momentum: its exponential factor).
    Autograd differentiates."""
    y = F.batch_norm(compress_conv(maps, weight), running_mean, running_var, gamma, beta, use_batch_stats, momentum, eps)
    return compress_finish(y, maps, True, True)


def compress_map_host(maps, weight, gamma, beta, running_mean, running_var, use_batch_stats, momentum, eps, relu=True):
    """The projection of NFP maps that keeps the map — NFPInsert's nfp_proj (models/mobilenetv3.py:346-350) and, with
    relu=False, NFPBottleneck's bn2(conv2(.)) (models/nfp_heads.py:270-272): [relu](batch_norm(conv1x1(maps))) as the ATen
    ops, any dtype and device, under torch.compile and torch.autocast: maps [B,N,H,W] (or [B,N,P]) -> [B,D,H,W] ([B,D,P]).
    weight [D,N,1,1] or [D,N]; gamma / beta may be None (affine=False); the running statistics, where given, are updated in
    place by batch_norm when use_batch_stats (momentum: its exponential factor).  Autograd differentiates."""
    y = F.batch_norm(compress_conv(maps, weight), running_mean, running_var, gamma, beta, use_batch_stats, momentum, eps)
    return compress_finish(y, maps, relu, False)
