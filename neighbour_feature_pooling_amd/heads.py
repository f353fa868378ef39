"""The heads the reference trains — drop-ins for models/nfp_heads.py::NFPHead (nfp_heads.py:11-46), MultiRadiusNFPHead
(80-118) and AdaptiveFusionNFP (283-332).

Same constructor signatures, attributes and state-dict keys; the RNG is consumed in the reference's order (each NFP layer's
two depthwise conv weights — drawn and dropped, NFPPooling(bias=False) holds no conv — then the constructor's
torch.randn(1, in_c, 7, 7) probe, then compress and the MLP / gate), so the same seed gives bit-identical parameters.
`compress` stays the reference's nn.Sequential(Conv2d 1x1, BatchNorm2d, ReLU) as the parameter holder; forward() does not
call it: GAP(fmap) and the maps come from one pass (NFPWithGap; radii (1, 2) from the single pass where served), the tail
GAP(compress(maps)) from functional.nfp_compress_pool, which on the GPU never forms the [B,D,H,W] activation, and only the
head's own MLP or gate runs as ATen ops.

NFPHead_NoConv (nfp_heads.py:50-77) is left out: as written it cannot run in the reference (its MLP expects in_c pooled
NFP channels, the layer yields 8: "mat1 and mat2 shapes cannot be multiplied").
"""
import torch
import torch.nn as nn

from .functional import nfp_compress_pool
from .nfp import EnhancedNFPPooling, MultiRadiusNFPPooling, NFPWithGap


def _reference_layer_draws(layer):
    """The draws of the reference layer's two depthwise convs (nfp.py:42-59: comp_neighbors, then center_value), which it
    overwrites at once — as SimilarityAwarePooling.__init__ makes them."""
    C, k = int(layer.in_channels), layer.kernel_size
    nn.Conv2d(C, layer.out_channels * C, k, groups=C, bias=False)
    nn.Conv2d(C, C, k, groups=C, bias=False)


def _compress(n_maps, bottleneck_dim):
    return nn.Sequential(nn.Conv2d(n_maps, bottleneck_dim, 1, bias=False), nn.BatchNorm2d(bottleneck_dim),
                         nn.ReLU(inplace=True))


def _gap_and_tail(gap_nfp, compress, fmap):
    """(GAP(fmap), GAP(compress(NFP(fmap)))) [B,C], [B,D], both in the tail's dtype."""
    gap_vec, maps = gap_nfp(fmap)
    nfp_vec = nfp_compress_pool(maps.to(fmap.dtype), compress[0].weight, compress[1])
    return gap_vec.to(nfp_vec.dtype), nfp_vec


class NFPHead(nn.Module):
    """GAP(fmap) beside the compressed maps of one NFP layer (R = 1 by default), fused by an MLP: [B,in_c,H,W] ->
    [B,bottleneck_dim]."""

    def __init__(self, in_c=512, bottleneck_dim=512, R=1, measure="cosine"):
        super().__init__()
        self.nfp = EnhancedNFPPooling(in_channels=in_c, R=R, measure=measure, padding=R)
        _reference_layer_draws(self.nfp)
        with torch.no_grad():                                   # nfp_heads.py:24-27
            dummy = torch.randn(1, in_c, 7, 7)
            self.nfp_out_channels = self.nfp(dummy).shape[1]
        self.compress = _compress(self.nfp_out_channels, bottleneck_dim)
        self.gap = nn.AdaptiveAvgPool2d(1)
        self.fusion_mlp = nn.Sequential(nn.Linear(in_c + bottleneck_dim, bottleneck_dim), nn.ReLU(inplace=True),
                                        nn.Linear(bottleneck_dim, bottleneck_dim))
        object.__setattr__(self, "_gap_nfp", NFPWithGap(self.nfp))      # (a view of self.nfp: no second state-dict entry)

    def forward(self, fmap):
        gap_vec, nfp_vec = _gap_and_tail(self._gap_nfp, self.compress, fmap)
        return self.fusion_mlp(torch.cat([gap_vec, nfp_vec], dim=1))


class MultiRadiusNFPHead(nn.Module):
    """GAP(fmap) plus a gated share of the compressed maps of one NFP layer per radius (default R = 1, 2: 8 + 24 maps),
    fused = gap + sigmoid(MLP(cat(gap, nfp_vec))) * nfp_vec — bottleneck_dim must equal in_c for the sum, as in the reference."""

    def __init__(self, in_c=512, bottleneck_dim=512, R_list=(1, 2), measure="cosine"):
        super().__init__()
        layers = MultiRadiusNFPPooling(in_c, R_list=tuple(R_list), measure=measure)
        self.nfp_blocks = layers.nfp_blocks                     # (the reference's ModuleList: nfp_heads.py:87-94)
        for blk in self.nfp_blocks:
            _reference_layer_draws(blk)
        with torch.no_grad():                                   # nfp_heads.py:95-97
            dummy = torch.randn(1, in_c, 7, 7)
            total_c = sum(b(dummy).shape[1] for b in self.nfp_blocks)
        self.compress = _compress(total_c, bottleneck_dim)
        self.se_gate = nn.Sequential(nn.Linear(in_c + bottleneck_dim, (in_c + bottleneck_dim) // 2), nn.ReLU(inplace=True),
                                     nn.Linear((in_c + bottleneck_dim) // 2, 1), nn.Sigmoid())
        self.gap = nn.AdaptiveAvgPool2d(1)
        object.__setattr__(self, "_gap_nfp", NFPWithGap(layers))        # (a view of self.nfp_blocks)

    def forward(self, fmap):
        gap_vec, nfp_vec = _gap_and_tail(self._gap_nfp, self.compress, fmap)
        alpha = self.se_gate(torch.cat([gap_vec, nfp_vec], dim=1))
        return gap_vec + alpha * nfp_vec


class AdaptiveFusionNFP(nn.Module):
    """GAP(x) plus a gated share of the compressed maps of one NFP layer, then dropout: fused = gap + alpha * nfp_feat."""

    def __init__(self, in_channels=512, bottleneck_dim=512, R=1, measure='cosine', dropout_p=0.2):
        super().__init__()
        self.gap = nn.AdaptiveAvgPool2d((1, 1))
        self.nfp = EnhancedNFPPooling(in_channels=in_channels, R=R, measure=measure, padding=R)
        _reference_layer_draws(self.nfp)
        with torch.no_grad():                                   # nfp_heads.py:295-298
            dummy = torch.randn(1, in_channels, 7, 7)
            nfp_out = self.nfp(dummy)
            self.nfp_dim = nfp_out.view(1, -1).size(1)
        self.compress = _compress(nfp_out.shape[1], bottleneck_dim)
        fusion_dim = in_channels + bottleneck_dim
        self.fusion_gate = nn.Sequential(nn.Linear(fusion_dim, fusion_dim // 2), nn.ReLU(inplace=True),
                                         nn.Linear(fusion_dim // 2, 1), nn.Sigmoid())
        self.dropout = nn.Dropout(p=dropout_p)
        object.__setattr__(self, "_gap_nfp", NFPWithGap(self.nfp))      # (a view of self.nfp)

    def forward(self, x):
        gap_feat, nfp_feat = _gap_and_tail(self._gap_nfp, self.compress, x)
        alpha = self.fusion_gate(torch.cat([gap_feat, nfp_feat], dim=1))
        return self.dropout(gap_feat + alpha * nfp_feat)
