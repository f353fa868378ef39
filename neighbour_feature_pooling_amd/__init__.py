"""neighbour_feature_pooling_amd — MI355X (gfx950) Neighbourhood Feature Pooling.

Drop-in for the reference's NFP hot path:
    NFPPooling, EnhancedNFPPooling   <- models/pooling/nfp.py::NFPPooling
    nfp_pooling                      <- models/NFP_Pooling.py::nfp_pooling
    MultiRadiusNFPPooling            <- the per-radius layers + concatenation of models/nfp_heads.py::MultiRadiusNFPHead
    nfp_op, nfp_pool, NfpConfig      functional forms (autograd ops over libnfp_hip.so)
    nfp_with_gap, NFPWithGap         <- gap(fmap) and nfp(fmap) of one feature map, the first step of models/nfp_heads.py's heads
                                        (NFPWithGap over a MultiRadiusNFPPooling: MultiRadiusNFPHead's gap + 32 maps, one pass)
    SimilarityAwarePooling           <- models/nfp_heads.py::SimilarityAwarePooling (attention-weighted sum of unpadded NFP maps)
    nfp_attention_pool               its tail (1x1 conv, softmax over the pixels, weighted sum) as one op
    NFPBottleneck                    <- models/nfp_heads.py::NFPBottleneck (a residual block around an unpadded cosine NFP layer)
    nfp_valid                        `nfp_op` for padding = 0 on the valid-map kernels (one launch each way)
    nfp_strided                      `nfp_op` for stride 2 to 4 on the strided row-band kernels (one launch each way; opt-in)
    NFPHead, MultiRadiusNFPHead,     <- models/nfp_heads.py: the three heads the reference trains (GAP + compressed NFP maps,
    AdaptiveFusionNFP                   fused by an MLP or a gate)
    nfp_compress_pool                their shared tail GAP(relu(bn(conv1x1(maps)))) as one op, without the [B,D,H,W] activation
    NFPInsert                        <- the nfp + nfp_proj block of models/mobilenetv3.py::MOBILENETV3_NFP_INSERT (345-353)
    nfp_compress_map                 its projection [relu](bn(conv1x1(maps))) as one op that keeps the map (models.NFPInsertNet:
                                        the whole net; NFPBottleneck(fused_project=True): the same op without the ReLU)
                                     (both ops follow an nn.SyncBatchNorm across the ranks of its process group: README,
                                        "SyncBatchNorm in the fused tails")
    nfp_pooled                       <- F.adaptive_avg_pool2d(NFPPooling(feat), 1) of models/texture_pooling.py:251-252, 320-321
    DeepTENEncoding                  <- models/deepten.py::DeepTENEncoding, the Deep-TEN baseline's encoding layer, without its
    nfp_deepten_encode                  [B,N,K,D] residual tensor (models.DeepTENNet: the nets of texture_pooling.py:468-526)
"""
from .functional import (NfpConfig, nfp_attention_pool, nfp_deepten_encode, nfp_compress_map, nfp_compress_map_tensors, nfp_compress_pool,
                         nfp_compress_pool_tensors, nfp_multi_radius, nfp_pool, nfp_pooled, nfp_strided, nfp_valid,
                         nfp_with_gap)
from .functional import nfp as nfp_op  # (`nfp` itself is the submodule holding NFPPooling)
from .nfp import (EnhancedNFPPooling, MultiRadiusNFPPooling, NFPBottleneck, NFPInsert, NFPPooling, NFPWithGap,
                  SimilarityAwarePooling)
from .pooling import nfp_pooling
from .deepten import DeepTENEncoding
from .heads import AdaptiveFusionNFP, MultiRadiusNFPHead, NFPHead
from . import _ops  # registers torch.ops.nfp_amd.* (torch.compile support)

__all__ = ["NFPPooling", "EnhancedNFPPooling", "MultiRadiusNFPPooling", "nfp_pooling", "nfp_op", "nfp_pool", "nfp_pooled",
           "nfp_multi_radius", "NfpConfig", "nfp_with_gap", "NFPWithGap", "SimilarityAwarePooling", "nfp_attention_pool",
           "NFPBottleneck", "nfp_valid", "NFPHead", "MultiRadiusNFPHead", "AdaptiveFusionNFP", "nfp_compress_pool",
           "nfp_compress_pool_tensors", "NFPInsert", "nfp_compress_map", "nfp_compress_map_tensors", "nfp_strided",
           "DeepTENEncoding", "nfp_deepten_encode"]
__version__ = "0.4.0"
