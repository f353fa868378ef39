"""NFPPooling — drop-in for models/pooling/nfp.py::NFPPooling (nfp.py:15-375).

Same constructor, same forward contract ([B,C,H,W] -> [B, k*k-1, H', W']), same
public attributes, same error on an unknown measure; the work is done by the
fused gfx950 kernels behind include/nfp.h instead of two frozen depthwise convs
and a chain of ATen ops.  With bias=False (the default) the module has no
trainable parameters (as in the reference, whose two conv weights are frozen:
nfp.py:61,82); with bias=True the two convs' biases are trainable parameters
under the reference's names, comp_neighbors.bias [C*N] and center_value.bias [C].
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _abi
from .functional import (NfpConfig, gap_servable, multi_radius_config, nfp, nfp_attention_pool, nfp_biased,
                         nfp_compress_map, nfp_multi_radius, nfp_strided, nfp_valid, nfp_with_gap)

_DISPATCH = set(_abi.MEASURES) | set(_abi.MEASURE_ALIASES)


class _ConvBias(nn.Module):
    """comp_neighbors / center_value of the reference with bias=True: only the trainable bias is a parameter here (the
    frozen one-hot weight is a constant of (C, R, measure), emitted into the state dict by NFPPooling)."""

    def __init__(self, bias):
        super().__init__()
        self.bias = nn.Parameter(bias)


class NFPPooling(nn.Module):
    def __init__(self, in_channels, R=1, measure='norm', p=1, stride=1, padding=0,
                 dilation=1, bias=False, padding_mode='reflect', similarity=True,
                 eps=1e-6, input_size=224, q_scs=1e-6):
        super().__init__()
        if padding_mode not in _abi.PAD_MODES:
            raise ValueError(f"padding_mode must be one of {_abi.PAD_MODES}, got {padding_mode!r}")
        self.in_size = input_size
        self.measure = measure.lower()          # nfp.py:21
        self.in_channels = in_channels
        self.R = R
        self.stride = stride
        self.padding = padding
        self.padding_mode = padding_mode
        self.similarity = similarity
        self.p = p
        self.dilation = dilation
        self.bias = bias
        self.eps = eps
        self.q_scs = q_scs
        self.kernel_size = int(2 * self.R + 1)          # nfp.py:38
        self.out_channels = int(self.kernel_size ** 2 - 1)  # nfp.py:39
        # nfp.py:74 tests the RAW string, nfp.py:85 the lower-cased one: 'Norm' yields |neighbour|.
        self._diff_weights = measure in ('norm', 'rmse', 'mahalanobis')
        if bias:
            # nfp.py:42-58 with bias=True: both depthwise convs get TRAINABLE biases (only the weights are frozen,
            # nfp.py:61,82).  The two convs are built as the reference builds them, so that nn.Conv2d.reset_parameters
            # draws from the RNG in the reference's order (comp_neighbors weight, its bias, center_value weight, its
            # bias): the same seed gives bit-identical biases.
            k, C = self.kernel_size, int(in_channels)
            comp = nn.Conv2d(C, self.out_channels * C, k, groups=C, bias=True)
            centre = nn.Conv2d(C, C, k, groups=C, bias=True)
            self.comp_neighbors = _ConvBias(comp.bias.data.clone())
            self.center_value = _ConvBias(centre.bias.data.clone())
        if self.measure not in _DISPATCH:
            raise RuntimeError(f'Similarity measure {self.measure} not implemented')  # nfp.py:120

    # -- the op ------------------------------------------------------------------------------
    @property
    def config(self):
        """Frozen view of the op-defining attributes (they are plain, assignable attributes as in the
        reference, so the view is rebuilt only when one of them changed)."""
        sig = (self.R, self.measure, self.p, self.stride, self.padding, self.dilation, self.padding_mode,
               self.similarity, self.eps, self.q_scs, self._diff_weights)
        cached = self.__dict__.get("_cfg_cache")
        if cached is not None and cached[0] == sig:
            return cached[1]
        cfg = self._build_config()
        if not torch.compiler.is_compiling():      # (no attribute mutation inside a traced forward)
            self.__dict__["_cfg_cache"] = (sig, cfg)
        return cfg

    def _build_config(self):
        return NfpConfig(R=int(self.R), measure=_abi.MEASURE_ALIASES.get(self.measure, self.measure),
                         p=self.p, stride=int(self.stride), padding=int(self.padding),
                         dilation=int(self.dilation), padding_mode=self.padding_mode,
                         similarity=bool(self.similarity), eps=float(self.eps), q_scs=float(self.q_scs),
                         diff_weights=self._diff_weights)

    def forward(self, x):
        if x.dim() == 4 and x.shape[1] != self.in_channels:
            raise RuntimeError(f"NFPPooling expected input with {self.in_channels} channels, "
                               f"got {x.shape[1]} channels instead")
        if self.bias:
            return nfp_biased(x, self.config, self.center_value.bias, self.comp_neighbors.bias)
        return nfp(x, self.config)

    @property
    def output_size(self):
        """nfp.py:125-130 (square-only helper based on input_size)."""
        return (self.in_size + 2 * self.padding - self.dilation * (self.kernel_size - 1) - 1) // self.stride + 1

    def extra_repr(self):
        return (f"in_channels={self.in_channels}, R={self.R}, measure={self.measure!r}, p={self.p}, "
                f"stride={self.stride}, padding={self.padding}, dilation={self.dilation}, "
                f"padding_mode={self.padding_mode!r}, similarity={self.similarity}" + (", bias=True" if self.bias else ""))

    # -- checkpoint compatibility ------------------------------------------------------------
    # A reference NFPPooling state-dict holds its two frozen conv weights,
    # comp_neighbors.weight [C*N,1,k,k] and center_value.weight [C,1,k,k] (nfp.py:42-82).
    # They are constants of (C, R, measure); emit them so reference code can load our
    # checkpoints, and accept (ignore) them when loading reference checkpoints.
    def _frozen_weights(self):
        C, k, N, R = int(self.in_channels), self.kernel_size, self.out_channels, int(self.R)
        centre = torch.zeros(C, 1, k, k)
        centre[:, :, R, R] = 1
        comp = torch.zeros(C * N, 1, k, k)
        taps = [t for t in range(k * k) if t != (k * k) // 2]
        ky = torch.tensor([t // k for t in taps]).repeat(C)
        kx = torch.tensor([t % k for t in taps]).repeat(C)
        rows = torch.arange(C * N)
        if self._diff_weights:
            comp[:, :, R, R] = 1
            comp[rows, 0, ky, kx] = -1
        else:
            comp[rows, 0, ky, kx] = 1
        return comp, centre

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        comp, centre = self._frozen_weights()
        destination[prefix + 'comp_neighbors.weight'] = comp
        destination[prefix + 'center_value.weight'] = centre

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys,
                              unexpected_keys, error_msgs):
        for key in ('comp_neighbors.weight', 'center_value.weight'):
            state_dict.pop(prefix + key, None)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys,
                                      unexpected_keys, error_msgs)


class EnhancedNFPPooling(NFPPooling):
    """Constructible stand-in for models.pooling.enhanced_nfp.EnhancedNFPPooling, which
    models/nfp_heads.py:6 and models/vittiny_models_new.py:7 import but the reference does
    not ship.  Call sites pass (in_channels=, R=, measure=, padding=[, **kw]) — see
    nfp_heads.py:18-23,58-63,88-93,208-214 — which NFPPooling accepts; unknown extra
    keyword arguments are ignored.  Parity for this class is unpinned (no reference code)."""

    def __init__(self, in_channels, R=1, measure='cosine', padding=0, **kw):
        known = {k: kw[k] for k in ('p', 'stride', 'dilation', 'bias', 'padding_mode', 'similarity',
                                    'eps', 'input_size', 'q_scs') if k in kw}
        super().__init__(in_channels, R=R, measure=measure, padding=padding, **known)


class MultiRadiusNFPPooling(nn.Module):
    """The NFP part of models/nfp_heads.py::MultiRadiusNFPHead (nfp_heads.py:80-118): one EnhancedNFPPooling per radius
    on the SAME feature map, concatenated along the channel axis (nfp_heads.py:88-93, 109-110).  `nfp_blocks` holds the
    per-radius layers exactly as the reference's ModuleList does (so state dicts line up); forward() returns
    torch.cat([blk(x) for blk in nfp_blocks], dim=1) — for R_list = (1, 2) on the GPU from one fused pass over x."""

    def __init__(self, in_channels, R_list=(1, 2), measure="cosine", **kw):
        super().__init__()
        self.nfp_blocks = nn.ModuleList([EnhancedNFPPooling(in_channels=in_channels, R=R, measure=measure, padding=R, **kw)
                                         for R in R_list])
        self.in_channels = in_channels
        self.out_channels = sum(b.out_channels for b in self.nfp_blocks)

    def forward(self, x):
        blocks = list(self.nfp_blocks)
        if len(blocks) == 2 and all(isinstance(b, NFPPooling) and not b.bias for b in blocks):   # (no fused form with biases)
            if x.dim() == 4 and x.shape[1] != self.in_channels:
                raise RuntimeError(f"MultiRadiusNFPPooling expected input with {self.in_channels} channels, "
                                   f"got {x.shape[1]} channels instead")
            return nfp_multi_radius(x, blocks[0].config, blocks[1].config)
        return torch.cat([b(x) for b in blocks], dim=1)


class NFPWithGap(nn.Module):
    """(GAP(x) [B,C] float32, NFP(x) [B,N,H',W']) of one feature map — how every head of models/nfp_heads.py starts
    (`gap(fmap)` and `nfp(fmap)`, nfp_heads.py:39-42).  Wraps any NFPPooling / EnhancedNFPPooling, or a
    MultiRadiusNFPPooling (MultiRadiusNFPHead, nfp_heads.py:80-118: the 8 + 24 maps of radii 1 and 2), which stays
    reachable (and keeps its state-dict entries) as `.nfp`.  On the GPU both come from one pass over x and one backward
    kernel takes the gradients of both (functional.nfp_with_gap); a bias=True layer, and a multi-radius layer other than
    two unbiased blocks that `nfp_multi_radius` would fuse, has no fused form: its own forward, then the mean."""

    def __init__(self, nfp_layer):
        super().__init__()
        if not isinstance(nfp_layer, (NFPPooling, MultiRadiusNFPPooling)):
            raise TypeError("NFPWithGap wraps an NFPPooling / EnhancedNFPPooling / MultiRadiusNFPPooling layer, "
                            f"got {type(nfp_layer).__name__}")
        self.nfp = nfp_layer

    @property
    def out_channels(self):
        return self.nfp.out_channels

    def _fused_pair_config(self):
        """The inner_R = 1 configuration of a MultiRadiusNFPPooling whose two blocks `nfp_multi_radius` would fuse, else None."""
        blocks = list(self.nfp.nfp_blocks)
        if len(blocks) != 2 or not all(isinstance(b, NFPPooling) and not b.bias for b in blocks):
            return None
        return multi_radius_config(blocks[0].config, blocks[1].config)

    def forward(self, x):
        layer = self.nfp
        if isinstance(layer, MultiRadiusNFPPooling):
            cfg = self._fused_pair_config()
            if cfg is not None and x.dim() == 4 and x.shape[1] != layer.in_channels:
                raise RuntimeError(f"MultiRadiusNFPPooling expected input with {layer.in_channels} channels, "
                                   f"got {x.shape[1]} channels instead")
            # (a CUDA call the gap kernels refuse — a map above 512 pixels, Norm p = 1 — is the layer's own forward, which
            # knows its own fallbacks, not nfp(x, cfg) with both radii in one descriptor)
            if cfg is not None and (not x.is_cuda or gap_servable(x, cfg)):
                return nfp_with_gap(x, cfg)
            return x.mean((2, 3)).float(), layer(x)
        if layer.bias:
            return x.mean((2, 3)).float(), layer(x)
        if x.dim() == 4 and x.shape[1] != layer.in_channels:
            raise RuntimeError(f"NFPPooling expected input with {layer.in_channels} channels, "
                               f"got {x.shape[1]} channels instead")
        return nfp_with_gap(x, layer.config)


class SimilarityAwarePooling(nn.Module):
    """Drop-in for models/nfp_heads.py::SimilarityAwarePooling (nfp_heads.py:204-232): the NFP maps of an unpadded layer,
    a trainable 1x1 conv `att_proj` over them, a softmax over the pixels, and the maps summed under that attention —
    [B,C,H,W] -> [B,N].  Same constructor, attributes and state-dict keys (nfp.comp_neighbors.weight,
    nfp.center_value.weight, att_proj.weight, att_proj.bias, the nfp.* biases with bias=True); the 7x7 CPU probe is drawn
    before att_proj is built, as in the reference, so the same seed gives bit-identical att_proj parameters.  On the GPU
    the tail behind the layer is one HIP kernel each way (functional.nfp_attention_pool)."""

    def __init__(self, in_channels=512, R=1, measure='cosine', **kwargs):
        super().__init__()
        # (`padding` in kwargs: TypeError, a keyword given twice — as in the reference, nfp_heads.py:208-214)
        self.nfp = EnhancedNFPPooling(in_channels=in_channels, R=R, measure=measure, padding=0, **kwargs)
        if not self.nfp.bias:
            # The reference's layer draws the weights of its two depthwise convs before it overwrites them (nfp.py:42-59);
            # NFPPooling(bias=False) here draws nothing, so the same draws are made — and dropped — at this point: the probe
            # and att_proj then see the RNG where the reference's do.  (bias=True: the layer has built both convs itself.)
            C, k = int(in_channels), self.nfp.kernel_size
            nn.Conv2d(C, self.nfp.out_channels * C, k, groups=C, bias=False)
            nn.Conv2d(C, C, k, groups=C, bias=False)
        with torch.no_grad():                                   # nfp_heads.py:216-219
            nfp_out = self.nfp(torch.randn(1, in_channels, 7, 7))
        nfp_channels = nfp_out.shape[1]
        self.att_proj = nn.Conv2d(nfp_channels, 1, kernel_size=1)
        self.softmax = nn.Softmax(dim=-1)
        self.nfp_channels = nfp_channels

    def forward(self, x):
        return nfp_attention_pool(self.nfp(x), self.att_proj.weight, self.att_proj.bias)


def _module_memory_format(memory_format, x):
    """The memory_format a block hands nfp_compress_map for input x: torch.preserve_format follows x — channels-last exactly
    when x is dense in that layout and not also NCHW-dense (H = W = 1 or one channel: both) —, the other two stand."""
    if memory_format != torch.preserve_format:
        return memory_format
    follows = x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()
    return torch.channels_last if follows else torch.contiguous_format


_MODULE_FORMATS = (torch.contiguous_format, torch.channels_last, torch.preserve_format)


class NFPBottleneck(nn.Module):
    """Drop-in for models/nfp_heads.py::NFPBottleneck (nfp_heads.py:234-278, the second definition — the one Python keeps):
    a residual block with an unpadded cosine NFP layer between two 1x1 convs,
        relu(bn1(conv1(x))) -> NFP(R=1, cosine, padding=0) -> bn2(conv2(.)) + downsample(_match(x)) -> relu
    [B, in, H, W] -> [B, out, H'-2, W'-2] (H' = H behind conv1's stride).  Same constructor, attributes and state-dict keys
    (conv1 / bn1 / nfp.* / conv2 / bn2 / downsample.*); the RNG is consumed in the reference's order — conv1, bn1, the
    layer's two depthwise conv weights (drawn and dropped: NFPPooling(bias=False) holds no conv), the 5x5 probe, conv2,
    bn2, downsample — so the same seed gives bit-identical parameters.  On the GPU the layer runs the valid-map kernels
    (functional.nfp_valid), forward and backward one launch each.
    fused_project=True (not in the reference; the default keeps the two ATen ops): bn2(conv2(.)) as one call of
    functional.nfp_compress_map(relu=False) — on the GPU, where it serves, without the copies of the [B,out,H,W]
    activation that conv2 and bn2 write, re-read and save.
    memory_format (with fused_project=True only; anything but the default without it is a ValueError): the layout the
    projection writes, and so the block returns — torch.channels_last for a channels-last network, where `out += identity`
    then adds like to like; torch.preserve_format: channels-last exactly when x is (dense in it and not also NCHW-dense)."""
    expansion = 1

    def __init__(self, in_channels: int, out_channels: int, stride=1, *, fused_project=False,
                 memory_format=torch.contiguous_format):
        super().__init__()
        self.fused_project = bool(fused_project)
        if memory_format not in _MODULE_FORMATS:
            raise ValueError(f"NFPBottleneck: memory_format must be torch.contiguous_format, torch.channels_last or "
                             f"torch.preserve_format, got {memory_format!r}")
        if memory_format != torch.contiguous_format and not self.fused_project:
            raise ValueError("NFPBottleneck: memory_format applies to the fused projection; pass fused_project=True")
        self.memory_format = memory_format
        mid = out_channels // 4
        self.conv1 = nn.Conv2d(in_channels, mid, 1, bias=False, stride=stride)
        self.bn1 = nn.BatchNorm2d(mid)
        self.nfp = EnhancedNFPPooling(mid, R=1, measure="cosine", padding=0)
        # (the draws of the reference layer's two depthwise convs, nfp.py:42-59 — as SimilarityAwarePooling.__init__)
        nn.Conv2d(mid, self.nfp.out_channels * mid, self.nfp.kernel_size, groups=mid, bias=False)
        nn.Conv2d(mid, mid, self.nfp.kernel_size, groups=mid, bias=False)
        with torch.no_grad():                                   # nfp_heads.py:245-246
            mid2 = self.nfp(torch.randn(1, mid, 5, 5)).shape[1]
        self.conv2 = nn.Conv2d(mid2, out_channels, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(out_channels)
        self.relu = nn.ReLU(inplace=True)
        if in_channels != out_channels:
            self.downsample = nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=1, bias=False),
                                            nn.BatchNorm2d(out_channels))
        else:
            self.downsample = nn.Identity()

    def _match(self, ident, target_hw):
        # sized from the LAST dimension alone (nfp_heads.py:261-265): a non-square map behind stride 2 fails here as there
        if ident.shape[-1] == target_hw:
            return ident
        k = ident.shape[-1] - target_hw + 1
        return F.avg_pool2d(ident, kernel_size=k, stride=1, padding=0)

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = nfp_valid(out, self.nfp.config)
        if self.fused_project:
            out = nfp_compress_map(out, self.conv2.weight, self.bn2, relu=False,
                                   memory_format=_module_memory_format(self.memory_format, x))
        else:
            out = self.bn2(self.conv2(out))
        identity = self._match(identity, out.shape[-1])
        identity = self.downsample(identity)
        out += identity
        return self.relu(out)


class NFPInsert(nn.Module):
    """The block models/mobilenetv3.py::MOBILENETV3_NFP_INSERT puts behind one stage of its trunk (mobilenetv3.py:345-353):
        nfp = NFPPooling(in_channels, **nfp_kwargs)      nfp_proj = Conv2d(nfp.out_channels, C, 1, bias=False) -> BN -> ReLU
        x -> nfp_proj(nfp(x))                            [B, in, H, W] -> [B, C, H', W']
    C = out_channels (None: in_channels, as in the reference, where the result replaces the stage's feature map).  The
    layer's keywords default to the class defaults, as there: Norm p = 1, padding 0, reflect — the map shrinks by 2R.
    `nfp_proj` is the reference's nn.Sequential as parameter holder, with its state-dict keys (nfp_proj.0.weight,
    nfp_proj.1.*); the RNG is consumed in the reference's order — the layer's two depthwise conv weights (drawn and
    dropped), then the conv — so the same seed gives bit-identical parameters.  forward is one call of
    functional.nfp_compress_map behind the layer: on the GPU, where it serves, the projected map is stored once and nothing
    of its size is saved for the backward.
    memory_format (keyword only): the layout of the result — torch.contiguous_format, torch.channels_last, or
    torch.preserve_format: channels-last exactly when x is (dense in it and not also NCHW-dense).
    valid_layer (keyword only, default False: `self.nfp(x)` as before): an unbiased layer with padding 0, stride 1 and
    dilation 1 — the class defaults — runs as functional.nfp_valid(x, self.nfp.config): on the GPU the valid-map kernels, one
    launch each way (for the default Norm p = 1 their L1 family, which saves x alone), where they serve; every other layer
    keeps `self.nfp(x)`.  Parameters, state dict, RNG order and CPU results do not depend on it.
    strided_layer (keyword only, default False): likewise, an unbiased layer with stride >= 2 and dilation 1 runs as
    functional.nfp_strided(x, self.nfp.config) — on the GPU the strided row-band kernels where they serve."""

    def __init__(self, in_channels, out_channels=None, *, memory_format=torch.contiguous_format, valid_layer=False,
                 strided_layer=False, **nfp_kwargs):
        super().__init__()
        if memory_format not in _MODULE_FORMATS:
            raise ValueError(f"NFPInsert: memory_format must be torch.contiguous_format, torch.channels_last or "
                             f"torch.preserve_format, got {memory_format!r}")
        self.memory_format = memory_format
        self.valid_layer = bool(valid_layer)
        self.strided_layer = bool(strided_layer)
        from .heads import _reference_layer_draws
        out_channels = int(in_channels if out_channels is None else out_channels)
        self.nfp = NFPPooling(in_channels=in_channels, **nfp_kwargs)
        if not self.nfp.bias:       # (bias=True: the layer has built both convs itself)
            _reference_layer_draws(self.nfp)
        self.nfp_proj = nn.Sequential(nn.Conv2d(self.nfp.out_channels, out_channels, kernel_size=1, bias=False),
                                      nn.BatchNorm2d(out_channels), nn.ReLU(inplace=True))
        self.in_channels, self.out_channels = int(in_channels), out_channels

    def _layer(self, x):
        cfg = self.nfp.config
        if (self.valid_layer and not self.nfp.bias and cfg.padding == 0 and cfg.stride == 1 and cfg.dilation == 1
                and x.dim() == 4 and x.shape[1] == self.nfp.in_channels):
            return nfp_valid(x, cfg)
        if (self.strided_layer and not self.nfp.bias and cfg.stride >= 2 and cfg.dilation == 1
                and x.dim() == 4 and x.shape[1] == self.nfp.in_channels):
            return nfp_strided(x, cfg)
        return self.nfp(x)      # (and the layer's own complaint about any other input)

    def forward(self, x):
        return nfp_compress_map(self._layer(x), self.nfp_proj[0].weight, self.nfp_proj[1],
                                memory_format=_module_memory_format(self.memory_format, x))
