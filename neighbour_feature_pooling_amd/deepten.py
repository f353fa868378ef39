"""The encoding layer of the Deep-TEN baseline (models/deepten.py::DeepTENEncoding; Zhang et al., CVPR 2017) — the layer the
reference's NFP numbers are compared against — as a drop-in module over `functional.nfp_deepten_encode`.

The reference forms the residual tensor pixel - codeword, [B,N,K,D], twice in its forward and keeps it for autograd (205 MB
each at [64,512,7,7] with 32 codewords).  On the GPU the HIP kernels of csrc/nfp_deepten.hip never form it.
"""
import torch
import torch.nn as nn

from .functional import nfp_deepten_encode


class DeepTENEncoding(nn.Module):
    """DeepTENEncoding(in_channels, num_codes): x [B,D,H,W] -> [B, K*D].  Attributes D, K, codewords [K,D], scale [K]; the
    reference's state-dict keys and its order of random draws, so the same seed gives the same parameters bit for bit."""

    def __init__(self, in_channels, num_codes):
        super().__init__()
        self.D = in_channels
        self.K = num_codes
        self.codewords = nn.Parameter(torch.randn(self.K, self.D))
        self.scale = nn.Parameter(torch.randn(self.K))
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / (self.K * self.D) ** 0.5
        with torch.no_grad():
            self.codewords.uniform_(-bound, bound)
            self.scale.uniform_(-1, 0)

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != self.D:
            raise RuntimeError(f"DeepTENEncoding({self.D}, {self.K}) expects [B,{self.D},H,W], got {tuple(x.shape)}")
        return nfp_deepten_encode(x, self.codewords, self.scale)

    def extra_repr(self):
        return f"in_channels={self.D}, num_codes={self.K}"
