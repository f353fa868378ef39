"""The leading (preloaded) kernel arguments of fwd_band / bwd_fast — csrc/nfp_common.h: the HEAD — on the GPU.

The two table kernels take what stands in front of their first memory request (pointers, batch stride, C, P / H / W / R,
rows per band, chunk size, channel groups, workgroup size) as individual leading arguments, several of them packed into one
dword, and everything else through the trailing parameter block.  A wrong, swapped or truncated head field shows as a
wrong result at the shapes below, the smallest at which each field matters: several bands per image with P % 4 != 0, the
smallest map, H != W, a batch stride that is not C * P, channels-last, bf16 (the matrix-core backward), more than one
channel chunk (Cc < C), k = 5, both radii from one pass, the fused pooling tail, and the padding modes (the backward's
table layout depends on the mode, which rides in the head).

Referee and tolerances: those of tests/test_gpu_parity.py — the CPU oracle on the same inputs; float32 at TOL, bf16
storage at 1e-2 (maps) / 2e-2 (gradients) against the oracle on the bf16-rounded inputs.  Every case runs forward and
backward and checks that the table kernels served it (nfp_last_variant)."""
import numpy as np
import pytest
import torch

from conftest import nfp_switch, rel_err
from neighbour_feature_pooling_amd import MultiRadiusNFPPooling, NFPPooling, NFPWithGap, _abi, nfp_pooled
from neighbour_feature_pooling_amd.synth import feature_map
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

COS = dict(R=1, measure="cosine", padding=1)
_REF = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _abi.load()
    return torch.device("cuda:0")


def _bf16_round(a):
    return torch.tensor(a).bfloat16().float().numpy()


def _reference(oracle, shape, ctor, bf=False, seed=31):
    """(x, grad_out, ref out, ref grad_x): computed once per (shape, ctor, dtype), shared, read-only."""
    key = (shape, tuple(sorted(ctor.items())), bf, seed)
    if key not in _REF:
        x = feature_map(shape, seed)
        N = (2 * ctor["R"] + 1) ** 2 - 1
        go = feature_map((shape[0], N, shape[2], shape[3]), seed + 1)
        if bf:
            x, go = _bf16_round(x), _bf16_round(go)
        _REF[key] = (x, go, oracle.forward(x, **ctor), oracle.backward(x, go, **ctor))
        for a in _REF[key]:
            a.setflags(write=False)
    return _REF[key]


def _run(x, go, ctor):
    """Forward + backward of NFPPooling on `x` (a leaf that requires grad); returns (out, grad_x, fwd variant, bwd variant)."""
    L = _abi.load()
    m = NFPPooling(x.shape[1], **ctor)
    n0 = L.nfp_launch_count()
    out = m(x)
    fv = L.nfp_last_variant().decode()
    out.backward(go)
    torch.cuda.synchronize()
    bv = L.nfp_last_variant().decode()
    assert L.nfp_launch_count() == n0 + 2, (fv, bv)
    return out.detach().float().cpu().numpy(), x.grad.float().cpu().numpy(), fv, bv


def _check(name, out, gx, ref_out, ref_gx, fv, bv, bf=False, fwd="fwd_band<"):
    e_out, e_gx = rel_err(out, ref_out), rel_err(gx, ref_gx)
    print(f"{name}: out {e_out:.2e} grad_x {e_gx:.2e} [{fv} | {bv}]")
    assert fv.startswith(fwd) and bv.startswith("bwd_fast<"), (fv, bv)
    assert e_out <= (1e-2 if bf else TOL), e_out
    assert e_gx <= (2e-2 if bf else TOL), e_gx


#          name             shape            ctor
PLAIN = [("many_bands",    (3, 16, 7, 7),   COS),                                            # P % 4 != 0, 7 bands per image
         ("smallest_map",  (2, 8, 2, 2),    COS),                                            # P = 4
         ("non_square",    (5, 12, 5, 6),   COS),                                            # H != W
         ("several_chunks", (2, 4096, 7, 7), COS),                                           # Cc < C
         ("k5_l2",         (2, 8, 6, 6),    dict(R=2, measure="norm", p=2, padding=2)),      # k = 5
         ("pad_zeros",     (3, 16, 7, 7),   dict(COS, padding_mode="zeros")),
         ("pad_replicate", (3, 16, 7, 7),   dict(COS, padding_mode="replicate"))]


@pytest.mark.parametrize("name,shape,ctor", PLAIN, ids=[c[0] for c in PLAIN])
def test_dense_f32_nchw(name, shape, ctor, dev, oracle_lib):
    xh, goh, ref_out, ref_gx = _reference(oracle_lib, shape, ctor)
    x = torch.tensor(xh).to(dev).requires_grad_(True)
    out, gx, fv, bv = _run(x, torch.tensor(goh).to(dev), ctor)
    if name == "many_bands":
        assert fv.endswith("x7"), fv
    _check(name, out, gx, ref_out, ref_gx, fv, bv)


def test_batch_strided_view(dev, oracle_lib):
    """x = big[:, :16] of a [3,32,7,7] tensor: batch stride 32 * 49, not C * P; grad_x is dense (its own batch stride)."""
    shape = (3, 16, 7, 7)
    xh, goh, ref_out, ref_gx = _reference(oracle_lib, shape, COS)
    big = torch.tensor(feature_map((3, 32, 7, 7), 77)).to(dev)
    big[:, :16] = torch.tensor(xh).to(dev)
    x = big[:, :16].detach().requires_grad_(True)
    assert x.stride(0) == 32 * 49 and not x.is_contiguous()
    out, gx, fv, bv = _run(x, torch.tensor(goh).to(dev), COS)
    assert x.grad.shape == x.shape
    _check("strided_view", out, gx, ref_out, ref_gx, fv, bv)


def test_channels_last_f32(dev, oracle_lib):
    shape = (3, 16, 7, 7)
    xh, goh, ref_out, ref_gx = _reference(oracle_lib, shape, COS)
    x = torch.tensor(xh).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out, gx, fv, bv = _run(x, torch.tensor(goh).to(dev), COS)
    assert ",nhwc" in fv and ",nhwc" in bv, (fv, bv)
    _check("channels_last_f32", out, gx, ref_out, ref_gx, fv, bv)


@pytest.mark.parametrize("cores", ["matrix", "vector"])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_bf16(layout, cores, dev, oracle_lib, monkeypatch):
    """bf16 storage.  'matrix': the dispatcher's choice — the matrix-core kernels where they apply (a bwd_fast<...,mfma>
    backward; the forward is then fwd_gram, which keeps its signature); 'vector' (NFP_MFMA=0): fwd_band / the vector
    bwd_fast in bf16."""
    nfp_switch(monkeypatch, "NFP_MFMA", "1" if cores == "matrix" else "0")
    shape = (2, 32, 7, 7)
    xh, goh, ref_out, ref_gx = _reference(oracle_lib, shape, COS, bf=True)
    x = torch.tensor(xh).to(dev, torch.bfloat16)
    if layout == "nhwc":
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    out, gx, fv, bv = _run(x, torch.tensor(goh).to(dev, torch.bfloat16), COS)
    assert ",bf16," in fv and ",bf16," in bv and f",{layout}" in fv and f",{layout}" in bv, (fv, bv)
    if cores == "matrix":
        assert ("mfma" in bv) == (layout == "nhwc"), bv   # (NCHW rows of 49 pixels are not 8-byte aligned: the vector backward)
    _check(f"bf16_{layout}_{cores}", out, gx, ref_out, ref_gx, fv, bv, bf=True,
           fwd="fwd_gram<" if cores == "matrix" else "fwd_band<")


def test_radii_1_and_2_with_gap(dev, oracle_lib):
    shape, mode = (2, 16, 7, 7), "reflect"
    c1 = dict(R=1, measure="cosine", padding=1, padding_mode=mode)
    c2 = dict(c1, R=2, padding=2)
    xh = feature_map(shape, 41)
    ggh, goh = feature_map(shape[:2], 42), feature_map((2, 32, 7, 7), 43)
    ref = np.concatenate([oracle_lib.forward(xh, **c1), oracle_lib.forward(xh, **c2)], axis=1)
    ref_gx = oracle_lib.backward(xh, goh[:, :8].copy(), **c1).astype(np.float64) + \
        oracle_lib.backward(xh, goh[:, 8:].copy(), **c2) + ggh.astype(np.float64)[:, :, None, None] / 49
    L = _abi.load()
    x = torch.tensor(xh).to(dev).requires_grad_(True)
    head = NFPWithGap(MultiRadiusNFPPooling(16, R_list=(1, 2), measure="cosine", padding_mode=mode))
    gap, maps = head(x)
    fv = L.nfp_last_variant().decode()
    ((gap * torch.tensor(ggh).to(dev)).sum() + (maps * torch.tensor(goh).to(dev)).sum()).backward()
    torch.cuda.synchronize()
    bv = L.nfp_last_variant().decode()
    assert fv.startswith("fwd_band<R1+2,") and bv.startswith("bwd_fast<R1+2,"), (fv, bv)
    e_gap = rel_err(gap.detach().cpu().numpy(), xh.astype(np.float64).mean((2, 3)))
    print(f"gap {e_gap:.2e}")
    assert e_gap <= TOL
    _check("radii_1_2", maps.detach().cpu().numpy(), x.grad.cpu().numpy(), ref, ref_gx, fv, bv)


def test_pooled(dev, oracle_lib):
    """nfp_pooled: the fused pooling tail — GAP of the maps; its backward's grad_out is grad[b,n] / P on every pixel."""
    shape = (2, 16, 7, 7)
    xh, _, ref_out, _ = _reference(oracle_lib, shape, COS)
    wh = feature_map((2, 8), 52)
    go_full = np.ascontiguousarray(np.broadcast_to(wh[:, :, None, None] / np.float32(49), (2, 8, 7, 7))).astype(np.float32)
    ref_gx = oracle_lib.backward(xh, go_full, **COS)
    L = _abi.load()
    x = torch.tensor(xh).to(dev).requires_grad_(True)
    nfpm = nfp_pooled(x, NFPPooling(16, **COS).config)
    fv = L.nfp_last_variant().decode()
    (nfpm * torch.tensor(wh).to(dev)).sum().backward()
    torch.cuda.synchronize()
    bv = L.nfp_last_variant().decode()
    assert tuple(nfpm.shape) == (2, 8) and nfpm.dtype == torch.float32
    _check("pooled", nfpm.detach().cpu().numpy(), x.grad.cpu().numpy(), ref_out.astype(np.float64).mean((2, 3)), ref_gx, fv, bv)
