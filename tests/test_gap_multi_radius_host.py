"""nfp_with_gap for radii (1, 2) together (MultiRadiusNFPHead: GAP(fmap) beside the 8 + 24 maps of one pass) and the C++
node of the pair, without a GPU: the library's host-only dry run on inner_R = 1 descriptors, the entry points' refusals,
the ABI, trace-time routing, the CPU composition and the head network."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from neighbour_feature_pooling_amd import MultiRadiusNFPPooling, NFPPooling, NFPWithGap, _abi
from neighbour_feature_pooling_amd.build import build_hip, build_torch_ext
from neighbour_feature_pooling_amd.functional import NfpConfig, _canon, build_desc, gap_servable_static

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build_hip()
    return _abi.load()


def cfg12(measure="cosine", **kw):
    return NfpConfig(R=2, padding=2, inner_R=1, measure=measure, diff_weights=measure in ("norm", "rmse"), **kw)


def desc12(lib, shape, measure="cosine", dtype=torch.float32, layout="nchw", ws=True, **kw):
    """An inner_R = 1 descriptor through functional.build_desc; ws: the workspace it is entitled to, stood in for."""
    d = build_desc(shape, _canon(shape, layout), dtype, cfg12(measure, **kw))
    if ws and lib.nfp_workspace_bytes(ctypes.byref(d)) > 0:
        d.ws = 0x1000
    return d


SERVED = [dict(shape=(64, 512, 7, 7)), dict(shape=(4, 192, 14, 14), measure="norm", p=2),
          dict(shape=(64, 512, 7, 7), dtype=torch.bfloat16, layout="nhwc"),
          dict(shape=(4, 192, 14, 14), measure="norm", p=2, dtype=torch.bfloat16, layout="nhwc"),
          dict(shape=(4, 64, 7, 7), measure="dot"), dict(shape=(4, 64, 7, 7), measure="gfc"),
          dict(shape=(4, 64, 7, 7), measure="rmse"), dict(shape=(300, 8, 5, 5)), dict(shape=(2, 16, 3, 3))]
REFUSED = [dict(shape=(64, 512, 7, 7), ws=False), dict(shape=(4, 64, 7, 7), measure="canberra"),
           dict(shape=(4, 64, 7, 7), measure="norm", p=1), dict(shape=(4, 64, 7, 7), measure="emd"),
           dict(shape=(4, 6, 7, 7)), dict(shape=(2, 8, 24, 24))]


def test_gap_supported_on_two_radius_descriptors(lib):
    for kw in SERVED:
        d = desc12(lib, **kw)
        assert d.ws, kw
        assert lib.nfp_gap_supported(ctypes.byref(d)) == 1, (kw, lib.nfp_last_error())
        assert lib.nfp_pool_supported(ctypes.byref(d)) == 0, kw
    for kw in REFUSED:
        d = desc12(lib, **kw)
        assert lib.nfp_gap_supported(ctypes.byref(d)) == 0, kw
        assert lib.nfp_pool_supported(ctypes.byref(d)) == 0, kw
    # the head's call shape, whatever the batch
    for B in (1, 32, 256, 1024):
        assert lib.nfp_gap_supported(ctypes.byref(desc12(lib, (B, 512, 7, 7)))) == 1, B


def test_saved_floats_and_the_dry_run_touches_nothing(lib):
    before, n0 = lib.nfp_last_variant(), lib.nfp_launch_count()
    assert lib.nfp_gap_saved_floats(ctypes.byref(desc12(lib, (4, 64, 7, 7)))) == 4 * 49      # norms only, one band
    assert lib.nfp_gap_saved_floats(ctypes.byref(desc12(lib, (4, 64, 7, 7), measure="norm", p=2))) == 0
    assert lib.nfp_gap_supported(ctypes.byref(desc12(lib, (64, 512, 7, 7)))) == 1
    assert lib.nfp_launch_count() == n0 and lib.nfp_last_variant() == before


def test_entry_points_refuse_before_touching_anything(lib):
    fake = ctypes.c_void_p(0x1000)
    n0 = lib.nfp_launch_count()
    d = desc12(lib, (4, 64, 7, 7))
    need = lib.nfp_gap_saved_floats(ctypes.byref(d))
    assert need == 4 * 49
    assert lib.nfp_gap_forward(ctypes.byref(d), fake, fake, fake, fake, need - 1, None) == -1      # short `saved`
    assert b"saved holds" in lib.nfp_last_error()
    assert lib.nfp_gap_forward(ctypes.byref(d), fake, fake, fake, None, need, None) == -1
    assert lib.nfp_gap_backward(ctypes.byref(d), fake, None, fake, fake, fake, need - 1, fake, None) == -1
    assert b"saved holds" in lib.nfp_last_error()
    assert lib.nfp_gap_forward(ctypes.byref(d), fake, None, fake, fake, need, None) == -1          # null gap
    for kw in (dict(measure="canberra"), dict(measure="norm", p=1)):                               # unserved measures
        d = desc12(lib, (4, 64, 7, 7), **kw)
        assert lib.nfp_gap_forward(ctypes.byref(d), fake, fake, fake, fake, 1 << 20, None) == -2
        assert lib.nfp_gap_backward(ctypes.byref(d), fake, None, fake, fake, fake, 1 << 20, fake, None) == -2
    d = desc12(lib, (2, 8, 24, 24))                                                                # above 512 pixels
    assert lib.nfp_gap_forward(ctypes.byref(d), fake, fake, fake, fake, 1 << 20, None) == -2
    assert lib.nfp_gap_backward(ctypes.byref(d), fake, None, fake, fake, fake, 1 << 20, fake, None) == -2
    assert lib.nfp_launch_count() == n0


def test_abi_is_unchanged(lib):
    header = open(os.path.join(ROOT, "include", "nfp.h")).read()
    assert re.search(r"#define NFP_ABI_VERSION 7\b", header) and lib.nfp_abi_version() == 7 and _abi.ABI_VERSION == 7
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = re.findall(r"^\s*(?:const\s+)?(?:int|int64_t|uint64_t|void|char)\s*\*?\s*(nfp_\w+)\s*\(", code, flags=re.M)
    assert sorted(_abi.EXPORTS) == sorted(declared)


def test_trace_time_servability_takes_two_radii(lib):
    cos = cfg12()
    assert gap_servable_static((4, 64, 7, 7), (64 * 49, 49, 7, 1), torch.float32, cos)
    assert gap_servable_static((4, 64, 7, 7), (64 * 49, 1, 7 * 64, 64), torch.bfloat16, cos)
    assert not gap_servable_static((2, 8, 24, 24), (8 * 576, 576, 24, 1), torch.float32, cos)
    assert not gap_servable_static((4, 64, 7, 7), (64 * 49, 49, 7, 1), torch.float16, cos)
    assert not gap_servable_static((4, 64, 7, 7), (64 * 49, 49, 7, 1), torch.float32, cfg12("canberra"))


@pytest.mark.parametrize("kw", [dict(R_list=(1, 2), measure="cosine"), dict(R_list=(1, 2), measure="norm", p=2),
                                dict(R_list=(1, 2, 3), measure="cosine"), dict(R_list=(1, 2), measure="cosine", bias=True)])
def test_cpu_tensors_equal_the_composition_values_and_both_gradients(kw):
    torch.manual_seed(3)
    layer = MultiRadiusNFPPooling(6, **kw)
    head = NFPWithGap(layer)
    assert head.nfp is layer and head.out_channels == layer.out_channels == sum((2 * R + 1) ** 2 - 1 for R in kw["R_list"])
    assert any(k.startswith("nfp.nfp_blocks.0.") for k in head.state_dict())
    x = torch.randn(2, 6, 7, 8, requires_grad=True)
    gap, maps = head(x)
    assert gap.dtype == torch.float32 and tuple(gap.shape) == (2, 6) and maps.shape[1] == head.out_channels
    xr = x.detach().clone().requires_grad_(True)
    gap_r, maps_r = xr.mean((2, 3)).float(), layer(xr)
    assert torch.equal(gap, gap_r) and torch.equal(maps, maps_r)
    wg, wm = torch.randn_like(gap), torch.randn_like(maps)
    ((gap * wg).sum() + (maps * wm).sum()).backward()
    ((gap_r * wg).sum() + (maps_r * wm).sum()).backward()
    assert torch.allclose(x.grad, xr.grad, rtol=0, atol=1e-6)
    for use in ("gap", "maps"):         # each output alone
        x2 = x.detach().clone().requires_grad_(True)
        g2, m2 = head(x2)
        ((g2 * wg).sum() if use == "gap" else (m2 * wm).sum()).backward()
        x3 = x.detach().clone().requires_grad_(True)
        ((x3.mean((2, 3)) * wg).sum() if use == "gap" else (layer(x3) * wm).sum()).backward()
        assert torch.allclose(x2.grad, x3.grad, rtol=0, atol=1e-6)
    with torch.no_grad():
        g4, m4 = head(x)
    assert not g4.requires_grad and not m4.requires_grad and torch.equal(m4, maps_r.detach())


def test_module_still_refuses_other_layers_and_keeps_the_wrapped_wording():
    with pytest.raises(TypeError):
        NFPWithGap(nn.Identity())
    with pytest.raises(RuntimeError, match="MultiRadiusNFPPooling expected input with 4 channels"):
        NFPWithGap(MultiRadiusNFPPooling(4))(torch.zeros(1, 5, 6, 6))
    with pytest.raises(RuntimeError, match="NFPPooling expected input with 4 channels"):
        NFPWithGap(NFPPooling(4, R=1, measure="cosine", padding=1))(torch.zeros(1, 5, 6, 6))


class _Head(nn.Module):
    def __init__(self, measure, device):
        super().__init__()
        with torch.device(device):
            self.conv = nn.Conv2d(3, 16, 3, padding=1)
            self.first = NFPWithGap(MultiRadiusNFPPooling(16, measure=measure))
            self.compress = nn.Conv2d(32, 4, 1)
            self.fc = nn.Linear(16 + 4, 3)

    def forward(self, x):
        gap, maps = self.first(self.conv(x))
        return self.fc(torch.cat([gap, self.compress(maps).mean((2, 3))], dim=1)), maps


@pytest.mark.parametrize("measure,fused", [("cosine", True), ("canberra", False)])
def test_cuda_model_traces_to_one_gap_node_or_the_composition(measure, fused, lib):
    """Fake CUDA tensors, no GPU.  Served: ONE nfp_gap node yields GAP and the 32 maps.  Canberra has no two-radius kernel at
    all, so the composition is the layer's own forward — one nfp node per radius — and a mean: a single inner_R = 1 node
    would be refused by the library when the graph runs."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        net = _Head(measure, "cuda")
        ep = torch.export.export(net, (torch.empty(2, 3, 9, 9, device="cuda"),), strict=True)
    targets = [str(n.target) for n in ep.graph.nodes if n.op == "call_function"]
    assert sum("nfp_amd.nfp_gap.default" in t for t in targets) == (1 if fused else 0), targets
    assert sum("nfp_amd.nfp.default" in t for t in targets) == (0 if fused else 2), targets
    out = [n for n in ep.graph.nodes if n.op == "output"][0]
    assert tuple(out.args[0][1].meta["val"].shape) == (2, 32, 9, 9)


PARENT_HEAD_PARAMETERS = ["compress.0.weight", "compress.1.weight", "compress.1.bias", "fusion_mlp.0.weight", "fusion_mlp.0.bias",
                          "fusion_mlp.2.weight", "fusion_mlp.2.bias", "fc.weight", "fc.bias"]
PARENT_FIRST_BACKBONE_PARAMETERS = ["backbone.stem.0.weight", "backbone.stem.1.weight", "backbone.stem.1.bias"]


def test_head_net_variants_train_on_cpu_and_the_default_is_unchanged():
    from neighbour_feature_pooling_amd.models import NFPHeadNet
    torch.manual_seed(0)
    names = [n for n, _ in NFPHeadNet("resnet18", num_classes=3, bottleneck_dim=16).named_parameters()]
    assert [n for n in names if not n.startswith("backbone.")] == PARENT_HEAD_PARAMETERS
    assert names[:3] == PARENT_FIRST_BACKBONE_PARAMETERS and len(names) == 69
    for kw in (dict(R_list=(1, 2), bottleneck_dim=16), dict(R_list=(1, 2), fusion="gate", bottleneck_dim=512),
               dict(fusion="gate", bottleneck_dim=512)):
        net = NFPHeadNet("resnet18", num_classes=3, **kw)
        if "R_list" in kw:
            assert isinstance(net.gap_nfp.nfp, MultiRadiusNFPPooling) and net.compress[0].in_channels == 32
        # (96 x 96 images: a 3 x 3 feature map, the smallest that reflect padding 2 of the radius-2 layer accepts — F.pad
        # refuses the 2 x 2 map of a 64 x 64 image)
        loss = nn.functional.cross_entropy(net(torch.randn(2, 3, 96, 96)), torch.tensor([0, 2]))
        loss.backward()
        for n, p in net.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), (kw, n)
    with pytest.raises(ValueError):
        NFPHeadNet("resnet18", num_classes=3, fusion="gate", bottleneck_dim=16)


def test_torch_extension_has_the_gap_node(lib):
    import importlib.util
    path = build_torch_ext()
    _abi.load()
    spec = importlib.util.spec_from_file_location("neighbour_feature_pooling_amd._nfp_torch", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.nfp_gap_apply) and callable(mod.nfp_apply) and callable(mod.nfp_pool_apply)
    assert mod.desc_bytes == ctypes.sizeof(_abi.NfpDesc)
