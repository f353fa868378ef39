"""nfp_with_gap / NFPWithGap (GAP(x) beside the full NFP maps, the first step of an NFP head) without a GPU: the CPU
composition, the three new C entry points, the host-only servability dry run against nfp_pool_supported's, and the
trace-time routing under torch.compile."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from neighbour_feature_pooling_amd import NFPPooling, NFPWithGap, EnhancedNFPPooling, _abi, _ops, nfp_op, nfp_with_gap
from neighbour_feature_pooling_amd.build import build_hip
from neighbour_feature_pooling_amd.functional import NfpConfig, gap_servable_static

from test_dispatch_plan import desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nfp_gap_supported", "nfp_gap_saved_floats", "nfp_gap_forward", "nfp_gap_backward")


@pytest.fixture(scope="module")
def lib():
    build_hip()
    return _abi.load()


@pytest.mark.parametrize("kw", [dict(R=1, measure="cosine", padding=1), dict(R=2, measure="norm", p=2, padding=2),
                                dict(R=1, measure="canberra", padding=0), dict(R=1, measure="scs", padding=1),
                                dict(R=1, measure="cosine", padding=1, bias=True)])
def test_cpu_tensors_equal_the_composition_values_and_both_gradients(kw):
    torch.manual_seed(3)
    layer = NFPPooling(6, **kw)
    x = torch.randn(2, 6, 5, 7, requires_grad=True)
    gap, maps = NFPWithGap(layer)(x)
    assert gap.dtype == torch.float32 and tuple(gap.shape) == (2, 6)
    xr = x.detach().clone().requires_grad_(True)
    gap_r, maps_r = xr.mean((2, 3)), layer(xr)
    assert torch.equal(gap, gap_r) and torch.equal(maps, maps_r) and maps.dtype == maps_r.dtype
    wg, wm = torch.randn_like(gap), torch.randn_like(maps)
    ((gap * wg).sum() + (maps * wm).sum()).backward()
    ((gap_r * wg).sum() + (maps_r * wm).sum()).backward()
    assert torch.allclose(x.grad, xr.grad, rtol=0, atol=1e-6)
    # one output alone, and none
    for use in ("gap", "maps"):
        x2 = x.detach().clone().requires_grad_(True)
        g2, m2 = nfp_with_gap(x2, layer.config) if not layer.bias else NFPWithGap(layer)(x2)
        ((g2 * wg).sum() if use == "gap" else (m2 * wm).sum()).backward()
        x3 = x.detach().clone().requires_grad_(True)
        ((x3.mean((2, 3)) * wg).sum() if use == "gap" else (layer(x3) * wm).sum()).backward()
        assert torch.allclose(x2.grad, x3.grad, rtol=0, atol=1e-6)
    with torch.no_grad():
        g4, m4 = NFPWithGap(layer)(x)
    assert not g4.requires_grad and not m4.requires_grad and torch.equal(m4, maps_r.detach())


def test_module_wraps_either_layer_class_and_keeps_its_state_dict_names():
    m = NFPWithGap(EnhancedNFPPooling(in_channels=4, R=1, measure="cosine", padding=1))
    assert m.out_channels == 8 and "nfp.comp_neighbors.weight" in m.state_dict()
    with pytest.raises(TypeError):
        NFPWithGap(nn.Identity())
    with pytest.raises(RuntimeError, match="expected input with 4 channels"):
        m(torch.zeros(1, 5, 4, 4))


def test_new_symbols_are_declared_listed_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "nfp.h")).read()
    assert re.search(r"#define NFP_ABI_VERSION 7\b", header) and lib.nfp_abi_version() == 7 and _abi.ABI_VERSION == 7
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _abi.EXPORTS
        assert getattr(lib, name) is not None


def _descs():
    """The descriptor list of tests/test_dispatch_plan.py's dispatch table, plus what the fused tail never serves."""
    import test_dispatch_plan as T
    marks = [m for m in T.test_forward_and_backward_variants.pytestmark if m.name == "parametrize"] \
        if hasattr(T, "test_forward_and_backward_variants") else []
    kws = [a[0] for m in marks for a in m.args[1]]
    if not kws:     # (whatever the parametrised test is called: every test of the module that takes d_kw)
        for f in vars(T).values():
            for m in getattr(f, "pytestmark", []):
                if m.name == "parametrize" and "d_kw" in str(m.args[0]):
                    kws += [a[0] for a in m.args[1]]
    assert len(kws) >= 40
    kws += [dict(shape=(4, 64, 7, 7), measure="canberra"), dict(shape=(4, 64, 8, 8), stride=2),
            dict(shape=(2, 8, 24, 24)), dict(shape=(1, 8, 23, 25), R=2, mode="replicate"), dict(shape=(0, 8, 7, 7))]
    return kws


def test_gap_supported_answers_as_pool_supported(lib):
    served = 0
    for kw in _descs():
        d = desc(**kw)
        for ws in (None, 0x1000):       # without and with the workspace the descriptor is entitled to
            d.ws = ws if (ws is None or lib.nfp_workspace_bytes(ctypes.byref(d)) > 0) else None
            g, p = lib.nfp_gap_supported(ctypes.byref(d)), lib.nfp_pool_supported(ctypes.byref(d))
            assert g == p, (kw, ws, g, p)
            if g:
                served += 1
                assert lib.nfp_gap_saved_floats(ctypes.byref(d)) >= 0, kw
    assert served >= 20
    for kw in (dict(shape=(4, 64, 7, 7), measure="canberra"), dict(shape=(4, 64, 8, 8), stride=2)):
        assert lib.nfp_gap_supported(ctypes.byref(desc(**kw))) == 0


def test_dry_run_launches_nothing_and_keeps_the_last_variant(lib):
    d = desc((64, 512, 7, 7))
    d.ws = 0x1000
    before, n0 = lib.nfp_last_variant(), lib.nfp_launch_count()
    assert lib.nfp_gap_supported(ctypes.byref(d)) == 1
    # per-pixel norms + nothing else: one band per image on the table kernels
    assert lib.nfp_gap_saved_floats(ctypes.byref(d)) == 64 * 49
    d2 = desc((2, 8, 24, 24))       # row bands: 12 rows of C partial sums per image behind the norms
    assert lib.nfp_gap_saved_floats(ctypes.byref(d2)) == 2 * 576 + 2 * 12 * 8
    assert lib.nfp_launch_count() == n0 and lib.nfp_last_variant() == before


def test_entry_points_refuse_before_touching_anything(lib):
    d = desc((4, 64, 7, 7), measure="canberra")
    fake = ctypes.c_void_p(0x1000)
    n0 = lib.nfp_launch_count()
    assert lib.nfp_gap_forward(ctypes.byref(d), fake, fake, fake, fake, 1 << 20, None) == -2
    assert lib.nfp_gap_backward(ctypes.byref(d), fake, None, fake, fake, fake, 1 << 20, fake, None) == -2
    d = desc((4, 64, 7, 7))
    d.ws = 0x1000
    need = lib.nfp_gap_saved_floats(ctypes.byref(d))
    assert need == 4 * 49
    assert lib.nfp_gap_forward(ctypes.byref(d), fake, fake, fake, fake, need - 1, None) == -1     # short `saved`
    assert b"saved holds" in lib.nfp_last_error()
    assert lib.nfp_gap_forward(ctypes.byref(d), fake, fake, fake, None, need, None) == -1
    assert lib.nfp_gap_backward(ctypes.byref(d), fake, None, fake, fake, fake, need - 1, fake, None) == -1
    assert lib.nfp_gap_forward(ctypes.byref(d), fake, None, fake, fake, need, None) == -1         # null gap
    assert lib.nfp_launch_count() == n0


def test_trace_time_servability_is_the_host_only_dry_run(lib):
    cos = NfpConfig(R=1, measure="cosine", padding=1)
    assert gap_servable_static((4, 64, 7, 7), (64 * 49, 49, 7, 1), torch.float32, cos)
    assert gap_servable_static((4, 64, 7, 7), (64 * 49, 1, 7 * 64, 64), torch.bfloat16, cos)
    assert gap_servable_static((4, 64, 7, 7), (50 * 64, 1, 7 * 64, 64), torch.float32, cos)       # tokens behind a class token
    assert not gap_servable_static((4, 64, 7, 7), (64 * 49, 49, 7, 1), torch.float32, NfpConfig(R=1, measure="canberra", padding=1))
    assert not gap_servable_static((4, 64, 7, 7), (64 * 49, 49, 7, 1), torch.float32, NfpConfig(R=1, measure="cosine", padding=0))
    assert not gap_servable_static((4, 62, 7, 7), (62 * 49, 49, 7, 1), torch.float32, cos)          # C % 4 != 0
    assert not gap_servable_static((4, 64, 7, 7), (64 * 49, 49, 7, 1), torch.float16, cos)


class _Head(nn.Module):
    def __init__(self, measure, device):
        super().__init__()
        with torch.device(device):
            self.conv = nn.Conv2d(3, 16, 3, padding=1)
            self.first = NFPWithGap(NFPPooling(16, R=1, measure=measure, padding=1))
            self.compress = nn.Conv2d(8, 4, 1)
            self.fc = nn.Linear(16 + 4, 3)

    def forward(self, x):
        gap, maps = self.first(self.conv(x))
        return self.fc(torch.cat([gap, self.compress(maps).mean((2, 3))], dim=1))


@pytest.mark.parametrize("measure,fused", [("cosine", True), ("canberra", False)])
def test_cuda_model_traces_to_one_graph_served_or_composed(measure, fused, lib):
    """Fake CUDA tensors, no GPU: a served call is ONE nfp_gap node; a call the fused kernels refuse is traced as the
    composition (the maps' own op and a mean) — decided at trace time, so nothing is left to raise inside the graph."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        net = _Head(measure, "cuda")
        ep = torch.export.export(net, (torch.empty(2, 3, 9, 9, device="cuda"),), strict=True)
    targets = [str(n.target) for n in ep.graph.nodes if n.op == "call_function"]
    assert sum("nfp_amd.nfp_gap.default" in t for t in targets) == (1 if fused else 0), targets
    assert sum("nfp_amd.nfp.default" in t for t in targets) == (0 if fused else 1), targets
    out = [n for n in ep.graph.nodes if n.op == "output"][0]
    assert tuple(out.args[0][0].meta["val"].shape) == (2, 3)


def test_fake_implementation_states_shapes_and_an_upper_bound_of_the_state(lib):
    from torch._subclasses.fake_tensor import FakeTensorMode
    cfg = NfpConfig(R=2, measure="norm", p=2, padding=2)
    with FakeTensorMode():
        x = torch.empty(3, 16, 30, 20, device="cuda", dtype=torch.bfloat16)
        gap, maps, saved = torch.ops.nfp_amd.nfp_gap(x, *_ops.cfg_args(cfg))
        assert tuple(gap.shape) == (3, 16) and gap.dtype == torch.float32
        assert tuple(maps.shape) == (3, 24, 30, 20) and maps.dtype == torch.bfloat16
        gx = torch.ops.nfp_amd.nfp_gap_backward(x, maps, saved, None, maps, *_ops.cfg_args(cfg))
        assert gx.shape == x.shape and gx.dtype == x.dtype
    d = desc((3, 16, 30, 20), R=2, measure="norm", dtype=_abi.BF16)
    assert 0 < lib.nfp_gap_saved_floats(ctypes.byref(d)) <= saved.numel()


def test_head_net_trains_on_cpu():
    from neighbour_feature_pooling_amd.models import NFPHeadNet
    torch.manual_seed(0)
    net = NFPHeadNet("resnet18", num_classes=3, bottleneck_dim=16)
    loss = nn.functional.cross_entropy(net(torch.randn(2, 3, 64, 64)), torch.tensor([0, 2]))
    loss.backward()
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
