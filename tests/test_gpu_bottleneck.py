"""NFPBottleneck on the device: every reference fixture (tests/golden/bneck_*.npz) through the module in float32 with the
layer served by fwd_valid / bwd_valid, a short training run of two chained blocks, bf16 channels-last against the float64
module, torch.compile and torch.autocast.

The float32 bars.  A block is ATen's conv / BatchNorm around the NFP layer, and BatchNorm over batches of 2-4 images
amplifies re-ordered sums (they move the batch variance), so the bar per tensor kind is not the kernels' 1e-5 but 4x the
worst error of the SAME module with NFP_VALID_OFF=1 — ATen on the device plus the general kernels, none of the valid-map
code — against the CPU fixtures, and not below 1e-5.  Measured on an MI355X (max over the six fixtures, relative to each
tensor's max magnitude; `measure_off_arm` below prints them):
    kind         NFP_VALID_OFF=1   4x        bar     with the valid-map kernels
    out          5.4e-7            2.1e-6    1e-5    5.4e-7
    grad_x       3.9e-7            1.5e-6    1e-5    4.6e-7
    grad_param   6.0e-7            2.4e-6    1e-5    9.0e-7
    running      2.3e-7            9.2e-7    1e-5    2.3e-7
Four times every figure lies below 1e-5, so every bar is 1e-5 — the kernels' own.

The bf16 block.  ATen's bf16 conv / BatchNorm alone put grad_x of a whole block outside the 2e-2 bar on most fixtures, with
or without the new kernels — the two arms agree to every printed digit (out / grad_x against the float64 module on the
bf16-rounded parameters and input, channels-last, valid arm = NFP_VALID_OFF=1 arm):
    fixture                    train              eval
    bneck_s1_down_4x16x9x9     6.6e-3 / 5.9e-2    4.2e-3 / 8.0e-2
    bneck_s1_ident_2x32x7x7    4.6e-3 / 5.1e-2    3.7e-3 / 7.3e-3
    bneck_s2_4x16x12x12        4.9e-3 / 1.9e-2    4.5e-3 / 1.2e-1
So the 1e-2 / 2e-2 bars against the float64 module are asserted where the path WITHOUT the new code meets them with room —
bneck_s1_ident_2x32x7x7 in eval() mode (no batch statistics, no downsample BatchNorm) — and on the train-mode step of
bneck_s1_down_4x16x9x9 the valid-map arm is held to the NFP_VALID_OFF=1 arm at the same bars, which isolates the layer.
"""
import numpy as np
import pytest
import torch

import cases_bottleneck as KB
from conftest import load_golden, rel_err
from test_bottleneck_host import bneck_module, fixture_errors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BARS = {"out": 1e-5, "grad_x": 1e-5, "grad_param": 1e-5, "running": 1e-5}      # 4x the NFP_VALID_OFF=1 figures, >= 1e-5
TOL_BF16_OUT, TOL_BF16_GX = 1e-2, 2e-2


def kind_of(name):
    return name if name in ("out", "grad_x") else ("grad_param" if name.startswith("g:") else "running")


def worst_by_kind(errs):
    worst = {}
    for k, e in errs.items():
        worst[kind_of(k)] = max(worst.get(kind_of(k), 0.0), e)
    return worst


def device_errors(c):
    """(errors of the case's step on the device against its CPU fixture, forward variant, backward variant)."""
    from neighbour_feature_pooling_amd import _abi
    L = _abi.load()
    m, g = bneck_module(c)
    m = m.to(DEV)
    x = torch.from_numpy(KB.make_input(c)).to(DEV).requires_grad_(True)
    m.zero_grad(set_to_none=True)
    out = m(x)
    fv = L.nfp_last_variant().decode()      # (the layer is the block's only call into the library)
    out.backward(torch.from_numpy(KB.make_grad_out(c, out.shape)).to(DEV))
    torch.cuda.synchronize()
    bv = L.nfp_last_variant().decode()
    grads = {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    after = {k: v.detach().float().cpu().numpy() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    return fixture_errors((out.detach().cpu().numpy(), x.grad.cpu().numpy(), grads, after), g), fv, bv


def measure_off_arm():
    """The figures behind BARS: the module with NFP_VALID_OFF=1 on the device against the CPU fixtures, worst per kind."""
    import os
    old = os.environ.get("NFP_VALID_OFF")
    os.environ["NFP_VALID_OFF"] = "1"
    try:
        worst = {}
        for c in KB.BNECK_CASES:
            errs, fv, bv = device_errors(c)
            assert not fv.startswith("fwd_valid") and not bv.startswith("bwd_valid")
            for k, e in worst_by_kind(errs).items():
                worst[k] = max(worst.get(k, 0.0), e)
    finally:
        if old is None:
            del os.environ["NFP_VALID_OFF"]
        else:
            os.environ["NFP_VALID_OFF"] = old
    return worst


@pytest.mark.parametrize("name", [c["name"] for c in KB.BNECK_CASES])
def test_device_matches_reference_fixture_on_the_valid_kernels(name):
    c = KB.BNECK_BY_NAME[name]
    errs, fv, bv = device_errors(c)
    print(name, fv, bv, worst_by_kind(errs))
    assert fv.startswith("fwd_valid<1,prod,f32,nchw") and bv.startswith("bwd_valid<1,prod,f32,nchw"), (fv, bv)
    for k, e in errs.items():
        assert e <= BARS[kind_of(k)], (k, e, BARS[kind_of(k)])


def test_the_bars_are_four_times_the_general_kernels_error():
    """BARS against what they are derived from, measured again here: no bar below 1e-5, and the NFP_VALID_OFF=1 arm — the
    path without the new code — meets the bars it sets."""
    worst = measure_off_arm()
    print("NFP_VALID_OFF=1 arm:", worst)
    for k, bar in BARS.items():
        assert bar >= 1e-5
        assert worst[k] <= bar, (k, worst[k], bar)


def test_two_chained_blocks_train():
    torch.manual_seed(0)
    from neighbour_feature_pooling_amd import NFPBottleneck, _abi
    net = torch.nn.Sequential(NFPBottleneck(16, 32), NFPBottleneck(32, 32)).to(DEV)
    c = KB.BNECK_BY_NAME["bneck_s1_down_4x16x9x9"]
    x = torch.from_numpy(KB.make_input(c)).to(DEV)
    target = torch.from_numpy(KB.make_grad_out(c, (4, 32, 5, 5))).to(DEV).abs()
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.mse_loss(net(x), target)
        assert _abi.load().nfp_last_variant().decode().startswith("fwd_valid")
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print(losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def _bf16_block(c, train):
    """(out, grad_x) of the bf16 channels-last block on the device and of the float64 module on the bf16-rounded parameters
    and input, plus the two variants."""
    from neighbour_feature_pooling_amd import _abi
    m, g = bneck_module(c)
    mb = bneck_module(c, g)[0].to(DEV).to(torch.bfloat16).to(memory_format=torch.channels_last)
    m64 = m.double()
    m64.load_state_dict({k: v.double().cpu() for k, v in mb.state_dict().items()}, strict=True)    # the bf16-rounded parameters
    mb.train(train)
    m64.train(train)
    xb = torch.from_numpy(KB.make_input(c)).bfloat16()
    go = torch.from_numpy(KB.make_grad_out(c, g["out"].shape)).bfloat16()
    x64 = xb.double().requires_grad_(True)
    ref = m64(x64)
    ref.backward(go.double())
    xd = xb.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out = mb(xd)
    fv = _abi.load().nfp_last_variant().decode()
    out.backward(go.to(DEV))
    torch.cuda.synchronize()
    bv = _abi.load().nfp_last_variant().decode()
    assert out.dtype == torch.bfloat16
    return (out.detach().float().cpu().numpy(), xd.grad.float().cpu().numpy(), ref.detach().numpy(), x64.grad.numpy(), fv, bv)


def test_bf16_channels_last_against_the_float64_module():
    out, gx, ref, gref, fv, bv = _bf16_block(KB.BNECK_BY_NAME["bneck_s1_ident_2x32x7x7"], train=False)
    assert fv.startswith("fwd_valid<1,prod,bf16,nhwc") and bv.startswith("bwd_valid<1,prod,bf16,nhwc"), (fv, bv)
    eo, eg = rel_err(out, ref), rel_err(gx, gref)
    print("bf16 channels-last, eval: out", eo, "grad_x", eg)
    assert eo <= TOL_BF16_OUT and eg <= TOL_BF16_GX


def test_bf16_train_step_agrees_with_the_general_kernels(monkeypatch):
    """The train-mode step, where ATen's bf16 BatchNorm alone misses the bars against float64 (module docstring): the
    valid-map arm against the NFP_VALID_OFF=1 arm, at the same bars."""
    c = KB.BNECK_BY_NAME["bneck_s1_down_4x16x9x9"]
    out, gx, ref, gref, fv, bv = _bf16_block(c, train=True)
    assert fv.startswith("fwd_valid<1,prod,bf16,nhwc") and bv.startswith("bwd_valid<1,prod,bf16,nhwc"), (fv, bv)
    monkeypatch.setenv("NFP_VALID_OFF", "1")
    out0, gx0, _, _, fv0, bv0 = _bf16_block(c, train=True)
    assert not fv0.startswith("fwd_valid") and not bv0.startswith("bwd_valid"), (fv0, bv0)
    eo, eg = rel_err(out, out0), rel_err(gx, gx0)
    print("bf16 channels-last, train: valid vs off arm: out", eo, "grad_x", eg,
          "| against float64: out", rel_err(out, ref), "grad_x", rel_err(gx, gref))
    assert eo <= TOL_BF16_OUT and eg <= TOL_BF16_GX


def test_compiled_block_agrees_with_eager():
    """torch.compile(fullgraph=True) traces `nfp`'s registered op (nfp_valid steps aside under tracing): it compiles, and
    agrees with the eager block at the float32 bar."""
    c = KB.BNECK_BY_NAME["bneck_s1_down_4x16x9x9"]
    m = bneck_module(c)[0].to(DEV).eval()
    x = torch.from_numpy(KB.make_input(c)).to(DEV)
    with torch.no_grad():
        eager = m(x)
        compiled = torch.compile(m, fullgraph=True)(x)
    e = rel_err(compiled.cpu().numpy(), eager.cpu().numpy())
    print("compiled vs eager", e)
    assert e <= BARS["out"]


def test_autocast_runs_and_returns_bf16():
    """Under torch.autocast(bf16) the reference's block returns bf16: conv2 is on autocast's bf16 list, BatchNorm and the
    in-place `out += identity` keep the type of `out`, whatever the identity's.  The NFP maps in between are float32 there
    (cosine_similarity is on the float32 list) and here (`_amp_input`)."""
    for name in ("bneck_s1_down_4x16x9x9", "bneck_s1_ident_2x32x7x7"):
        c = KB.BNECK_BY_NAME[name]
        m = bneck_module(c)[0].to(DEV)
        x = torch.from_numpy(KB.make_input(c)).to(DEV).requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(x)
        assert out.dtype == torch.bfloat16 and tuple(out.shape) == tuple(load_golden(name)["out"].shape)
        out.float().sum().backward()
        assert x.grad is not None and x.grad.dtype == torch.float32 and bool(torch.isfinite(x.grad).all())
