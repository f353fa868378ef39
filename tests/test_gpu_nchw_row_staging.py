"""NCHW maps staged by pixel rows in the k = 3 float32 table backward (csrc/nfp_fast.h: StagedRows).

fwd_band and bwd_fast fill their LDS slab from a dense NCHW map in 4-pixel x 4-channel blocks transposed in registers.
bwd_fast has a second form for one class of launches — float32, k = 3, plain maps, cosine / L2 and their riders, one
channel chunk, at most one workgroup per CU: thread (channel group, pixel) loads the slots it reads first itself, four
coalesced 4-byte loads per slot, and holds the slot's float4.  Only the route into the slab differs, so the two forms
must agree BITWISE; NFP_STAGE_BLOCKS=1 forces the block form.  (The forward was built the same way, measured no faster and
keeps its blocks: nfp_plan says `stage=blocks` for it under either value of the switch.)

Every case runs forward and backward under both values of the switch and asserts that the default arm matches the
oracle, that its `out` and `grad_x` are bit-identical to the block arm's, and that nfp_plan names the form each arm
launched.  A backward workgroup owns Cwg channels = Cwg / 4 quads, on G channel groups (csrc/nfp_table_bwd.hip:
launch_bwd_fast_t); a thread stages ceil(quads / G) slots.  Small batches split the channels down to one quad per
workgroup, so the small shapes — P % 4 != 0, the smallest map, H != W, one quad, 129 quads (a last workgroup of one quad
beside two-quad ones), the padding modes, L2 and a VAR measure, a batch stride that is not C * P — run ONE slot per
thread; the B = 64 shapes run several: two and four full rounds, and [64,348,7,7], whose rounds are 8 + 8 + 6 quads (8 + 8
+ 5 in the image's last workgroup): a partial last round, i.e. clamped loads that commit nothing, and the skipped rounds
behind it.  Four cases at the class's edge: [2,4096,7,7] (the forward takes several chunks; the backward splits the
channels over 128 workgroups of one chunk each and stays inside the class), [256,512,7,7] (the backward takes two
chunks), bf16 and channels-last, which keep the blocks and still match the oracle.

Referee and tolerances: those of tests/test_gpu_entry_args.py — the CPU oracle on the same inputs; float32 at TOL, bf16
storage at 1e-2 (maps) / 2e-2 (gradients) against the oracle on the bf16-rounded inputs."""
import ctypes

import pytest
import torch

from conftest import nfp_switch
from neighbour_feature_pooling_amd import NFPPooling, _abi
from neighbour_feature_pooling_amd import functional as F
from neighbour_feature_pooling_amd.synth import feature_map
from test_gpu_entry_args import COS, _check, _reference

pytestmark = pytest.mark.gpu

L2 = dict(R=1, measure="norm", p=2, padding=1)
DOT = dict(R=1, measure="dot", padding=1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _abi.load()
    return torch.device("cuda:0")


def _plans(x, ctor):
    """nfp_plan's (forward, backward) records for the call NFPPooling(**ctor)(x) makes."""
    lib = _abi.load()
    d = F.make_desc(x, NFPPooling(x.shape[1], **ctor).config)
    out = []
    for backward in (0, 1):
        buf = ctypes.create_string_buffer(1024)
        assert lib.nfp_plan(ctypes.byref(d), backward, buf, len(buf)) == 0, lib.nfp_last_error()
        out.append(buf.value.decode())
    return out


def _arm(make_x, go, ctor):
    """Forward + backward on a fresh leaf; (out, grad_x, forward variant, backward variant, forward plan, backward plan)."""
    lib = _abi.load()
    x = make_x()
    n0 = lib.nfp_launch_count()
    out = NFPPooling(x.shape[1], **ctor)(x)
    fv = lib.nfp_last_variant().decode()
    out.backward(go)
    torch.cuda.synchronize()
    bv = lib.nfp_last_variant().decode()
    assert lib.nfp_launch_count() == n0 + 2, (fv, bv)
    return (out.detach(), x.grad.detach(), fv, bv) + tuple(_plans(x, ctor))


def _both_arms(monkeypatch, name, make_x, go, ctor, ref_out, ref_gx, expect=("stage=blocks", "stage=rows"), bf=False,
               fwd="fwd_band<"):
    """`expect`: the (forward, backward) token of the default arm; None = the record carries no token at all."""
    nfp_switch(monkeypatch, "NFP_STAGE_BLOCKS", None)
    out_r, gx_r, fv, bv, pf, pb = _arm(make_x, go, ctor)
    for text, tok in ((pf, expect[0]), (pb, expect[1])):
        assert (text.endswith(" " + tok) if tok else "stage=" not in text), (text, tok)
    assert pf.split(" | ")[0] == fv and pb.split(" | ")[0] == bv, (pf, fv, pb, bv)
    _check(name + "[default]", out_r.float().cpu().numpy(), gx_r.float().cpu().numpy(), ref_out, ref_gx, fv, bv, bf=bf, fwd=fwd)
    nfp_switch(monkeypatch, "NFP_STAGE_BLOCKS", "1")
    out_b, gx_b, fv_b, bv_b, pf_b, pb_b = _arm(make_x, go, ctor)
    assert (fv_b, bv_b) == (fv, bv)
    for text, tok in ((pf_b, expect[0]), (pb_b, expect[1])):
        assert (text.endswith(" stage=blocks") if tok else "stage=" not in text), text
    _check(name + "[blocks]", out_b.float().cpu().numpy(), gx_b.float().cpu().numpy(), ref_out, ref_gx, fv_b, bv_b, bf=bf, fwd=fwd)
    assert torch.equal(out_r, out_b), f"{name}: out differs between the two staging forms"
    assert torch.equal(gx_r, gx_b), f"{name}: grad_x differs between the two staging forms"
    return fv, bv


#         name               shape             ctor                                  the backward's workgroups: quads on groups -> slots per thread
ROWS = [("many_bands",      (3, 16, 7, 7),    COS),                                   # 1 on 1 (P % 4 = 1; forward: 7 bands)
        ("smallest_map",    (2, 8, 2, 2),     COS),                                   # 1 on 1, P = 4
        ("non_square",      (5, 12, 5, 6),    COS),                                   # 1 on 1, H != W
        ("one_quad",        (2, 4, 7, 7),     COS),                                   # 1 on 1, one workgroup per image
        ("129_quads",       (2, 516, 7, 7),   COS),                                   # 2 on 2, the last workgroup 1 on 2: an idle group's clamp
        ("small_split",     (64, 32, 7, 7),   COS),                                   # 2 on 2 -> 1; grid (64, 4) as the headline (forward: 4 bands)
        ("one_image",       (1, 512, 7, 7),   COS),                                   # 1 on 1, 128 workgroups
        ("two_rounds",      (64, 256, 7, 7),  COS),                                   # 16 on 8 -> 2 full rounds
        ("partial_round",   (64, 348, 7, 7),  COS),                                   # 22 on 8 -> 8 + 8 + 6; last workgroup 21 -> 8 + 8 + 5
        ("headline",        (64, 512, 7, 7),  COS),                                   # 32 on 8 -> 4 full rounds
        ("pad_zeros",       (3, 16, 7, 7),    dict(COS, padding_mode="zeros")),
        ("pad_replicate",   (3, 16, 7, 7),    dict(COS, padding_mode="replicate")),
        ("l2",              (3, 16, 7, 7),    L2),
        ("dot",             (3, 16, 7, 7),    DOT),                                   # VAR
        ("l2_partial",      (64, 348, 7, 7),  L2)]                                    # the L2 instantiation with several slots
BLOCK = {"two_rounds": 448, "partial_round": 448, "headline": 448, "l2_partial": 448}   # 8 groups x 49 pixels, in wavefronts


@pytest.mark.parametrize("name,shape,ctor", ROWS, ids=[c[0] for c in ROWS])
def test_rows_match_oracle_and_blocks_bitwise(name, shape, ctor, dev, oracle_lib, monkeypatch):
    xh, goh, ref_out, ref_gx = _reference(oracle_lib, shape, ctor)
    xd, go = torch.tensor(xh).to(dev), torch.tensor(goh).to(dev)
    fv, _ = _both_arms(monkeypatch, name, lambda: xd.clone().requires_grad_(True), go, ctor, ref_out, ref_gx)
    if name == "many_bands":
        assert fv.endswith("x7"), fv
    if name in ("small_split", "headline"):
        assert fv.endswith("x4"), fv
    if name in BLOCK:   # the launch shape the slot counts above are derived from
        assert f"grid=(64,4,1) block={BLOCK[name]} " in _plans(xd, ctor)[1]


def test_batch_strided_view(dev, oracle_lib, monkeypatch):
    """x = big[:, :16] of a [3,32,7,7] tensor: batch stride 32 * 49, not C * P."""
    shape = (3, 16, 7, 7)
    xh, goh, ref_out, ref_gx = _reference(oracle_lib, shape, COS)
    big = torch.tensor(feature_map((3, 32, 7, 7), 77)).to(dev)
    big[:, :16] = torch.tensor(xh).to(dev)

    def view():
        x = big[:, :16].detach().requires_grad_(True)
        assert x.stride(0) == 32 * 49 and not x.is_contiguous()
        return x
    _both_arms(monkeypatch, "strided_view", view, torch.tensor(goh).to(dev), COS, ref_out, ref_gx)


def test_several_chunks(dev, oracle_lib, monkeypatch):
    """[2,4096,7,7]: the forward stages its 1024 quads in several chunks.  The backward splits the channels over 128
    workgroups of 32 channels, one chunk each: inside the class."""
    shape = (2, 4096, 7, 7)
    xh, goh, ref_out, ref_gx = _reference(oracle_lib, shape, COS)
    xd = torch.tensor(xh).to(dev)
    _both_arms(monkeypatch, "several_chunks", lambda: xd.clone().requires_grad_(True), torch.tensor(goh).to(dev), COS,
               ref_out, ref_gx, expect=("stage=blocks", "stage=rows"))


def test_two_chunk_backward_keeps_the_blocks(dev, oracle_lib, monkeypatch):
    """[256,512,7,7] (config 4): one workgroup per image, its 128 quads in two chunks — outside the class."""
    shape = (256, 512, 7, 7)
    xh, goh, ref_out, ref_gx = _reference(oracle_lib, shape, COS)
    xd = torch.tensor(xh).to(dev)
    _both_arms(monkeypatch, "two_chunks", lambda: xd.clone().requires_grad_(True), torch.tensor(goh).to(dev), COS,
               ref_out, ref_gx, expect=("stage=blocks", "stage=blocks"))


def test_bf16_keeps_the_blocks(dev, oracle_lib, monkeypatch):
    """bf16 storage on the vector kernels (NFP_MFMA=0: fwd_band / the vector bwd_fast)."""
    nfp_switch(monkeypatch, "NFP_MFMA", "0")
    shape = (2, 32, 7, 7)
    xh, goh, ref_out, ref_gx = _reference(oracle_lib, shape, COS, bf=True)
    xd = torch.tensor(xh).to(dev, torch.bfloat16)
    _both_arms(monkeypatch, "bf16", lambda: xd.clone().requires_grad_(True), torch.tensor(goh).to(dev, torch.bfloat16), COS,
               ref_out, ref_gx, expect=("stage=blocks", "stage=blocks"), bf=True)


def test_channels_last_is_not_staged_by_rows(dev, oracle_lib, monkeypatch):
    shape = (3, 16, 7, 7)
    xh, goh, ref_out, ref_gx = _reference(oracle_lib, shape, COS)
    xd = torch.tensor(xh).to(dev).contiguous(memory_format=torch.channels_last)
    fv, bv = _both_arms(monkeypatch, "channels_last", lambda: xd.clone(memory_format=torch.preserve_format).requires_grad_(True),
                        torch.tensor(goh).to(dev), COS, ref_out, ref_gx, expect=(None, None))
    assert ",nhwc" in fv and ",nhwc" in bv, (fv, bv)
