"""The NCHW staging form of the table kernels, as nfp_plan reports it — no GPU needed.

fwd_band / bwd_fast stage a dense NCHW map in 4-pixel x 4-channel blocks; the k = 3 float32 backward of one class of
launches stages it by pixel rows instead (csrc/nfp_fast.h: StagedRows; the forward was built the same way, measured no
faster and keeps its blocks).  The launch record of nfp_plan carries the form as a token behind `lds=`; the variant strings
and `grid= block= lds=` are those tests/test_dispatch_plan.py pins, whichever form serves."""
import pytest

from conftest import nfp_switch
from neighbour_feature_pooling_amd import _abi
from neighbour_feature_pooling_amd.build import build_hip
from test_dispatch_plan import desc, launches, plan


@pytest.fixture(scope="module")
def lib():
    build_hip()
    return _abi.load()


def _records(lib, d):
    out = []
    for backward in (False, True):
        rc, text = plan(lib, d, backward)
        assert rc == 0, lib.nfp_last_error()
        out.append(text)
    return out


def test_headline_plan_keeps_its_strings_and_names_the_form(lib, monkeypatch):
    d = desc((64, 512, 7, 7))
    fwd, bwd = _records(lib, d)
    assert fwd.startswith("fwd_band<R1,cos,f32,nchw>x4 | fwd_band grid=(64,4,1)"), fwd
    assert fwd.split(" | ")[0] == "fwd_band<R1,cos,f32,nchw>x4" and bwd.split(" | ")[0] == "bwd_fast<R1,cos,f32,nchw>"
    assert fwd.endswith(" stage=blocks") and bwd.endswith(" stage=rows"), (fwd, bwd)
    nfp_switch(monkeypatch, "NFP_STAGE_BLOCKS", "1")
    fwd_b, bwd_b = _records(lib, d)
    assert fwd_b == fwd and bwd_b.endswith(" stage=blocks"), (fwd_b, bwd_b)
    # only the token differs: same variant, grid, block and LDS bytes under either form
    assert bwd_b[:-len(" stage=blocks")] == bwd[:-len(" stage=rows")]
    assert launches(fwd) == launches(fwd_b) and launches(bwd) == launches(bwd_b)
    nfp_switch(monkeypatch, "NFP_STAGE_BLOCKS", None)
    assert _records(lib, d) == [fwd, bwd]


#  descriptor                                                        forward token    backward token (the forward: always blocks)
CLASS = [
    (dict(shape=(64, 512, 7, 7), measure="norm"),                     "stage=blocks",  "stage=rows"),     # L2
    (dict(shape=(64, 512, 7, 7), measure="dot"),                      "stage=blocks",  "stage=rows"),     # VAR riders
    (dict(shape=(64, 512, 7, 7), measure="gfc"),                      "stage=blocks",  "stage=rows"),
    (dict(shape=(64, 512, 7, 7), measure="rmse"),                     "stage=blocks",  "stage=rows"),
    (dict(shape=(256, 512, 7, 7)),                                    "stage=blocks",  "stage=blocks"),   # config 4: the backward takes two chunks
    (dict(shape=(128, 512, 7, 7)),                                    "stage=blocks",  "stage=blocks"),   # one chunk, but 64 quads on 10 groups
                                                                      # are 7 slots per thread: above the rows form's 6 (kRS)
    (dict(shape=(64, 348, 7, 7)),                                     "stage=blocks",  "stage=rows"),     # 22 quads on 8 groups: 3 slots
    (dict(shape=(64, 512, 7, 7), measure="norm", p=1.0),              "stage=blocks",  "stage=blocks"),   # Norm p = 1 keeps the blocks
    (dict(shape=(64, 512, 7, 7), measure="chisquared1"),              "stage=blocks",  "stage=blocks"),   # symmetric-term measures too
    (dict(shape=(64, 512, 7, 7), R=2),                                "stage=blocks",  "stage=blocks"),   # k = 5
    (dict(shape=(4096, 512, 7, 7)),                                   "stage=blocks",  "stage=blocks"),   # saturating batch
    (dict(shape=(2, 4096, 7, 7)),                                     "stage=blocks",  "stage=rows"),     # forward: several chunks; the
                                                                      # backward splits the channels over 128 workgroups, one chunk each
    (dict(shape=(64, 512, 7, 7), channels_last=True),                 None,            None),             # not an NCHW launch
    (dict(shape=(64, 200, 7, 7), dtype=_abi.BF16),                    "stage=blocks",  "stage=blocks"),   # bf16 on the vector kernels
]


@pytest.mark.parametrize("d_kw,fwd_tok,bwd_tok", CLASS, ids=[str(i) for i in range(len(CLASS))])
def test_which_launches_stage_by_rows(lib, d_kw, fwd_tok, bwd_tok):
    fwd, bwd = _records(lib, desc(**d_kw))
    for text, tok in ((fwd, fwd_tok), (bwd, bwd_tok)):
        assert "stage=rows" not in text or tok == "stage=rows", text
        if tok is not None:
            assert text.endswith(" " + tok), text
        else:
            assert "stage=" not in text, text
