"""What the forward / backward entry points of csrc/nfp_hip.hip answer BEFORE anything launches — return code and the
leading words of nfp_last_error() — as one table, without a GPU.  The rows pin two things a fold of the entries' shared
checks must keep: each refusal's text, and, where two checks fail at once, which one wins (the pool entries look at the
pointers before the measure and before the empty batch; the gap entries at the measure, then the empty batch, then the
pointers; the valid and biased entries at x / out only for B > 0).  Every row leaves nfp_launch_count() as it was.

(An empty biased backward is not refused: it launches bias_reduce to zero the bias gradients, so its B = 0 row here is
the one with a required bias pointer missing.)"""
import ctypes

import pytest

from neighbour_feature_pooling_amd import _abi
from neighbour_feature_pooling_amd.build import build_hip

from test_dispatch_plan import desc

F = 0x1000   # a stand-in device pointer: no row gets as far as reading it
NULL = "null tensor pointer"


@pytest.fixture(scope="module")
def lib():
    build_hip()
    return _abi.load()


def D(shape=(2, 8, 7, 7), ws=F, inner_R=0, map_f32=0, **kw):
    return dict(shape=shape, ws=ws, inner_R=inner_R, map_f32=map_f32, **kw)


COS, CANB, SCS, DOT = D(), D(measure="canberra"), D(measure="scs"), D(measure="dot")
COS0, CANB0 = D(shape=(0, 8, 7, 7)), D(shape=(0, 8, 7, 7), measure="canberra")
MIXED = D(dtype=_abi.BF16, map_f32=1)
TWO_RADII = D(R=2, inner_R=1)
BANDS = D(shape=(2, 8, 24, 24), ws=None)                      # 576 pixels: the row-band kernels, no tables
VCOS, VCANB = D(pad=0, ws=None), D(pad=0, ws=None, measure="canberra")   # valid maps
VCOS0 = D(shape=(0, 8, 7, 7), pad=0, ws=None)
VL1, VL10 = D(pad=0, ws=None, measure="norm", p=1.0), D(shape=(0, 8, 7, 7), pad=0, ws=None, measure="norm", p=1.0)
ATT = D(measure="attention")
NORM0 = D(shape=(0, 8, 7, 7), measure="norm")

# (id, entry, descriptor, the arguments behind it, return code, leading words of nfp_last_error() — None: not refused)
CASES = [
    # nfp_forward(d, x, out, saved, stream)
    ("fwd-null-x", "nfp_forward", COS, (None, F, F, None), -1, NULL),
    ("fwd-unserved", "nfp_forward", SCS, (F, F, F, None), -2, "measure 16 (SharpenedCosine mixes batch elements"),
    ("fwd-mixed-attention", "nfp_forward", D(measure="attention", dtype=_abi.BF16, map_f32=1), (F, F, F, None), -2,
     "map_f32: one radius"),
    ("fwd-attention-bf16-no-saved", "nfp_forward", D(measure="attention", dtype=_abi.BF16), (F, F, None, None), -1,
     "attention on bf16 maps needs the scratch of nfp_saved_floats"),
    ("fwd-empty-null", "nfp_forward", COS0, (None, None, None, None), -1, NULL),
    ("fwd-empty", "nfp_forward", COS0, (F, F, None, None), 0, None),
    # nfp_backward(d, x, grad_out, out, saved, grad_x, stream)
    ("bwd-null-gx", "nfp_backward", COS, (F, F, F, F, None, None), -1, NULL),
    ("bwd-no-saved", "nfp_backward", COS, (F, F, F, None, F, None), -1, "measure 1 needs the saved state of nfp_forward"),
    ("bwd-null-gx-and-no-saved", "nfp_backward", COS, (F, F, F, None, None, None), -1, NULL),
    ("bwd-unserved", "nfp_backward", SCS, (F, F, F, None, F, None), -2, "measure 16 (SharpenedCosine) has no HIP kernel"),
    ("bwd-empty-null", "nfp_backward", COS0, (None, None, None, None, None, None), -1, NULL),
    ("bwd-empty-no-saved", "nfp_backward", COS0, (F, F, F, None, F, None), -1, "measure 1 needs the saved state"),
    ("bwd-empty", "nfp_backward", COS0, (F, F, F, F, F, None), 0, None),
    # nfp_pool_forward(d, x, gap, nfpm, out_map, saved, stream)
    ("pool-fwd-null-nfpm", "nfp_pool_forward", COS, (F, F, None, F, F, None), -1, NULL),
    ("pool-fwd-unserved", "nfp_pool_forward", CANB, (F, F, F, F, F, None), -2, "fused pooling tail: cosine / dot / gfc / L2 (norm p=2) / rmse, one radius"),
    ("pool-fwd-two-radii", "nfp_pool_forward", TWO_RADII, (F, F, F, F, F, None), -2, "fused pooling tail: cosine"),
    ("pool-fwd-mixed", "nfp_pool_forward", MIXED, (F, F, F, F, F, None), -2, "fused pooling tail: cosine"),
    ("pool-fwd-null-x-and-unserved", "nfp_pool_forward", CANB, (None, F, F, F, F, None), -1, NULL),
    ("pool-fwd-bands-no-saved", "nfp_pool_forward", BANDS, (F, F, F, F, None, None), -1,
     "fused pooling tail on this map needs the scratch of nfp_pool_saved_floats"),
    ("pool-fwd-empty-null", "nfp_pool_forward", COS0, (None, None, None, None, None, None), -1, NULL),
    ("pool-fwd-empty-unserved", "nfp_pool_forward", CANB0, (F, F, F, F, F, None), -2, "fused pooling tail: cosine"),
    ("pool-fwd-empty", "nfp_pool_forward", COS0, (F, None, F, None, None, None), 0, None),
    # nfp_pool_backward(d, x, grad_gap, grad_nfpm, out_map, saved, grad_x, stream)
    ("pool-bwd-null-gnfpm", "nfp_pool_backward", COS, (F, F, None, F, F, F, None), -1, NULL),
    ("pool-bwd-unserved", "nfp_pool_backward", CANB, (F, F, F, F, F, F, None), -2, "fused pooling tail: cosine / dot / gfc / L2 (norm p=2) / rmse, one radius"),
    ("pool-bwd-no-saved", "nfp_pool_backward", COS, (F, F, F, F, None, F, None), -1, "missing saved state"),
    ("pool-bwd-null-x-and-unserved", "nfp_pool_backward", CANB, (None, F, F, F, F, F, None), -1, NULL),
    ("pool-bwd-mixed-and-no-saved", "nfp_pool_backward", MIXED, (F, F, F, F, None, F, None), -2, "fused pooling tail: cosine"),
    ("pool-bwd-empty-null", "nfp_pool_backward", COS0, (None, None, None, None, None, None, None), -1, NULL),
    ("pool-bwd-empty-no-saved", "nfp_pool_backward", COS0, (F, None, F, F, None, F, None), -1, "missing saved state"),
    ("pool-bwd-empty", "nfp_pool_backward", COS0, (F, None, F, F, F, F, None), 0, None),
    # nfp_gap_forward(d, x, gap, out_map, saved, saved_floats, stream)
    ("gap-fwd-null-gap", "nfp_gap_forward", COS, (F, None, F, F, 98, None), -1, NULL),
    ("gap-fwd-unserved", "nfp_gap_forward", CANB, (F, F, F, F, 1 << 20, None), -2, "GAP beside the maps: cosine / dot / gfc / L2 (norm p=2) / rmse"),
    ("gap-fwd-mixed", "nfp_gap_forward", MIXED, (F, F, F, F, 1 << 20, None), -2, "GAP beside the maps: cosine"),
    ("gap-fwd-short-saved", "nfp_gap_forward", COS, (F, F, F, F, 97, None), -1, "saved holds 97 floats, nfp_gap_saved_floats is 98"),
    ("gap-fwd-no-saved", "nfp_gap_forward", COS, (F, F, F, None, 98, None), -1, "saved holds 0 floats, nfp_gap_saved_floats is 98"),
    ("gap-fwd-no-saved-no-state", "nfp_gap_forward", DOT, (F, F, F, None, 0, None), -1, "saved holds 0 floats, nfp_gap_saved_floats is 1"),
    ("gap-fwd-null-x-and-unserved", "nfp_gap_forward", CANB, (None, F, F, F, 98, None), -2, "GAP beside the maps: cosine"),
    ("gap-fwd-null-gap-and-short-saved", "nfp_gap_forward", COS, (F, None, F, F, 97, None), -1, NULL),
    ("gap-fwd-empty-null", "nfp_gap_forward", COS0, (None, None, None, None, 0, None), 0, None),
    ("gap-fwd-empty-unserved", "nfp_gap_forward", CANB0, (None, None, None, None, 0, None), -2, "GAP beside the maps: cosine"),
    # nfp_gap_backward(d, x, grad_gap, grad_out, out_map, saved, saved_floats, grad_x, stream)
    ("gap-bwd-null-go", "nfp_gap_backward", COS, (F, F, None, F, F, 98, F, None), -1, NULL),
    ("gap-bwd-unserved", "nfp_gap_backward", CANB, (F, F, F, F, F, 1 << 20, F, None), -2, "GAP beside the maps: cosine / dot / gfc / L2 (norm p=2) / rmse"),
    ("gap-bwd-short-saved", "nfp_gap_backward", COS, (F, None, F, F, F, 97, F, None), -1, "saved holds 97 floats, the backward reads 98"),
    ("gap-bwd-no-saved", "nfp_gap_backward", COS, (F, None, F, F, None, 98, F, None), -1, "saved holds 0 floats, the backward reads 98"),
    ("gap-bwd-null-gx-and-unserved", "nfp_gap_backward", CANB, (F, F, F, F, F, 98, None, None), -2, "GAP beside the maps: cosine"),
    ("gap-bwd-null-gx-and-short-saved", "nfp_gap_backward", COS, (F, F, F, F, F, 97, None, None), -1, NULL),
    ("gap-bwd-empty-null", "nfp_gap_backward", COS0, (None, None, None, None, None, 0, None, None), 0, None),
    # nfp_valid_forward(d, x, out, saved, saved_floats, stream)
    ("valid-fwd-null-out", "nfp_valid_forward", VCOS, (F, None, F, 98, None), -1, NULL),
    ("valid-fwd-unserved", "nfp_valid_forward", VCANB, (F, F, F, 98, None), -2, "valid maps: "),
    ("valid-fwd-padded", "nfp_valid_forward", D(ws=None), (F, F, F, 98, None), -2, "valid maps: "),
    ("valid-fwd-short-saved", "nfp_valid_forward", VCOS, (F, F, F, 97, None), -1, "saved holds 97 floats, nfp_valid_saved_floats is 98"),
    ("valid-fwd-null-out-and-short-saved", "nfp_valid_forward", VCOS, (F, None, F, 97, None), -1, NULL),
    ("valid-fwd-null-x-and-unserved", "nfp_valid_forward", VCANB, (None, F, F, 98, None), -2, "valid maps: "),
    ("valid-fwd-empty-null", "nfp_valid_forward", VCOS0, (None, None, None, 0, None), 0, None),
    # nfp_valid_backward(d, x, grad_out, out, saved, saved_floats, grad_x, stream)
    ("valid-bwd-null-gx", "nfp_valid_backward", VCOS, (F, F, F, F, 98, None, None), -1, NULL),
    ("valid-bwd-unserved", "nfp_valid_backward", VCANB, (F, F, F, F, 98, F, None), -2, "valid maps: "),
    ("valid-bwd-short-saved", "nfp_valid_backward", VCOS, (F, F, F, F, 97, F, None), -1, "saved holds 97 floats, nfp_valid_saved_floats is 98"),
    ("valid-bwd-no-saved", "nfp_valid_backward", VCOS, (F, F, F, None, 98, F, None), -1, "saved holds 0 floats, nfp_valid_saved_floats is 98"),
    ("valid-bwd-empty-null", "nfp_valid_backward", VCOS0, (None, None, None, None, 0, None, None), 0, None),
    # nfp_valid_abs_forward(d, x, out, stream) / nfp_valid_abs_backward(d, x, grad_out, grad_x, stream)
    ("valid-abs-fwd-null-out", "nfp_valid_abs_forward", VL1, (F, None, None), -1, NULL),
    ("valid-abs-fwd-unserved", "nfp_valid_abs_forward", VCOS, (F, F, None), -2, "valid L1 maps: "),
    ("valid-abs-fwd-null-x-and-unserved", "nfp_valid_abs_forward", VCOS, (None, F, None), -2, "valid L1 maps: "),
    ("valid-abs-fwd-empty-null", "nfp_valid_abs_forward", VL10, (None, None, None), 0, None),
    ("valid-abs-bwd-null-go", "nfp_valid_abs_backward", VL1, (F, None, F, None), -1, NULL),
    ("valid-abs-bwd-unserved", "nfp_valid_abs_backward", VCOS, (F, F, F, None), -2, "valid L1 maps: "),
    ("valid-abs-bwd-empty-null", "nfp_valid_abs_backward", VL10, (None, None, None, None), 0, None),
    # nfp_bias_forward(d, x, centre_bias, neighbour_bias, out, saved, saved_floats, stream)
    ("bias-fwd-null-x", "nfp_bias_forward", COS, (None, F, F, F, F, 1568, None), -1, NULL),
    ("bias-fwd-null-centre", "nfp_bias_forward", COS, (F, None, F, F, F, 1568, None), -1, NULL),
    ("bias-fwd-unserved", "nfp_bias_forward", SCS, (F, F, F, F, F, 1568, None), -2, "biased NFP: measure 16 (SharpenedCosine mixes batch elements)"),
    ("bias-fwd-two-radii", "nfp_bias_forward", TWO_RADII, (F, F, F, F, F, 1 << 20, None), -2, "biased NFP: one radius per call"),
    ("bias-fwd-mixed", "nfp_bias_forward", MIXED, (F, F, F, F, F, 1 << 20, None), -2, "biased NFP: maps in the storage type"),
    ("bias-fwd-short-saved", "nfp_bias_forward", COS, (F, F, F, F, F, 1567, None), -1, "saved holds 1567 floats, nfp_bias_saved_floats is 1568"),
    ("bias-fwd-attention-no-saved", "nfp_bias_forward", ATT, (F, F, F, F, None, 5, None), -1, "saved holds 5 floats, nfp_bias_saved_floats is 784"),
    ("bias-fwd-null-x-and-unserved", "nfp_bias_forward", SCS, (None, F, F, F, F, 1568, None), -2, "biased NFP: measure 16"),
    ("bias-fwd-empty-null-neighbour", "nfp_bias_forward", COS0, (None, F, None, None, None, 0, None), -1, NULL),
    ("bias-fwd-empty-null", "nfp_bias_forward", COS0, (None, F, F, None, None, 0, None), 0, None),
    ("bias-fwd-empty-norm-no-centre", "nfp_bias_forward", NORM0, (None, None, F, None, None, 0, None), 0, None),
    # nfp_bias_backward(d, x, centre_bias, neighbour_bias, grad_out, out, saved, saved_floats, grad_x, grad_centre_bias,
    #                   grad_neighbour_bias, scratch, scratch_floats, stream)
    ("bias-bwd-null-gbeta", "nfp_bias_backward", COS, (F, F, F, F, F, F, 1568, F, F, None, F, 1 << 20, None), -1, NULL),
    ("bias-bwd-null-gx", "nfp_bias_backward", COS, (F, F, F, F, F, F, 1568, None, F, F, F, 1 << 20, None), -1, NULL),
    ("bias-bwd-unserved", "nfp_bias_backward", SCS, (F, F, F, F, F, F, 1568, F, F, F, F, 1 << 20, None), -2, "biased NFP: measure 16"),
    ("bias-bwd-short-saved", "nfp_bias_backward", COS, (F, F, F, F, F, F, 1567, F, F, F, F, 1 << 20, None), -1,
     "saved holds 1567 floats, nfp_bias_saved_floats is 1568"),
    ("bias-bwd-no-saved", "nfp_bias_backward", COS, (F, F, F, F, F, None, 1568, F, F, F, F, 1 << 20, None), -1,
     "saved holds 1568 floats, nfp_bias_saved_floats is 1568"),
    ("bias-bwd-short-scratch", "nfp_bias_backward", COS, (F, F, F, F, F, F, 1568, F, F, F, F, 1, None), -1,
     "scratch holds 1 floats, nfp_bias_scratch_floats is 2496"),
    ("bias-bwd-no-scratch", "nfp_bias_backward", COS, (F, F, F, F, F, F, 1568, F, F, F, None, 1 << 20, None), -1,
     "scratch holds 1048576 floats, nfp_bias_scratch_floats is 2496"),
    ("bias-bwd-short-saved-and-scratch", "nfp_bias_backward", COS, (F, F, F, F, F, F, 1567, F, F, F, F, 1, None), -1,
     "saved holds 1567 floats"),
    ("bias-bwd-null-gbeta-and-short-saved", "nfp_bias_backward", COS, (F, F, F, F, F, F, 1567, F, F, None, F, 1 << 20, None), -1, NULL),
    ("bias-bwd-empty-null-neighbour", "nfp_bias_backward", COS0, (None, F, None, None, None, None, 0, None, F, F, None, 0, None), -1, NULL),
    # the two calls beside them that take a descriptor and refuse: nfp_workspace_init(d, ws, stream), nfp_plan(d, backward, buf, len)
    ("ws-init-null", "nfp_workspace_init", COS, (None, None), -1, "workspace pointer must be non-null and 16-byte aligned"),
    ("ws-init-no-tables", "nfp_workspace_init", D(stride=2, ws=None), (F, None), -2, "this descriptor has no workspace tables"),
    ("plan-null-buffer", "nfp_plan", COS, (0, None, 0), -1, "null plan buffer"),
]


def run(lib, entry, dkw, args):
    """(return code, nfp_last_error(), launches) of one call"""
    dkw = dict(dkw)
    extra = {k: dkw.pop(k) for k in ("ws", "inner_R", "map_f32")}
    d = desc(**dkw)
    d.ws, d.inner_R, d.map_f32 = extra["ws"], extra["inner_R"], extra["map_f32"]
    n0 = lib.nfp_launch_count()
    rc = getattr(lib, entry)(ctypes.byref(d), *args)
    return rc, lib.nfp_last_error().decode(), lib.nfp_launch_count() - n0


def test_the_table_names_every_entry_and_case_once():
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids)
    entries = {c[1] for c in CASES}
    assert entries == {"nfp_%s%s" % (f, w) for f in ("", "pool_", "gap_", "valid_", "valid_abs_", "bias_")
                       for w in ("forward", "backward")} | {"nfp_workspace_init", "nfp_plan"}
    for e in entries - {"nfp_workspace_init", "nfp_plan"}:
        rows = [c for c in CASES if c[1] == e]
        assert any(c[5] == NULL for c in rows) and any(c[4] == -2 for c in rows), e           # a null pointer, an unserved measure
        assert any(c[2]["shape"][0] == 0 for c in rows), e                                        # an empty batch


@pytest.mark.parametrize("cid,entry,dkw,args,code,text", CASES, ids=[c[0] for c in CASES])
def test_refusal(lib, cid, entry, dkw, args, code, text):
    rc, err, launched = run(lib, entry, dkw, args)
    assert launched == 0
    assert rc == code, (rc, err)
    if text is not None:
        assert err.startswith(text), err
