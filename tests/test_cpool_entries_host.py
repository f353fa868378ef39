"""The eight entries of the compress-BN family that serve one rank's call (nfp_cpool_forward / _backward, their
nfp_cpool_wide_* forms, nfp_cproj_forward / _backward and their _fmt forms) share one host path: every refusal carries the
code include/nfp.h documents, the name of the entry that was called at the head of its message and, for a short scratch, the
length query of that entry's kind.  All of it is checked before any HIP call: the pointers are never dereferenced and the
launch counter stands still.  No GPU needed."""
import pytest

from neighbour_feature_pooling_amd import _abi

INVALID, UNSUPPORTED = -1, -2
MOM, EPS = 0.1, 1e-5
SIZES = dict(B=4, N=8, P=49, D=32)
PTR = 0x1000      # (never dereferenced)

# entry -> (kind, direction, takes a layout)
ENTRIES = {
    "nfp_cpool_forward": ("cpool", "fwd", False),
    "nfp_cpool_backward": ("cpool", "bwd", False),
    "nfp_cproj_forward": ("cproj", "fwd", False),
    "nfp_cproj_backward": ("cproj", "bwd", False),
    "nfp_cproj_forward_fmt": ("cproj", "fwd", True),
    "nfp_cproj_backward_fmt": ("cproj", "bwd", True),
    "nfp_cpool_wide_forward": ("cpool_wide", "fwd", False),
    "nfp_cpool_wide_backward": ("cpool_wide", "bwd", False),
}

# what every entry refuses, with its code; `short` names the buffer given one float less than its length query asks for
CASES = [
    ("N = 0", dict(N=0), INVALID),
    ("P = 0", dict(P=0), INVALID),
    ("D = 0", dict(D=0), INVALID),
    ("B = -1", dict(B=-1), INVALID),
    ("N = 33", dict(N=33), UNSUPPORTED),
    ("dtype = 2", dict(dtype=2), INVALID),
    ("NULL w", dict(w=None), INVALID),
    ("short saved", dict(short="saved"), INVALID),
    ("short scratch", dict(short="scratch"), INVALID),
    ("layout = 2", dict(layout=2), INVALID),
]
# the wide kernels take up to 96 maps: the same refusals, with 97 maps where the others refuse 33
WIDE_CASES = [("N = 97", dict(N=97), UNSUPPORTED) if case[0] == "N = 33" else case for case in CASES]


@pytest.fixture(scope="module")
def lib():
    from neighbour_feature_pooling_amd.build import build_hip
    build_hip()
    return _abi.load()


def _call(L, name, B, N, P, D, dtype=0, training=1, w=PTR, short=None, layout=0):
    kind, direction, fmt = ENTRIES[name]
    ns = int(L.nfp_cpool_saved_floats(N, D)) - (short == "saved")
    nscr = int(getattr(L, f"nfp_{kind}_scratch_floats")(B, N, P, D, direction == "bwd")) - (short == "scratch")
    p = PTR
    args = [B, N, P, D, dtype, training] + ([1] if kind == "cproj" else [])
    if direction == "fwd":      # maps, w, gamma, beta, rm, rv, momentum, eps, out, saved, its length, scratch, its length
        args += [p, w, p, p, p, p, MOM, EPS, p, p, ns, p, nscr, None]
    else:                       # maps .. beta, rm, rv, eps, saved, its length, grad_out, four gradients, scratch, its length
        args += [p, w, p, p, None, None, EPS, p, ns, p, p, p, p, p, p, nscr, None]
    return getattr(L, name)(*args, *([layout] if fmt else []))


@pytest.mark.parametrize("name,label,kw,code", [(name, *case) for name, (kind, _, fmt) in ENTRIES.items()
                                                for case in (WIDE_CASES if kind == "cpool_wide" else CASES)
                                                if fmt or "layout" not in case[1]],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_every_entry_refuses_under_its_own_name(lib, name, label, kw, code):
    L = lib
    kind = ENTRIES[name][0]
    n0 = L.nfp_launch_count()
    assert _call(L, name, **{**SIZES, **kw}) == code
    err = L.nfp_last_error()
    assert err.startswith(name.encode() + b":"), err
    if kw.get("short") == "scratch":    # the length query of this entry's kind, and no other, is the one named
        assert f"nfp_{kind}_scratch_floats is".encode() in err, err
    if kw.get("short") == "saved":
        assert b"nfp_cpool_saved_floats is" in err, err
    assert L.nfp_launch_count() == n0


@pytest.mark.parametrize("name", [n for n in ENTRIES if n.endswith("backward") or n.endswith("backward_fmt")])
def test_a_backward_checks_the_scratch_length_of_its_own_kind(lib, name):
    """At 196 pixels the two kinds ask for different lengths (cproj slices the batch by 64-pixel passes, cpool and its wide
    form by images): each backward takes exactly its own and refuses one float less."""
    L = lib
    B, N, P, D = 4, 8, 196, 32
    pool, proj = L.nfp_cpool_scratch_floats(B, N, P, D, 1), L.nfp_cproj_scratch_floats(B, N, P, D, 1)
    assert (pool, proj) == (4 * D * (N + 1) + (N + N * N), 16 * D * (N + 1) + (N + N * N))
    n0 = L.nfp_launch_count()
    assert _call(L, name, B, N, P, D, short="scratch") == INVALID
    want = {"cproj": proj, "cpool": pool, "cpool_wide": L.nfp_cpool_wide_scratch_floats(B, N, P, D, 1)}[ENTRIES[name][0]]
    assert f"scratch holds {want - 1} floats".encode() in L.nfp_last_error() and f"is {want}".encode() in L.nfp_last_error()
    assert L.nfp_launch_count() == n0
