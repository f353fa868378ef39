"""The projection of NFP maps that keeps the map on the MI355X (csrc/nfp_cpool.hip: the cproj kernels, include/nfp.h
nfp_cproj_*) against the float64 torch composition (conv2d, batch_norm, optional relu) of the same inputs under a random
grad_out [B,D,H,W]: the output and all four gradients, training and eval, with the ReLU and without.

Bars, of each tensor's max magnitude — the ones test_gpu_cpool.py states for the same formulas: 1e-5 for float32 — grad_w,
a difference of two larger sums, 5e-5; 1e-2 (out) and 2e-2 (gradients) for bf16 maps, against the reference on the
bf16-rounded maps (and grad_out, an input of the maps' dtype); 1e-4 on every tensor for maps of mean 10 and spread 0.1.

The ReLU mask: a pre-activation whose sign differs between float32 and float64 changes a gradient by a whole term, so
every case fixes a seed for which the float64 reference has min|a| >= 1e-5 max|a|, in training and in eval (and, for the
two bf16 cases, on the bf16-rounded maps too); the guard is asserted on the reference before anything is compared, and no
element is ever excluded.  The seeds were searched on the CPU: the first that passes.  The runs without the ReLU need no
guard."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

F32, F32_GW, BF_OUT, BF_GRAD, OFFSET = 1e-5, 5e-5, 1e-2, 2e-2, 1e-4
GUARD = 1e-5
EPS, MOM = 1e-5, 0.1

# name: (maps shape, D, seed, what it covers)
CASES = {
    "common": ((4, 8, 7, 7), 32, 2, "the common insert and bottleneck shape"),
    "n32_nonsquare": ((3, 32, 5, 7), 48, 0, "32 maps, non-square, D not a wavefront multiple"),
    "chunked": ((2, 32, 40, 40), 16, 38, "an image walked in chunks"),
    "one_pixel": ((5, 24, 1, 1), 16, 0, "P = 1"),
    "d_tiles": ((2, 8, 3, 3), 520, 2, "several D tiles and a ragged last one"),
    "one_image": ((1, 8, 7, 7), 32, 0, "B = 1"),
    "zero_row": ((4, 8, 7, 7), 32, 2, "an all-zero weight row: var = 0, a = beta"),
    "offset": ((4, 8, 7, 7), 32, 0, "maps = 10 + 0.1 randn"),
    "tiny_d": ((2, 8, 9, 9), 5, 0, "D smaller than any tile"),
    "n12": ((3, 12, 6, 5), 70, 1, "12 maps: the NP = 16 instantiations"),
}
BF16_CASES = ("common", "n32_nonsquare")


def make_inputs(name, seed=None):
    """maps [B,N,H,W], w [D,N,1,1], gamma, beta, running_mean, running_var [D], grad_out [B,D,H,W]: float32 CPU tensors."""
    shape, D, dflt, _ = CASES[name]
    seed = dflt if seed is None else seed
    g = torch.Generator().manual_seed(7919 * seed + sum(shape) + D)
    B, N = shape[:2]
    maps = torch.randn(*shape, generator=g)
    if name == "offset":
        maps = 10 + 0.1 * maps
    w = torch.randn(D, N, 1, 1, generator=g) * 0.5
    if name == "zero_row":
        w[3] = 0
    gamma = torch.rand(D, generator=g) + 0.5
    beta = torch.randn(D, generator=g) * 0.5
    rm = torch.randn(D, generator=g) * 0.3
    if name == "offset":
        rm = rm + 10 * w.reshape(D, N).sum(1)      # (near the conv output's mean, as a trained BatchNorm's would be)
    rv = torch.rand(D, generator=g) + 0.5
    go = torch.randn(B, D, *shape[2:], generator=g)
    return maps, w, gamma, beta, rm, rv, go


def reference64(ins, training, relu, dtype=torch.float32):
    """dict(out, gm, gw, gg, gb, rm, rv, guard) of the float64 composition on `ins` (maps and grad_out rounded to dtype)."""
    maps, w, gamma, beta, rm, rv, go = ins
    m, w_, ga, be = (t.double().requires_grad_(True) for t in (maps.to(dtype), w, gamma, beta))
    rm, rv = rm.double().clone(), rv.double().clone()
    a = F.batch_norm(F.conv2d(m, w_), rm, rv, ga, be, training, MOM, EPS)
    out = F.relu(a) if relu else a
    gm, gw, gg, gb = torch.autograd.grad(out, (m, w_, ga, be), go.to(dtype).double())
    aa = a.detach().abs()
    return dict(out=out.detach(), gm=gm, gw=gw, gg=gg, gb=gb, rm=rm, rv=rv, guard=float(aa.min() / aa.max()))


@functools.lru_cache(maxsize=None)
def case_ref(name, training, relu=True, bf16=False):
    """(inputs, float64 reference) of a case — computed once, shared by the tests, never modified."""
    ins = make_inputs(name)
    return ins, reference64(ins, training, relu, torch.bfloat16 if bf16 else torch.float32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from neighbour_feature_pooling_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _hip_wherever_it_can_serve(monkeypatch):
    """NFP_CPROJ_TORCH=0: the kernels are tested for everything they serve, whatever the default routing takes."""
    monkeypatch.setenv("NFP_CPROJ_TORCH", "0")


def _lib():
    from neighbour_feature_pooling_amd import _abi
    return _abi.load()


def _count():
    return _lib().nfp_launch_count()


def run_hip(ins, training, dev, relu=True, dtype=torch.float32, want=(True, True, True, True), inplace=None):
    """dict(out, gm, gw, gg, gb, rm, rv, fwd, bwd) of nfp_compress_map_tensors on the device: None for a gradient not asked
    for; fwd / bwd the launch-counter deltas.  inplace: "relu" / "add" — the output modified in place before the backward
    (`out` is then the copy taken before that)."""
    from neighbour_feature_pooling_amd import nfp_compress_map_tensors
    maps, w, gamma, beta, rm, rv, go = ins
    t = [x.to(dev) for x in (maps.to(dtype), w, gamma, beta)]
    t = [x.requires_grad_(r) for x, r in zip(t, want)]
    rm, rv = rm.clone().to(dev), rv.clone().to(dev)
    n0 = _count()
    out = nfp_compress_map_tensors(t[0], t[1], t[2], t[3], rm, rv, training, MOM, EPS, relu)
    n1 = _count()
    kept = out.detach().clone()
    if inplace == "relu":
        out.relu_()
    elif inplace == "add":
        out += 1
    asked = [x for x in t if x.requires_grad]
    grads = iter(torch.autograd.grad(out, asked, go.to(dev).to(out.dtype)) if asked else ())
    torch.cuda.synchronize()
    n2 = _count()
    res = dict(zip(("gm", "gw", "gg", "gb"), (next(grads) if r else None for r in want)))
    res.update(out=kept, rm=rm, rv=rv, fwd=n1 - n0, bwd=n2 - n1)
    return res


def _np(t):
    return t.detach().double().cpu().numpy()


def errors(got, ref):
    e = {k: rel_err(_np(got[k]).reshape(-1), _np(ref[k]).reshape(-1)) for k in ("out", "gm", "gw", "gg", "gb")}
    e["guard"] = ref["guard"]
    return e


MODES = [pytest.param(True, id="train"), pytest.param(False, id="eval")]
RELU = [pytest.param(True, id="relu"), pytest.param(False, id="lin")]


def _variant(which, dtype, training, relu):
    return f"cproj_{which}<{dtype},{'train' if training else 'eval'},{'relu' if relu else 'lin'}>"


@pytest.mark.parametrize("relu", RELU)
@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("name", [n for n in CASES if n != "offset"])
def test_float32_matches_the_float64_composition(name, training, relu, dev):
    ins, ref = case_ref(name, training, relu)
    assert not relu or ref["guard"] >= GUARD, ref["guard"]
    got = run_hip(ins, training, dev, relu)
    e = errors(got, ref)
    print(name, "train" if training else "eval", "relu" if relu else "lin", e, got["fwd"], got["bwd"])
    B, D = ins[0].shape[0], ins[1].shape[0]
    assert got["out"].dtype == torch.float32 and got["out"].shape == (B, D) + ins[0].shape[2:]
    assert got["gm"].shape == ins[0].shape and got["gw"].shape == ins[1].shape
    for k in ("out", "gm", "gg", "gb"):
        assert e[k] <= F32, (k, e[k])
    assert e["gw"] <= F32_GW, e["gw"]
    assert got["fwd"] == (3 if training else 1) and got["bwd"] == 3
    assert _lib().nfp_last_variant().decode() == _variant("bwd", "f32", training, relu)
    if name == "zero_row" and training:
        b3 = ins[3][3]                                      # var = 0: a = beta, whatever the maps
        want = (torch.relu(b3) if relu else b3).expand(4, 7, 7)
        assert torch.allclose(got["out"][:, 3].cpu(), want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("relu", RELU)
@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("name", BF16_CASES)
def test_bf16_maps(name, training, relu, dev):
    ins, ref = case_ref(name, training, relu, True)
    assert not relu or ref["guard"] >= GUARD, ref["guard"]
    got = run_hip(ins, training, dev, relu, torch.bfloat16)
    e = errors(got, ref)
    print(name, "train" if training else "eval", "relu" if relu else "lin", e)
    assert got["out"].dtype == torch.bfloat16 and got["gm"].dtype == torch.bfloat16 and got["gw"].dtype == torch.float32
    assert e["out"] <= BF_OUT
    for k in ("gm", "gw", "gg", "gb"):
        assert e[k] <= BF_GRAD, (k, e[k])
    assert _lib().nfp_last_variant().decode() == _variant("bwd", "bf16", training, relu)


@pytest.mark.parametrize("relu", RELU)
@pytest.mark.parametrize("training", MODES)
def test_offset_maps(training, relu, dev):
    """Maps of mean 10 and spread 0.1: the second moments must be taken centred."""
    ins, ref = case_ref("offset", training, relu)
    assert not relu or ref["guard"] >= GUARD, ref["guard"]
    got = run_hip(ins, training, dev, relu)
    e = errors(got, ref)
    print("offset", "train" if training else "eval", "relu" if relu else "lin", e)
    for k in ("out", "gm", "gw", "gg", "gb"):
        assert e[k] <= OFFSET, (k, e[k])


def test_the_forward_names_its_variant_and_counts_its_launches(dev):
    for training in (True, False):
        for relu in (True, False):
            ins, _ = case_ref("common", training, relu)
            got = run_hip(ins, training, dev, relu, want=(False,) * 4)
            assert got["fwd"] == (3 if training else 1) and got["bwd"] == 0
            assert _lib().nfp_last_variant().decode() == _variant("fwd", "f32", training, relu)


def test_running_statistics_and_num_batches_tracked(dev):
    from neighbour_feature_pooling_amd import nfp_compress_map
    for name in ("common", "chunked", "offset"):
        ins, ref = case_ref(name, True)
        got = run_hip(ins, True, dev)
        e = dict(rm=rel_err(_np(got["rm"]), _np(ref["rm"])), rv=rel_err(_np(got["rv"]), _np(ref["rv"])))
        print(name, e)
        assert e["rm"] <= F32 and e["rv"] <= F32
        assert not torch.equal(got["rm"].cpu(), ins[4])
        ins, ref = case_ref(name, False)
        got = run_hip(ins, False, dev)
        assert torch.equal(got["rm"].cpu(), ins[4]) and torch.equal(got["rv"].cpu(), ins[5])       # eval leaves them
    # the module form against nn.BatchNorm2d itself: its own buffers, its counter bumped on the Python side
    ins, ref = case_ref("common", True)
    bn = torch.nn.BatchNorm2d(32, eps=EPS, momentum=MOM).to(dev)
    with torch.no_grad():
        bn.weight.copy_(ins[2]), bn.bias.copy_(ins[3]), bn.running_mean.copy_(ins[4]), bn.running_var.copy_(ins[5])
    twin = torch.nn.BatchNorm2d(32, eps=EPS, momentum=MOM).to(dev).double()
    twin.load_state_dict(bn.state_dict())
    maps, w = ins[0].to(dev), ins[1].to(dev)
    for step in (1, 2):
        n0 = _count()
        out = nfp_compress_map(maps, w, bn)
        assert _count() - n0 == 3
        want = F.relu(twin(F.conv2d(maps.double(), w.double())))
        assert int(bn.num_batches_tracked) == step == int(twin.num_batches_tracked)
        assert rel_err(_np(out), _np(want)) <= F32
        assert rel_err(_np(bn.running_mean), _np(twin.running_mean)) <= F32
        assert rel_err(_np(bn.running_var), _np(twin.running_var)) <= F32
    bn.eval(), twin.eval()
    n0 = _count()
    out = nfp_compress_map(maps, w, bn, relu=False)
    assert _count() - n0 == 1 and int(bn.num_batches_tracked) == 2
    assert rel_err(_np(out), _np(twin(F.conv2d(maps.double(), w.double())))) <= F32
    # track_running_stats=False: batch statistics in both modes, nothing to update
    bn2 = torch.nn.BatchNorm2d(32, eps=EPS, momentum=MOM, track_running_stats=False).to(dev).eval()
    with torch.no_grad():
        bn2.weight.copy_(ins[2]), bn2.bias.copy_(ins[3])
    n0 = _count()
    out = nfp_compress_map(maps, w, bn2)
    assert _count() - n0 == 3 and rel_err(_np(out), _np(ref["out"])) <= F32


@pytest.mark.parametrize("relu", RELU)
@pytest.mark.parametrize("training", MODES)
def test_each_gradient_switched_off_in_turn(training, relu, dev):
    ins, _ = case_ref("n32_nonsquare", training, relu)
    full = run_hip(ins, training, dev, relu)
    keys = ("gm", "gw", "gg", "gb")
    for off in range(4):
        want = tuple(i != off for i in range(4))
        got = run_hip(ins, training, dev, relu, want=want)
        assert got[keys[off]] is None
        for i, k in enumerate(keys):
            if i != off:
                assert torch.equal(got[k], full[k]), (keys[off], k)
        assert got["bwd"] == (2 if off == 0 else 3)       # without grad_maps its kernel is skipped
    # the maps alone: in eval no batch sum is needed — one launch
    got = run_hip(ins, training, dev, relu, want=(True, False, False, False))
    assert torch.equal(got["gm"], full["gm"]) and got["bwd"] == (3 if training else 1)
    # nothing asked for: no saved state, no backward
    got = run_hip(ins, training, dev, relu, want=(False,) * 4)
    assert torch.equal(got["out"], full["out"]) and got["bwd"] == 0


@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("name", ["common", "chunked", "d_tiles"])
def test_two_runs_agree_bitwise(name, training, dev):
    ins, _ = case_ref(name, training)
    a, b = run_hip(ins, training, dev), run_hip(ins, training, dev)
    for k in ("out", "gm", "gw", "gg", "gb", "rm", "rv"):
        assert torch.equal(a[k], b[k]), k


def test_eval_rows_do_not_depend_on_the_batch(dev):
    ins, _ = case_ref("n32_nonsquare", False)
    full = run_hip(ins, False, dev)
    part = run_hip(tuple(t[:2] if i in (0, 6) else t for i, t in enumerate(ins)), False, dev)
    assert torch.equal(part["out"], full["out"][:2]) and torch.equal(part["gm"], full["gm"][:2])


@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("relu,inplace", [(True, "relu"), (True, "add"), (False, "add")])
def test_the_backward_does_not_read_the_output(relu, inplace, training, dev):
    """ReLU(inplace=True) behind the op, `out += identity` in the bottleneck: the output is the caller's to overwrite."""
    ins, ref = case_ref("common", training, relu)
    plain = run_hip(ins, training, dev, relu)
    got = run_hip(ins, training, dev, relu, inplace=inplace)
    assert torch.equal(got["out"], plain["out"])
    for k in ("gm", "gw", "gg", "gb"):                      # (relu_ of a ReLU's output and + 1 leave the gradient as it is)
        assert torch.equal(got[k], plain[k]), k
    e = errors(got, ref)
    for k in ("gm", "gg", "gb"):
        assert e[k] <= F32, (k, e[k])
    assert e["gw"] <= F32_GW


def test_empty_batch(dev):
    from neighbour_feature_pooling_amd import nfp_compress_map_tensors
    L = _lib()
    p = torch.zeros(2048, device=dev).data_ptr()
    n0 = _count()
    assert L.nfp_cproj_forward(0, 8, 49, 32, 0, 1, 1, None, p, p, p, p, p, MOM, EPS, None, p, 112, None, 0, None) == 0
    assert L.nfp_cproj_backward(0, 8, 49, 32, 0, 1, 1, None, p, p, p, None, None, EPS, p, 112, None, None, p, p, p, None, 0,
                                None) == 0
    assert _count() == n0
    ins = make_inputs("common")
    out = nfp_compress_map_tensors(ins[0][:0].to(dev), *(t.to(dev) for t in ins[1:6]), False)
    assert out.shape == (0, 32, 7, 7) and _count() == n0


def test_the_switch_and_the_unserved_calls_take_the_composition(dev, monkeypatch):
    from neighbour_feature_pooling_amd import functional, nfp_compress_map_tensors
    from neighbour_feature_pooling_amd._host import compress_map_host
    ins, ref = case_ref("common", True)
    d = [t.to(dev) for t in ins]

    def call(maps, params=d[1:4], dtype=None, relu=True):
        cast = (lambda t: t) if dtype is None else (lambda t: None if t is None else t.to(dtype))
        args = [cast(t) for t in params] + [cast(d[4].clone()), cast(d[5].clone())]
        n0 = _count()
        out = nfp_compress_map_tensors(maps, *args, True, MOM, EPS, relu)
        want = compress_map_host(maps, *[cast(t) for t in params], cast(d[4].clone()), cast(d[5].clone()), True, MOM, EPS, relu)
        return out, want, _count() - n0

    out, want, k = call(d[0])
    assert k == 3 and rel_err(_np(out), _np(want)) <= 1e-4
    monkeypatch.setenv("NFP_CPROJ_TORCH", "1")          # the A/B switch, read at call time
    for relu in (True, False):
        out, want, k = call(d[0], relu=relu)
        assert k == 0 and torch.equal(out, want)
    monkeypatch.delenv("NFP_CPROJ_TORCH")               # the default routing: what DESIGN 4g's table shows faster
    assert call(d[0])[2] == 0                           # a train-mode step below CPROJ_ROUTED_TRAIN_PIXELS: the composition
    assert d[0].shape[0] * 49 < functional.CPROJ_ROUTED_TRAIN_PIXELS
    n0 = _count()
    with torch.no_grad():                               # the forward on running statistics, no backward: the HIP kernel
        out = nfp_compress_map_tensors(d[0], d[1], d[2], d[3], d[4].clone(), d[5].clone(), False, MOM, EPS)
    assert _count() - n0 == 1 and _lib().nfp_last_variant().decode() == "cproj_fwd<f32,eval,relu>"
    big = torch.randn(64, 8, 54, 54, device=dev)        # the smallest train-mode class that measured faster
    n0 = _count()
    nfp_compress_map_tensors(big, d[1], d[2], d[3], d[4].clone(), d[5].clone(), True, MOM, EPS)
    assert _count() - n0 == 3
    monkeypatch.setenv("NFP_CPROJ_TORCH", "0")
    assert call(d[0])[2] == 3
    strided = torch.randn(4, 8, 7, 14, device=dev)[..., ::2]
    for maps, dtype in ((strided, None), (d[0].half(), torch.float16), (d[0].double(), torch.float64)):
        out, want, k = call(maps, dtype=dtype)
        assert k == 0 and torch.equal(out, want) and out.dtype == maps.dtype
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out, want, k = call(d[0])
    assert k == 0 and torch.equal(out, want)
    out, want, k = call(d[0], params=[d[1], None, None])          # affine=False
    assert k == 0 and torch.equal(out, want)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        call(d[0][:1, :, :1, :1].contiguous())


def test_short_null_and_negative_arguments_are_invalid_without_a_launch(dev):
    """Every refusal comes before any HIP call: the launch counter stands still.  (No call here could launch: each has the
    one defect it is about, and the well-formed call is the other tests'.)"""
    L = _lib()
    INVALID, UNSUPPORTED = -1, -2
    B, N, P, D = 4, 8, 49, 32
    buf = torch.zeros(1 << 16, device=dev)
    p = buf.data_ptr()
    ns = int(L.nfp_cpool_saved_floats(N, D))
    nf, nb = int(L.nfp_cproj_scratch_floats(B, N, P, D, 0)), int(L.nfp_cproj_scratch_floats(B, N, P, D, 1))
    assert ns == 2 * N + N * N + D and nf > 1 and nb > 1 and max(ns, nf, nb) < buf.numel()

    def fwd(B=B, N=N, P=P, D=D, dtype=0, training=1, relu=1, maps=p, w=p, gamma=p, beta=p, rm=p, rv=p, mom=MOM, eps=EPS, out=p,
            saved=p, ns=ns, scratch=p, nscr=nf):
        return L.nfp_cproj_forward(B, N, P, D, dtype, training, relu, maps, w, gamma, beta, rm, rv, mom, eps, out, saved, ns,
                                   scratch, nscr, None)

    def bwd(B=B, N=N, P=P, D=D, dtype=0, training=1, relu=1, maps=p, w=p, gamma=p, beta=p, rm=None, rv=None, eps=EPS, saved=p,
            ns=ns, go=p, gm=p, gw=p, gg=p, gb=p, scratch=p, nscr=nb):
        return L.nfp_cproj_backward(B, N, P, D, dtype, training, relu, maps, w, gamma, beta, rm, rv, eps, saved, ns, go, gm, gw,
                                    gg, gb, scratch, nscr, None)

    n0 = _count()
    for kw in (dict(B=-1), dict(N=0), dict(P=0), dict(D=0), dict(dtype=2), dict(eps=-1.0), dict(mom=float("nan")),
               dict(maps=None), dict(w=None), dict(gamma=None), dict(beta=None), dict(out=None), dict(rm=None),
               dict(training=0, rm=None, rv=None), dict(saved=None), dict(ns=ns - 1), dict(scratch=None), dict(nscr=nf - 1)):
        assert fwd(**kw) == INVALID, kw
        assert b"nfp_cproj_forward" in L.nfp_last_error()
    for kw in (dict(B=-1), dict(N=0), dict(P=0), dict(D=0), dict(dtype=2), dict(eps=-1.0), dict(maps=None), dict(w=None),
               dict(gamma=None), dict(beta=None), dict(go=None), dict(training=0), dict(saved=None), dict(ns=ns - 1),
               dict(scratch=None), dict(nscr=nb - 1), dict(training=0, rm=p, rv=p, gm=None, scratch=None, nscr=0)):
        assert bwd(**kw) == INVALID, kw
        assert b"nfp_cproj_backward" in L.nfp_last_error()
    for kw in (dict(N=33), dict(P=2 ** 28), dict(N=1, P=2 ** 27), dict(D=2 ** 22 + 1), dict(B=1, P=1)):
        assert fwd(**kw) == UNSUPPORTED, kw                 # N > 32; N * P and D * P at 2^31; D > 2^22; B * P = 1 in training
        assert bwd(**kw) == UNSUPPORTED, kw
    assert bwd(gm=None, gw=None, gg=None, gb=None) == 0     # nothing asked for: nothing to do
    assert _count() == n0
