"""Poisoned and fenced buffers for the binding's allocations — a helper module, not a conftest.

Every output, gradient, `saved`, scratch, record and workspace buffer the binding (functional.py, compress.py, the device
branches of _ops.py) hands the library comes from `torch.empty` / `torch.empty_like`: a kernel must write every element of
every buffer it owns, and must never let a value it did not write reach a result ("Caller-allocated buffers").
The caching allocator hides a violation of either: a repeated case gets back the block the previous call just filled with
the right answer.  Inside

    with Poison("nan") as poison:
        x = poison.fenced(x0)
        ...                      # forward, backward
        poison.check()

the name `torch` in those three modules is a proxy whose `empty` / `empty_like` carve each tensor out of a flat uint8
buffer of its own — GUARD bytes of a fixed pattern, the tensor, GUARD bytes — and fill the tensor with the run's poison;
everything else of `torch` passes through, and outside the context nothing is replaced.  The tensor is an ordinary one set
onto the flat buffer's storage (`set_`, no view), with the shape, dtype, device and strides of the unpatched call, at an
address that is a multiple of 512 — the caching allocator's own alignment, so the dispatcher picks the same kernels.

Fills: floating buffers get "zero", "nan" (a quiet NaN) or "big" (+-3e38 alternating: fmaxf, ReLU and `>` swallow a NaN);
integer, bool and uint8 buffers — the workspace tables of functional._workspace — get zeros in every run, so nothing a
kernel may use as an index, an offset or a counter ever holds a wild pattern.  A tensor without an element is the unpatched
call's (no bytes to poison or fence; its NULL data pointer is part of the binding's contract).

`fenced(t)` is a copy of an input inside the same kind of buffer: same sizes, strides and address modulo 512; for a view
with gaps (a class token in front of every image, a batch stride) the gaps are poisoned too.

`check()` synchronises and asserts that every guard byte of every buffer made inside the context is untouched, naming the
buffer by the file and line that asked for it and the first and last changed offset, and that the seam served at least one
allocation.  `run_fills` / `assert_same_bits` are the assertion every case of tests/test_gpu_poison.py makes.
"""
import os
import sys

import torch

GUARD = 512                 # bytes before and after every buffer: the caching allocator's alignment
GUARD_BYTE = 0x7F           # float32 0x7F7F7F7F = 3.39e38, bf16 0x7F7F = 3.39e38, float64 1.4e306: huge and finite in every type
FILLS = ("zero", "nan", "big")
BIG = 3e38

_HERE = os.path.abspath(__file__)


def binding_modules():
    """The modules whose `torch` the context replaces: the binding's three."""
    from neighbour_feature_pooling_amd import _ops, compress, functional
    return [functional, compress, _ops]


def _extent(size, stride):
    """Elements from a tensor's first to one past its last (non-negative strides); 0 for a tensor without an element."""
    if any(n == 0 for n in size):
        return 0
    return 1 + sum((n - 1) * s for n, s in zip(size, stride))


def _caller():
    """file:line of the first frame outside this module."""
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    return "?" if f is None else "%s:%d" % (os.path.basename(f.f_code.co_filename), f.f_lineno)


class _Buffer:
    """One flat uint8 buffer: [0, lo) guard, [lo, hi) the tensor's bytes, [hi, end) guard."""
    __slots__ = ("flat", "lo", "hi", "site", "what")

    def __init__(self, flat, lo, hi, site, what):
        self.flat, self.lo, self.hi, self.site, self.what = flat, lo, hi, site, what

    def damage(self):
        """None, or (first, last) changed guard byte as offsets from the tensor's first byte (negative: in front of it;
        >= its length: behind it)."""
        bad = []
        for a, b in ((0, self.lo), (self.hi, self.flat.numel())):
            idx = (self.flat[a:b] != GUARD_BYTE).nonzero()
            if idx.numel():
                bad += [a + int(idx[0]) - self.lo, a + int(idx[-1]) - self.lo]
        return (min(bad), max(bad)) if bad else None


class _TorchProxy:
    """`torch` with `empty` and `empty_like` replaced; every other attribute is torch's own."""

    def __init__(self, poison):
        self._poison = poison

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, **kwargs):
        return self._poison._allocate(torch.empty, args, kwargs)

    def empty_like(self, *args, **kwargs):
        return self._poison._allocate(torch.empty_like, args, kwargs)


class Poison:
    def __init__(self, fill, modules=None):
        assert fill in FILLS, fill
        self.fill = fill
        self.modules = modules
        self.buffers = []
        self.served = 0
        self._saved = []

    # ---- the seam ---------------------------------------------------------------------------------------------------
    def __enter__(self):
        proxy = _TorchProxy(self)
        for m in (binding_modules() if self.modules is None else self.modules):
            assert getattr(m, "torch", None) is torch, "%s does not reach its allocations by the name `torch`" % m.__name__
            self._saved.append(m)
            m.torch = proxy
        return self

    def __exit__(self, *exc):
        for m in self._saved:
            m.torch = torch
        self._saved = []
        return False

    # ---- one guarded buffer --------------------------------------------------------------------------------------------
    def _carve(self, size, stride, dtype, device, lead, site, what):
        """A tensor of (size, stride, dtype) on `device` whose first element lies `lead` bytes (< 512) into the poisoned
        interior of a new guarded buffer, at an address of `lead` modulo 512."""
        item = dtype.itemsize
        assert lead % item == 0 and 0 <= lead < GUARD
        nbytes = lead + _extent(size, stride) * item
        flat = torch.empty(3 * GUARD + nbytes, dtype=torch.uint8, device=device)
        lo = GUARD + (-(flat.data_ptr() + GUARD)) % GUARD       # (the allocator's blocks are 512-aligned on the GPU: lo = GUARD)
        flat.fill_(GUARD_BYTE)
        store = flat.untyped_storage()
        off = flat.storage_offset() + lo
        assert off % item == 0
        interior = torch.empty(0, dtype=dtype, device=device).set_(store, off // item, (nbytes // item,), (1,))
        self._fill(interior)
        t = torch.empty(0, dtype=dtype, device=device).set_(store, (off + lead) // item, tuple(size), tuple(stride))
        assert t.data_ptr() % GUARD == lead
        self.buffers.append(_Buffer(flat, lo, lo + nbytes, site, what))
        return t

    def _fill(self, interior):
        if not interior.dtype.is_floating_point or self.fill == "zero":
            interior.zero_()        # integer, bool, uint8: zeros in every run — never a wild index, offset or counter
        elif self.fill == "nan":
            interior.fill_(float("nan"))
        else:
            big = min(BIG, torch.finfo(interior.dtype).max)
            interior.fill_(big)
            interior[1::2] = -big

    def _allocate(self, real, args, kwargs):
        if torch.compiler.is_compiling():
            return real(*args, **kwargs)
        self.served += 1
        meta = real(*args, **dict(kwargs, device="meta"))      # shape, dtype and strides of the unpatched call
        if meta.numel() == 0:
            return real(*args, **kwargs)       # (no bytes to poison or fence; its NULL data pointer is the binding's contract)
        device = kwargs.get("device")
        if device is None:
            device = args[0].device if real is torch.empty_like else torch.get_default_device()
        return self._carve(meta.shape, meta.stride(), meta.dtype, torch.device(device), 0, _caller(), real.__name__)

    # ---- inputs ---------------------------------------------------------------------------------------------------------
    def fenced(self, t):
        """A detached copy of `t` inside a guarded buffer: the same sizes, strides and address modulo 512; what lies
        between its elements (a class token, a batch stride's gap) is poisoned."""
        if t.numel() == 0:
            return t.detach().clone()
        lead = t.data_ptr() % GUARD
        c = self._carve(t.shape, t.stride(), t.dtype, t.device, lead - lead % t.element_size(), _caller(), "fenced")
        c.copy_(t.detach())
        return c

    # ---- the assertion ---------------------------------------------------------------------------------------------------
    def check(self):
        if any(b.flat.is_cuda for b in self.buffers):
            torch.cuda.synchronize()
        assert self.served > 0, "the harness served no allocation: the binding no longer allocates through `torch.empty`"
        for b in self.buffers:
            d = b.damage()
            assert d is None, ("%s buffer of %s (%d bytes, fill %r): guard bytes changed, first at offset %d, last at %d"
                               % (b.what, b.site, b.hi - b.lo, self.fill, d[0], d[1]))


def raw(t):
    """The bytes of a tensor (on the CPU, dense) — bf16 as int16 — or None."""
    if t is None:
        return None
    t = t.detach().cpu().contiguous()
    t = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
    return t.numpy().tobytes()


def assert_same_bits(runs, what=""):
    """`runs`: {fill: {name: tensor or None or str}} — every entry equal across the fills, tensors bit for bit."""
    fills = list(runs)
    base = runs[fills[0]]
    for f in fills[1:]:
        assert set(runs[f]) == set(base), (what, f, sorted(runs[f]), sorted(base))
        for name, a in base.items():
            b = runs[f][name]
            if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
                assert isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor), (what, name, fills[0], f)
                assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
                ra, rb = raw(a), raw(b)
                if ra != rb:
                    n = sum(x != y for x, y in zip(ra, rb))
                    first = next(i for i, (x, y) in enumerate(zip(ra, rb)) if x != y)
                    raise AssertionError("%s: %s differs between fill %r and fill %r in %d of %d bytes, first at byte %d"
                                         % (what, name, fills[0], f, n, len(ra), first))
            else:
                assert a == b, (what, name, fills[0], a, f, b)


def run_fills(case, what="", modules=None):
    """The one assertion of every case.  `case(poison)` runs forward and backward once on fresh inputs (each
    `poison.fenced`) and returns {name: tensor / None / str}: every tensor the caller can see — outputs, every gradient
    asked for, the running statistics — and the names of the kernels that served.  It is run once per fill; `check()` must
    pass in each run and every entry must be the same in all of them, tensors bit for bit.  Returns the "zero" run."""
    runs = {}
    for fill in FILLS:
        with Poison(fill, modules) as poison:
            runs[fill] = case(poison)
            poison.check()
    assert_same_bits(runs, what)
    return runs["zero"]
