"""The poison harness itself (tests/poison.py) on CPU tensors: three small stand-ins for a bad kernel — one that leaves the
last element unwritten, one that adds 0 * (an unwritten element) into a result, one that writes one element past the end —
must each be caught by the assertion every GPU case makes (`run_fills`), and a correct stand-in must pass; a patched
allocation has the layout, strides, dtype and alignment of the unpatched one."""
import sys

import pytest
import torch

import poison as P

ME = sys.modules[__name__]      # the "binding" of this file: the stand-ins below reach their buffers by its name `torch`
REAL = torch                    # ... which is the proxy inside a context, in this file's own code too


def _kernel_good(x):
    out = torch.empty_like(x)
    scratch = torch.empty(x.numel() + 3, dtype=torch.float32)
    scratch[:x.numel()] = x.reshape(-1).float() * 2         # (the 3 spare floats: never written, never read)
    out.reshape(-1)[:] = scratch[:x.numel()].to(x.dtype)
    return out


def _kernel_skips_last(x):
    out = torch.empty_like(x)
    out.reshape(-1)[:-1] = x.reshape(-1)[:-1] * 2
    return out


def _kernel_zero_times_unwritten(x):
    out = torch.empty_like(x)
    scratch = torch.empty(4, dtype=torch.float32)
    out.reshape(-1)[:] = (x.reshape(-1).float() * 2 + 0 * scratch[1]).to(x.dtype)
    return out


def _kernel_writes_past_the_end(x):
    out = torch.empty_like(x)
    flat = torch.as_strided(out, (out.numel() + 1,), (1,))      # (inside the harness's flat buffer: the guard behind `out`)
    flat[:-1] = x.reshape(-1) * 2
    flat[-1] = 1
    return out


def _case(kernel, dtype):
    x0 = (torch.arange(24, dtype=torch.float32).reshape(2, 3, 4) / 7 - 1).to(dtype)

    def case(poison):
        return dict(out=kernel(poison.fenced(x0)), variant=kernel.__name__)
    return case, x0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64], ids=str)
def test_a_correct_kernel_passes(dtype):
    case, x0 = _case(_kernel_good, dtype)
    res = P.run_fills(case, "good", modules=[ME])
    assert torch.equal(res["out"], x0 * 2)
    assert ME.torch is REAL        # (outside the context nothing is replaced)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_an_unwritten_element_is_caught(dtype):
    case, _ = _case(_kernel_skips_last, dtype)
    with pytest.raises(AssertionError, match="out differs between fill"):
        P.run_fills(case, "skips_last", modules=[ME])
    assert ME.torch is REAL


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_zero_times_an_unwritten_element_is_caught(dtype):
    """0 * NaN is NaN, while 0 * 3e38 is 0: the "nan" run is the one that differs from the "zero" run."""
    case, _ = _case(_kernel_zero_times_unwritten, dtype)
    with pytest.raises(AssertionError, match="out differs between fill 'zero' and fill 'nan'"):
        P.run_fills(case, "zero_times", modules=[ME])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_a_write_past_the_end_is_caught(dtype):
    case, _ = _case(_kernel_writes_past_the_end, dtype)
    size = 24 * dtype.itemsize
    with pytest.raises(AssertionError) as e:
        P.run_fills(case, "past_the_end", modules=[ME])
    msg = str(e.value)      # the buffer by its call site, the first and last changed offset (one element behind the tensor)
    assert "empty_like buffer of test_poison_host.py:" in msg and "first at offset %d, last at %d" % (size, size + dtype.itemsize - 1) in msg


def test_a_write_in_front_of_an_input_is_caught():
    with P.Poison("zero", modules=[ME]) as poison:
        x = poison.fenced(torch.ones(5))
        torch.empty(1)
        poison.check()
        lead = x.data_ptr() % P.GUARD // 4      # (floats of poison in front of x: the copy keeps x's address modulo 512)
        torch.as_strided(x, (1,), (1,), x.storage_offset() - lead - 1).fill_(0)
        with pytest.raises(AssertionError, match=r"fenced buffer of test_poison_host.py:\d+ .* first at offset -4, last at -"):
            poison.check()


def test_a_context_that_served_nothing_fails():
    """If the seam moves (the binding stops allocating by the name `torch`), check() must not pass silently."""
    with P.Poison("nan", modules=[ME]) as poison:
        poison.fenced(torch.ones(3))
        with pytest.raises(AssertionError, match="served no allocation"):
            poison.check()


def _alignment(t):
    return (t.data_ptr() & -t.data_ptr()) if t.data_ptr() else 0


NCHW, NHWC = torch.contiguous_format, torch.channels_last


@pytest.mark.parametrize("fill", P.FILLS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64, torch.uint8, torch.int32], ids=str)
def test_a_patched_allocation_is_laid_out_as_the_unpatched_one(dtype, fill):
    like_nhwc = torch.zeros(2, 6, 3, 5, dtype=dtype).contiguous(memory_format=NHWC)
    like_strided = torch.zeros(3, 11, 6, dtype=dtype)[:, 1:].transpose(1, 2)      # (empty_like: preserve_format -> dense)
    calls = [lambda t: t.empty((2, 6, 3, 5), dtype=dtype, memory_format=NCHW),
             lambda t: t.empty((2, 6, 3, 5), dtype=dtype, memory_format=NHWC),
             lambda t: t.empty(2, 7, dtype=dtype),
             lambda t: t.empty(37, dtype=dtype, device=torch.device("cpu")),
             lambda t: t.empty((0,), dtype=dtype),
             lambda t: t.empty(0, 8, dtype=dtype),
             lambda t: t.empty((0, 4, 3, 3), dtype=dtype, memory_format=NHWC),
             lambda t: t.empty_like(like_nhwc),
             lambda t: t.empty_like(like_strided),
             lambda t: t.empty_like(like_nhwc, memory_format=NCHW)]
    with P.Poison(fill, modules=[ME]) as poison:
        proxy = ME.torch
        assert proxy is not REAL
        for call in calls:
            a, b = call(proxy), call(REAL)
            assert a.shape == b.shape and a.stride() == b.stride() and a.dtype == b.dtype and a.device == b.device
            assert a.is_contiguous(memory_format=NHWC) == b.is_contiguous(memory_format=NHWC)
            assert type(a) is torch.Tensor and not a._is_view()     # an ordinary tensor set onto the storage
            if b.numel() == 0:
                assert a.data_ptr() == b.data_ptr() == 0        # (the binding hands the library NULL for such a tensor)
                continue
            assert a.data_ptr() % P.GUARD == 0 and _alignment(a) >= min(_alignment(b), P.GUARD)
            flat = torch.as_strided(a, (a.numel(),), (1,))      # dense: the interior is exactly the tensor
            if not dtype.is_floating_point or fill == "zero":
                assert (flat == 0).all()
            elif fill == "nan":
                assert flat.isnan().all()
            else:
                assert (flat[0::2] > 2.9e38).all() and (flat[1::2] < -2.9e38).all()
        assert poison.served == len(calls)
        poison.check()
    assert ME.torch is REAL


@pytest.mark.parametrize("fill", P.FILLS)
def test_fenced_keeps_a_views_strides_and_poisons_its_gaps(fill):
    """A class token in front of every image: [B, 1 + HW, C] viewed as [B, C, H, W], as the suite builds it."""
    B, C, H, W = 2, 4, 3, 5
    buf = torch.randn(B, 1 + H * W, C)
    view = buf[:, 1:].transpose(1, 2).unflatten(2, (H, W))
    with P.Poison(fill, modules=[ME]) as poison:
        f = poison.fenced(view)
        assert f.shape == view.shape and f.stride() == view.stride() and torch.equal(f, view)
        assert f.data_ptr() % P.GUARD == view.data_ptr() % P.GUARD and not f.requires_grad
        gaps = torch.as_strided(f, (B - 1, C), (f.stride(0), 1), f.storage_offset() + H * W * C)   # the later images' tokens
        if fill == "zero":
            assert (gaps == 0).all()
        elif fill == "nan":
            assert gaps.isnan().all()
        else:
            assert (gaps.abs() > 2.9e38).all()
        dense = poison.fenced(torch.arange(6.0).reshape(2, 3))
        assert torch.equal(dense, torch.arange(6.0).reshape(2, 3)) and dense.is_contiguous()
        torch.empty(1)
        poison.check()


def test_integer_buffers_are_zero_in_every_run():
    for fill in P.FILLS:
        with P.Poison(fill, modules=[ME]) as poison:
            ws = torch.empty(1000, dtype=torch.uint8)
            idx = torch.empty(7, 3, dtype=torch.int64)
            assert not ws.any() and not idx.any()
            assert ws.data_ptr() % P.GUARD == 0
            poison.check()


def test_the_binding_reaches_its_allocations_by_the_name_torch():
    """The seam: functional, compress and _ops hold `torch` itself outside a context and the proxy inside."""
    mods = P.binding_modules()
    assert [m.__name__.rsplit(".", 1)[1] for m in mods] == ["functional", "compress", "_ops"]
    with P.Poison("nan"):
        assert all(m.torch is not torch and m.torch.float32 is torch.float32 for m in mods)
        t = mods[0]._empty_grad_x(torch.zeros(2, 8, 3, 3), True)
        assert t.is_contiguous(memory_format=torch.channels_last) and t.isnan().all()
    assert all(m.torch is torch for m in mods)
