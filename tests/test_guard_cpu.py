"""The guard-band harness (`guard.py`) tested without a GPU: `device="cpu"` buffers and small numpy "kernels", one correct and
five wrong in the five ways the harness exists to catch.  Each wrong kernel must fail for its own reason - `check()` for a byte
before or after the payload and for a modified operand, the two-fill comparison for an element left unwritten and for a value
read from an operand's band - and the message must name the allocation and the offset."""
import ctypes
import types

import numpy as np
import pytest
import torch

import guard
from guard import Guard, GuardError, two_fills

BAND = 4096          # (the CPU kernels stray by one element; the device tests use guard.BAND)
N = 37


def _np(t):
    return t.numpy()


def _bytes_at(t, byte_offset, n):
    """n raw bytes at `byte_offset` from a tensor's first byte (inside its guarded buffer)."""
    return (ctypes.c_uint8 * n).from_address(t.data_ptr() + byte_offset)


class fake_ops:
    """A stand-in for `ops.py`: the wrapper allocates its output with the module's `torch`, the "kernel" is numpy."""
    torch = torch
    bug = None

    @staticmethod
    def scale(x):
        torch = fake_ops.torch
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        xs, o = _np(x), _np(out)
        n = x.numel() - (1 if fake_ops.bug == "unwritten" else 0)
        o.reshape(-1)[:n] = 2.0 * xs.reshape(-1)[:n]
        if fake_ops.bug == "before":
            _bytes_at(out, -1, 1)[0] = 0
        elif fake_ops.bug == "after":
            _bytes_at(out, out.numel() * 4, 1)[0] = 0
        elif fake_ops.bug == "operand":
            xs.reshape(-1)[5] = 1.0
        elif fake_ops.bug == "leak":     # the last element is computed from the float that FOLLOWS the operand
            o.reshape(-1)[-1] = 2.0 * np.frombuffer(_bytes_at(x, x.numel() * 4, 4), np.float32)[0]
        return out


@pytest.fixture
def ops_module():
    fake_ops.torch, fake_ops.bug = torch, None
    yield fake_ops
    fake_ops.torch, fake_ops.bug = torch, None


X = torch.arange(N, dtype=torch.float32).reshape(1, N) + 0.5


def _run(place):
    return fake_ops.scale(place(X))


def _guarded(fill, bug):
    fake_ops.bug = bug
    g = Guard(fill, BAND, "cpu")
    with g.patch(fake_ops):
        out = fake_ops.scale(g.place(X))
    return g, out


def test_layout_of_an_allocation():
    g = Guard(0x5A, BAND, "cpu")
    for shape, dtype in (((3, 5), torch.float16), ((7,), torch.uint8), ((2, 2), torch.int64), ((1,), torch.bfloat16)):
        t = g.empty(shape, dtype)
        a = g.allocs[-1]
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
        assert t.data_ptr() % 256 == 0 and a.off >= BAND
        assert a.raw.numel() == a.off + a.nbytes + BAND                       # the rear band starts at the payload's end
        assert t.data_ptr() == a.raw.data_ptr() + a.off
        assert bool((a.raw == 0x5A).all())                                     # bands and payload at fill
    x = torch.randn(4, 3).to(torch.bfloat16)
    p = g.place(x)
    assert torch.equal(p, x) and g.allocs[-1].cpu is not x and g.allocs[-1].kind == "operand"
    g.check()
    assert g.empty((0, 4), torch.float32).shape == (0, 4)
    g.check()


def test_fills_mean_what_the_rule_says():
    nan = Guard(0xFF, 16, "cpu")
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        assert bool(torch.isnan(nan.empty((3,), dt)).all())
    assert nan.empty((3,), torch.int32).tolist() == [-1] * 3
    fin = Guard(0x5A, 16, "cpu")
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        assert bool(torch.isfinite(fin.empty((3,), dt)).all())
    assert float(fin.empty((1,), torch.float16)) == 203.25
    assert int(fin.empty((1,), torch.int32)) == 0x5A5A5A5A
    assert guard.BAND >= guard.LARGEST_TILE_BYTES == 224 * 256 * 2


def test_correct_kernel_passes(ops_module):
    ref = two_fills(_run, [fake_ops], device="cpu", band=BAND, what="scale")
    assert torch.equal(ref[0], 2.0 * X)
    assert fake_ops.torch is torch                                             # the patch is undone


@pytest.mark.parametrize("bug,region,offset,order", [("before", "front", -1, 1), ("after", "rear", 0, 1), ("operand", "operand", 22, 0)])     # (5.5 -> 1.0 = 0x40B00000 -> 0x3F800000: element 5's byte 2)
def test_check_names_the_allocation_and_the_offset(ops_module, bug, region, offset, order):
    for fill in guard.FILLS:
        g, _ = _guarded(fill, bug)
        with pytest.raises(GuardError) as e:
            g.check()
        assert (e.value.order, e.value.region, e.value.offset) == (order, region, offset)
        msg = str(e.value)
        assert "allocation #%d" % order in msg and "offset %d" % offset in msg
        if order == 1:
            assert "[1, 37] float32" in msg and "asked for by test_guard_cpu.scale" in msg and "empty" in msg
        else:
            assert "operand" in msg and "asked for by test_guard_cpu._guarded" in msg
    with pytest.raises(GuardError):
        fake_ops.bug = bug
        two_fills(_run, [fake_ops], device="cpu", band=BAND)
    assert fake_ops.torch is torch                                             # undone after a failure too


def test_unwritten_element_fails_the_two_fill_rule(ops_module):
    g, out = _guarded(0x5A, "unwritten")
    g.check()                                                                  # nothing out of bounds: the bands cannot see it
    assert float(out[0, -1]) == float(torch.tensor([0x5A5A5A5A], dtype=torch.int32).view(torch.float32))
    fake_ops.bug = "unwritten"
    with pytest.raises(AssertionError, match=r"result 0 differs between fill 0xFF and fill 0x5A.*first at \[0, 36\]"):
        two_fills(_run, [fake_ops], device="cpu", band=BAND, what="scale")


def test_value_read_from_a_band_fails_the_two_fill_rule(ops_module):
    g, out = _guarded(0x5A, "leak")
    g.check()                                                                  # reads leave no trace in the bands
    assert bool(torch.isfinite(out).all())
    fake_ops.bug = "leak"
    with pytest.raises(AssertionError, match=r"result 0 differs between fill 0xFF and fill 0x5A.*first at \[0, 36\]"):
        two_fills(_run, [fake_ops], device="cpu", band=BAND, what="scale")


def test_result_that_differs_from_the_unguarded_call_fails():
    calls = []

    def run(place):
        calls.append(1)
        return place(X) + (1.0 if len(calls) == 1 else 0.0)
    with pytest.raises(AssertionError, match="differs from the unguarded call"):
        two_fills(run, device="cpu", band=BAND)
    assert guard.first_difference(torch.tensor([float("nan")]), torch.tensor([float("nan")])) is None     # bits, not values
    assert guard.first_difference(torch.tensor([0.0]), torch.tensor([-0.0])) is not None


def test_proxy_overrides_five_functions_and_delegates_the_rest():
    m = types.SimpleNamespace(torch=torch)
    g = Guard(0xFF, BAND, "cpu")
    with g.patch(m):
        t = m.torch
        assert t is not torch and t.float16 is torch.float16 and t.cuda is torch.cuda and t.Tensor is torch.Tensor
        assert t.from_numpy is torch.from_numpy and isinstance(t.empty((2,), device="cpu"), t.Tensor)
        e = t.empty((3, 5), dtype=torch.float16, device="cpu")
        assert len(g.allocs) == 2 and g.allocs[1].shape == (3, 5) and g.allocs[1].nbytes == 30 and bool(torch.isnan(e).all())
        assert t.empty(2, 3, dtype=torch.int32, device="cpu").tolist() == [[-1] * 3] * 2
        z = t.zeros((4,), dtype=torch.int64, device=torch.device("cpu"))
        assert z.tolist() == [0] * 4 and g.allocs[-1].nbytes == 32
        assert t.full((2,), -1, dtype=torch.int32, device="cpu").tolist() == [-1, -1]
        assert t.zeros_like(e).tolist() == [[0.0] * 5] * 3 and t.empty_like(z).shape == (4,) and t.empty_like(z).dtype == torch.int64
        n = len(g.allocs)
        assert n == 8 and all(a.who == "test_guard_cpu.test_proxy_overrides_five_functions_and_delegates_the_rest" for a in g.allocs)
        # a request without a device is a host tensor of the wrapper's own: torch's, not the guard's
        assert t.empty((2,)).shape == (2,) and t.zeros((2,)).tolist() == [0.0, 0.0] and t.full((2,), -1, dtype=torch.int32).tolist() == [-1, -1]
        assert len(g.allocs) == n
    assert m.torch is torch
    g.check()
    # a guard for the GPU leaves a proxied module's CPU requests to torch (constructing it needs no GPU)
    gg = Guard(0xFF, BAND, "cuda")
    with gg.patch(m):
        assert m.torch.empty((2,), dtype=torch.float32, device="cpu").shape == (2,) and m.torch.zeros((2,), device="cpu").tolist() == [0.0, 0.0]
        assert gg.allocs == []
    assert m.torch is torch
