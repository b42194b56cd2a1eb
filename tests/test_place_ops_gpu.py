"""GPU: the layout / pool / cast kernels, the heads, the matching entry points, the transformer kernels and the trackers where
their buffers start, the launchers' refusals, and what the binding does with a view.

1. Every two-fill test of `test_guard_ops_gpu.py` (all of its cases: its shapes are already the smallest that reach each path) runs
   again under `guard.shifted`: every operand, and every output and workspace the wrapper allocates, "aligned to A and not to 2 A"
   for the A of `place_cases.requirement`, under both fills; `check()` passes, the bits are the aligned call's, and the tests that
   compare with a float64 reference (layout / pool / cast) go on to do so.  The only atomics are on integers: no exception.
2. The same tests once more with every placed operand a contiguous view one element into its allocation (`flat[1:1 + n].view(shape)`):
   the binding copies an operand that is below its argument's requirement and passes on one that meets it (the element-wise heads
   and casts then run on a pointer aligned to one element and not to two), so the result holds the bits of the call on clones.
3. Every launcher's refusal (`place_cases.misaligned_calls`, 100+ calls): the smallest valid call with one pointer moved by half its
   requirement - one element where that is more - inside guarded device memory of 64 KiB per argument, so that even a missing check
   could touch only memory this test owns.  The call returns -1, the text names the argument and the bytes, the device is clean
   afterwards and no byte of any buffer or band has changed.
4. A caller-owned tensor cannot be copied: a misaligned tracker state raises ValueError naming the requirement, and a `packed=` slice
   that meets its 4 bytes (a micro-batch's rows of one record buffer) is written in place.
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import place_cases as pc  # noqa: E402
import test_guard_ops_gpu as tg  # noqa: E402
from frmap_amd import _lib, ops, synth  # noqa: E402

DEV = "cuda"
GUARD_TESTS = [n for n in dir(tg) if n.startswith("test_") and n != "test_positive_control_one_element_too_many"]
assert len(GUARD_TESTS) >= 20

for _name in GUARD_TESTS:
    globals()[_name + "_at_minimum_alignment"] = pc.mirror(tg, _name)
    globals()[_name + "_on_offset_views"] = pc.mirror_offset(tg, _name)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,arg,need", pc.misaligned_calls(), ids=["%s-%s" % (e[6:], a) for e, a, _ in pc.misaligned_calls()])
def test_a_pointer_below_its_requirement_is_refused_before_any_launch(entry, arg, need):
    lib = _lib.load()
    g = guard.Guard(0x5A, band=4096)
    bufs = {a: g.empty((pc.REJECT_BYTES,), torch.uint8).data_ptr() for a in _lib.ALIGNMENT[entry]}
    mean, std = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25)
    args = pc.reject_args(entry, arg, bufs, mean, std)
    args[-1] = torch.cuda.current_stream().cuda_stream
    rc = getattr(lib, entry)(*args)
    msg = lib.frmap_last_error().decode()
    assert rc == -1, (entry, arg, rc, msg)
    assert re.search(r"(?<![\w])%s(?![\w])" % re.escape(arg), msg) and "%d-byte aligned" % need in msg, (entry, arg, msg)
    torch.cuda.synchronize()
    g.check()                                                     # the bands
    for a in g.allocs:                                            # ... and every payload: still the fill
        assert bool((a.raw == 0x5A).all()), (entry, arg, a.describe())


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. caller-owned tensors
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_misaligned_tracker_state_raises():
    S, M, D = 2, 3, 8
    hw = torch.tensor([[240, 320]] * S, dtype=torch.int32, device=DEV)
    boxes = torch.zeros((S, M, 4), device=DEV)
    counts = torch.zeros((S,), dtype=torch.int32, device=DEV)
    n = ops.track_state_bytes(S, M)
    raw = torch.zeros((n + 16,), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.track_step(raw[8:8 + n], boxes, None, counts, hw)
    assert int(raw.max()) == 0
    ops.track_step(raw[:n], boxes, None, counts, hw)              # (the aligned view of the same buffer is taken)
    nf = ops.track_fuse_state_bytes(S, M, D)
    rawf = torch.zeros((nf + 16,), dtype=torch.uint8, device=DEV)
    ids = torch.full((S, M), -1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.track_fuse(rawf[4:4 + nf], ids, counts, torch.zeros((0, D), device=DEV), np.zeros((0, 2), np.int32))
    torch.cuda.synchronize()
    assert int(rawf.max()) == 0


def test_a_packed_slice_at_four_bytes_is_written_in_place():
    """`GraphedEmbedMatch` hands each micro-batch's rows of one [B, 2] record buffer to the match: 8-byte steps; 4 bytes serve."""
    B, G, Dm = 5, 7, 64
    gal, pr = synth.unit_rows(41, G, Dm, "g.gal").to(DEV), synth.unit_rows(42, B, Dm, "g.pr").to(DEV)
    want = ops.match_top1(pr, gal, 0.9, packed=True)[3]
    flat = torch.full((2 * B + 1,), -7, dtype=torch.int32, device=DEV)
    pk = flat[1:].view(B, 2)
    assert pk.data_ptr() % 8 == 4
    got = ops.match_top1(pr, gal, 0.9, packed=pk)[3]
    assert got.data_ptr() == pk.data_ptr() and torch.equal(pk, want) and int(flat[0]) == -7


def test_two_copied_operands_of_one_call_keep_their_own_memory():
    """The binding copies an operand it cannot pass on (strided here, misaligned in the offset-view tests).  Three such operands of
    equal size in ONE call: each copy must live until the launch - a copy freed as soon as its address is taken gives its block to
    the next one, and pos, gamma and beta would be one vector."""
    B, L, D = 2, 5, 64
    x = synth.randn(51, (B, L, D), "g.x").to(torch.float16).to(DEV)
    wide = synth.randn(52, (3, D, 2), "g.p").to(DEV)
    pos_row, gamma, beta = wide[0, :, 0], wide[1, :, 0].abs() + 0.5, wide[2, :, 0]
    pos = pos_row.expand(L, D)                                     # (strided: stride 0 over tokens, 2 over channels)
    assert not pos.is_contiguous() and not wide[2, :, 0].is_contiguous()
    t0, y0 = ops.add_pos_layernorm(x, pos.contiguous(), gamma.contiguous(), beta.contiguous(), want_sum=True)
    t1, y1 = ops.add_pos_layernorm(x, pos, wide[1, :, 0].abs() + 0.5, wide[2, :, 0], want_sum=True)
    assert torch.equal(t0, t1) and torch.equal(y0, y1)
    m0 = ops.mean_layernorm(x, gamma.contiguous(), beta.contiguous())
    assert torch.equal(m0, ops.mean_layernorm(x, (wide[1] * 1)[:, 0].abs() + 0.5, wide[2, :, 0]))
