"""CPU: the pointer-alignment contract (include/frmap_hip.h, Conventions, "pointer alignment") and the tools that test it.

* `guard.Guard` with a placement rule on `device="cpu"`: payloads start where the rule says, and `check()` still finds a one-byte
  overrun just before and just after a shifted payload (positive controls, as `test_guard_cpu.py` has for the aligned guard).
* `guard.shifted` rejects an emulated kernel that reads its operand in 16-byte vectors at addresses TRUNCATED to 16 bytes - what a
  vector load does on hardware that ignores the low address bits, the failure the rule is about - and one that takes its whole
  output tile from the 256-byte line the payload starts in; it accepts an honest element-wise kernel.
* The requirement table of the binding (`_lib.ALIGNMENT`) names every device-pointer argument of every launching prototype of the
  header and nothing else, and every figure in it is the header's: its class's line in the Conventions block, or the argument's
  own note next to its declaration.
* Every launcher refuses a pointer below its requirement: the calls of `place_cases.REJECT_CALLS` with host dummy pointers.  The
  refusal comes before any HIP call, so no GPU is needed; with a GPU present `test_place_ops_gpu.py` makes the same calls on
  device memory instead, and these are skipped.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import guard
import place_cases as pc
from frmap_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()


# ---------------------------------------------------------------------------------------------------------------------------------
# the shifted guard
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,need", [(torch.uint8, 1), (torch.float16, 2), (torch.float32, 4), (torch.float32, 16), (torch.float16, 16),
                                        (torch.int32, 8), (torch.float64, 8), (torch.float32, 128), (torch.uint8, 256)])
def test_placement_obeys_the_rule(dtype, need):
    g = guard.Guard(0x5A, 512, "cpu", shift=guard.min_placement(need))
    t = g.place(torch.arange(37).to(dtype))
    e = g.empty((5, 3), dtype)
    for p in (t, e):
        assert p.data_ptr() % need == 0 and (need >= guard.ALIGN or p.data_ptr() % (2 * need) == need), (p.data_ptr() % 256, need)
        assert p.data_ptr() % guard.ALIGN == (need if need < guard.ALIGN else 0)
    assert torch.equal(t, torch.arange(37).to(dtype)) and bool((e.view(torch.uint8) == 0x5A).all())
    g.check()


def test_no_rule_is_the_aligned_guard_and_bad_shifts_are_refused():
    g = guard.Guard(0xFF, 64, "cpu")
    assert g.place(torch.zeros(3)).data_ptr() % guard.ALIGN == 0
    rule_by_kind = lambda dtype, kind, who: {"operand": 16, "empty": 4}[kind]
    g = guard.Guard(0xFF, 64, "cpu", shift=guard.min_placement(rule_by_kind))
    assert g.place(torch.zeros(3)).data_ptr() % 256 == 16 and g.empty((3,), torch.float32).data_ptr() % 256 == 4
    for bad in (lambda *a: 2, lambda *a: 256, lambda *a: -4):         # not a multiple of the element size / outside [0, 256)
        with pytest.raises(ValueError):
            guard.Guard(0xFF, 64, "cpu", shift=bad).place(torch.zeros(3))
    with pytest.raises(ValueError):
        guard.min_placement(12)(torch.float32, "operand", "?")


@pytest.mark.parametrize("need", [4, 16])
@pytest.mark.parametrize("side", ["front", "rear"])
def test_check_finds_a_one_byte_overrun_beside_a_shifted_payload(side, need):
    """Positive control: the band begins at the byte before the payload's first and at the byte after its last, shifted or not."""
    g = guard.Guard(0x5A, 512, "cpu", shift=guard.min_placement(need))
    g.place(torch.zeros(7))
    out = g.empty((9,), torch.float32)
    a = g.allocs[1]
    g.check()
    a.raw[a.off - 1 if side == "front" else a.off + a.nbytes] = 0
    with pytest.raises(guard.GuardError) as e:
        g.check()
    assert (e.value.order, e.value.region, e.value.offset) == (1, side, -1 if side == "front" else 0), str(e.value)
    assert out.data_ptr() % 256 == need


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule against emulated kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def _bytes_at(t, addr, n):
    """n bytes at absolute address `addr` of the storage `t` is a view of (a guarded payload: the bands around it are addressable)."""
    base = t.untyped_storage().data_ptr()
    whole = torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage())
    return whole[addr - base: addr - base + n]


def _double_it(load):
    """An element-wise "kernel" y = 2 x over fp32 whose operand reads go through `load(x, i)` -> the 4 floats of vector i."""
    def op(x):
        n = x.numel()
        out = torch.empty((n,), dtype=torch.float32, device=x.device)
        for i in range((n + 3) // 4):
            v = load(x, i)
            k = min(4, n - 4 * i)
            out[4 * i: 4 * i + k] = 2 * v[:k]
        return out
    return op


def _honest(x, i):
    v = torch.zeros(4)
    k = min(4, x.numel() - 4 * i)
    v[:k] = x[4 * i: 4 * i + k]
    return v


def _truncating(x, i):
    """A 16-byte vector load whose address loses its low four bits."""
    addr = (x.data_ptr() + 16 * i) & ~15
    return _bytes_at(x, addr, 16).view(torch.float32).clone()


def _line_based(x, i):
    """A fetch that starts from the 256-byte line the operand lies in (a descriptor base assumed 256-byte aligned)."""
    line = x.data_ptr() & ~255
    if line < x.untyped_storage().data_ptr():      # (the unguarded call: the CPU allocator's 64 bytes stand for the aligned start)
        line = x.data_ptr()
    return _bytes_at(x, line + 16 * i, 16).view(torch.float32).clone()


def test_shifted_accepts_an_honest_kernel_and_rejects_truncated_vector_loads():
    x = torch.arange(1, 24, dtype=torch.float32)
    rule = lambda load, need: guard.shifted(lambda place: _double_it(load)(place(x)), device="cpu", band=1024, requirement=need, what="emulated")
    for need in (4, 8, 16):
        y, = rule(_honest, need)
        assert torch.equal(y, 2 * x)
    # at 16 bytes and beyond a truncated 16-byte load IS the load: accepted, and rightly
    assert torch.equal(rule(_truncating, 16)[0], 2 * x)
    for need in (4, 8):                        # below the vector width the truncated address is another one
        with pytest.raises(AssertionError, match="differs from the aligned call"):
            rule(_truncating, need)
    for need in (4, 16, 128):                  # a base rounded down to its line reads the band wherever the payload is shifted
        with pytest.raises(AssertionError, match="differs from the aligned call"):
            rule(_line_based, need)
    assert torch.equal(rule(_line_based, 256)[0], 2 * x)


def test_shifted_rejects_a_store_that_overruns_a_shifted_output():
    """The output is placed by the rule as well: a kernel that rounds its store address up to 16 bytes writes the rear band."""
    x = torch.arange(1, 9, dtype=torch.float32)
    mod = type("M", (), {"torch": torch})()

    def op(xd):
        out = mod.torch.empty((8,), dtype=torch.float32, device=xd.device)
        addr = (out.data_ptr() + 15) & ~15
        _bytes_at(out, addr, 32).view(torch.float32).copy_(2 * xd)
        return out
    assert torch.equal(guard.shifted(lambda place: op(place(x)), [mod], device="cpu", band=1024, requirement=16)[0], 2 * x)
    with pytest.raises(guard.GuardError) as e:
        guard.shifted(lambda place: op(place(x)), [mod], device="cpu", band=1024, requirement=4)
    assert e.value.region == "rear" and e.value.offset == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the table and the header
# ---------------------------------------------------------------------------------------------------------------------------------
def _launching_prototypes():
    """{entry point: [device-pointer argument names]} of the header's prototypes that take a `stream`, and where each is declared.
    Host pointers (`*_host`) and the model handle are not device pointers."""
    text = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), HEADER, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|size_t)\s+(frmap_\w+)\s*\(([^)]*)\)\s*;", text):
        name, args = m.group(1), m.group(2)
        if "void* stream" not in args:
            continue
        ptrs = [a.split("*")[-1].strip() for a in (s.strip() for s in args.split(","))
                if "*" in a and not a.endswith("stream") and "frmap_model" not in a and not a.endswith("_host")]
        if ptrs:
            out[name] = (ptrs, m.start())
    return out


def test_the_table_names_every_pointer_of_every_launching_prototype_and_nothing_else():
    protos = _launching_prototypes()
    assert len(protos) >= 50 and "frmap_conv_igemm" in protos and "frmap_track_step_host" not in protos
    assert set(_lib.ALIGNMENT) == set(protos), (set(_lib.ALIGNMENT) ^ set(protos))
    for entry, (ptrs, _) in protos.items():
        assert list(_lib.ALIGNMENT[entry]) == ptrs, (entry, list(_lib.ALIGNMENT[entry]), ptrs)     # (in declaration order)
        assert entry in _lib.PROTOTYPES
        for arg, (cls, need) in _lib.ALIGNMENT[entry].items():
            assert cls in _lib.ALIGN_CLASS and need in (1, 2, 4, 8, 16, 256), (entry, arg, cls, need)
            assert _lib.align_of(entry, arg) == need


CLASS_LINE = {"tensor": r"tensors in `dtype`", "vector": r"fp32 per-channel vectors of the MFMA kernels", "matrix": r"fp32 matrices that a GEMM",
              "element": r"everything walked element by element", "record": r"records with 8-byte fields", "workspace": r"workspaces and state buffers"}


def _conventions():
    block = HEADER[HEADER.index("pointer alignment:"):HEADER.index("#ifndef FRMAP_HIP_H")]
    return re.sub(r"\s*\n \*\s*", " ", block)


def test_every_class_figure_is_in_the_conventions_block():
    text = _conventions()
    starts = sorted((re.search(pat, text).start(), cls) for cls, pat in CLASS_LINE.items())
    for k, (at, cls) in enumerate(starts):
        line = text[at: starts[k + 1][0] if k + 1 < len(starts) else len(text)]
        want = _lib.ALIGN_CLASS[cls]
        if want is None:
            assert "the element size" in line, (cls, line)
        else:
            assert "%d-byte aligned" % want in line, (cls, want, line)
    assert "256-byte aligned where the entry point says so" in text and "rejected (-1" in text and "before any launch" in text


def _comment_for(entry, arg, at):
    """The nearest comment above the declaration at `at` that speaks of `arg` (several entry points may share one comment)."""
    comments = [(m.start(), m.group(0)) for m in re.finditer(r"/\*.*?\*/", HEADER, flags=re.S) if m.start() < at]
    for _, c in reversed(comments[1:]):                       # (comments[0] is the file's own, with the Conventions block)
        c = re.sub(r"\s*\n \*\s*", " ", c)
        if re.search(r"(?<![\w])%s(?![\w])" % re.escape(arg), c):
            return c
    return ""


def test_every_departure_from_a_class_is_stated_next_to_the_declaration():
    protos = _launching_prototypes()
    seen = 0
    for entry, args in _lib.ALIGNMENT.items():
        for arg, (cls, need) in args.items():
            default = _lib.ALIGN_CLASS[cls]
            if default is None:
                default = pc.element_size(entry, arg)
            if need == default:
                continue
            seen += 1
            c = _comment_for(entry, arg, protos[entry][1])
            near = re.search(r"(?<![\w])%s(?![\w])[^.]{0,220}?\b%d-byte aligned|\b%d-byte aligned[^.]{0,220}?(?<![\w])%s(?![\w])"
                             % (re.escape(arg), need, need, re.escape(arg)), c)
            assert near, "%s(%s): %d bytes departs from class %r (%s) and the header does not say so next to the declaration" % (
                entry, arg, need, cls, default)
    assert seen >= 20          # the 256-byte workspaces, the 8-byte NHWC4 pixels, the element-wise packers, rois_out, x_u8_hwc ...


# ---------------------------------------------------------------------------------------------------------------------------------
# the rejections, on host dummy pointers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_rejection_table_covers_the_requirement_table():
    calls = pc.misaligned_calls()
    assert len(calls) >= 100
    for entry, arg, need in calls:
        assert entry in pc.REJECT_CALLS and arg in pc.REJECT_CALLS[entry], (entry, arg)
        ptrs = [a for a in pc.REJECT_CALLS[entry] if isinstance(a, str) and a not in ("mean", "std")]
        assert ptrs == list(_lib.ALIGNMENT[entry]), entry
        assert len(pc.REJECT_CALLS[entry]) + 1 == len(_lib.PROTOTYPES[entry][1]), entry


@pytest.mark.skipif(torch.cuda.is_available(), reason="with a GPU test_place_ops_gpu.py makes these calls on device memory")
@pytest.mark.parametrize("entry,arg,need", pc.misaligned_calls(), ids=["%s-%s" % (e[6:], a) for e, a, _ in pc.misaligned_calls()])
def test_a_pointer_below_its_requirement_is_refused_before_any_work(entry, arg, need):
    lib = _lib.load()
    pool = {a: np.zeros(pc.REJECT_BYTES + 256, np.uint8) for a in _lib.ALIGNMENT[entry]}
    bufs = {a: (b.ctypes.data + 255) // 256 * 256 for a, b in pool.items()}
    mean, std = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25)
    rc = getattr(lib, entry)(*pc.reject_args(entry, arg, bufs, mean, std))
    msg = lib.frmap_last_error().decode()
    assert rc == -1, (entry, arg, rc, msg)
    assert re.search(r"(?<![\w])%s(?![\w])" % re.escape(arg), msg) and "%d-byte aligned" % need in msg, (entry, arg, msg)
    if (entry, arg) not in pc.OWN_WORDING:
        assert msg.startswith(entry[6:] + ": ") or msg.startswith(entry[6:].rsplit("_", 1)[0]), (entry, msg)
    assert all(not b.any() for b in pool.values())
