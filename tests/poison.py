"""Non-finite propagation and batch isolation for kernel tests: one poisoned element in, the right elements out.

A plain helper module like `guard.py` (no fixture, no setting, no GPU).  A case runs its kernel twice on the same operands, CLEAN
and with ONE element of ONE operand replaced by a poison (`KINDS`: a quiet NaN, +inf, -inf and, for fp16 storage only, `overflow`:
a finite value that drives some outputs past 65504).  `compare()` holds the two outputs against the float64 reference evaluated on
the same two operand sets ("Non-finite values"):

1. NO SWALLOWING.  Every output element falls in the class (`classify`: NaN, +inf, -inf, finite) of the reference on the poisoned
   operands, the reference rounded to the storage type first.
2. NO FINITE-BUT-WRONG OUTPUT.  Where the float64 reference is unchanged by the poison the kernel's element holds the bits of its
   own clean run; where it changes and stays finite the element passes the case's own rule (`finite_ok`; default: it equals the
   rounded reference), never a wider one.
3. BATCH ISOLATION.  No bit of image b' != b changes when the poison sits in image b (axis 0 of every output).  No exception.
4. FOOTPRINT.  Outside the poison's receptive field (`footprint`: taken structurally, `nan_footprint`) every element holds the bits
   of the clean run.  The only exception is a HALO the case declares as explicit positions: inside it an element may be NaN; if it
   is not NaN it obeys rules 1 and 2 like any other.  A halo never reaches another image: rule 3 is checked first and ignores it.

No tolerance lives here: every comparison is a class test, a bit identity or the rule the case brings along.
A failure is a `PoisonError` that names the rule, the operand, position and kind of the poison (`what`) and the first offending
output index.
"""
import math

import numpy as np
import torch

NAN, PINF, NINF, FINITE = 0, 1, 2, 3
CLASS_NAMES = ("NaN", "+inf", "-inf", "finite")
KINDS = ("nan", "+inf", "-inf")            # every storage type
OVERFLOW = "overflow"                      # fp16 storage only: the value is the case's (`overflow_ok` checks its choice)
F16_MAX = 65504.0


class PoisonError(AssertionError):
    def __init__(self, msg, rule, index):
        super().__init__(msg)
        self.rule, self.index = rule, index


def classify(t):
    """int8 tensor of the four classes, elementwise."""
    t = t.detach()
    c = torch.full(t.shape, FINITE, dtype=torch.int8)
    c[torch.isnan(t)] = NAN
    c[t == math.inf] = PINF
    c[t == -math.inf] = NINF
    return c


def poison_value(kind):
    return {"nan": math.nan, "+inf": math.inf, "-inf": -math.inf}[kind]


def positions(shape):
    """[(name, index)] of the poisons of an operand whose axis 0 is the image (NCHW, or [rows, features]); one poison per run.
    NCHW: the first element of image 0 (padding taps apply), the last element of the last image, the last row of image 0 and the
    first row of image 1 (the tile and halo rows that straddle two images), the centre of a middle image; first and last channel
    both occur.  Other ranks: first element, last element, the last element of row 0 and the first of row 1, the centre."""
    shape = tuple(int(s) for s in shape)
    B, last = shape[0], tuple(s - 1 for s in shape)
    if len(shape) == 4:
        _, C, H, W = shape
        out = [("first", (0, 0, 0, 0)), ("last", last), ("img0-last-row", (0, C - 1, H - 1, W // 2))]
        if B > 1:
            out.append(("img1-first-row", (1, 0, 0, W // 2)))
        out.append(("centre", (B // 2, C // 2 if C > 2 else C - 1, H // 2, W // 2)))
    else:
        rest = shape[1:]
        out = [("first", (0,) * len(shape)), ("last", last), ("row0-end", (0,) + tuple(s - 1 for s in rest))]
        if B > 1:
            out.append(("row1-start", (1,) + (0,) * len(rest)))
        out.append(("centre", (B // 2,) + tuple(s // 2 for s in rest)))
    seen, uniq = set(), []
    for name, idx in out:                    # (tiny operands: two names may hit one element)
        if idx not in seen:
            seen.add(idx)
            uniq.append((name, idx))
    return uniq


def poisoned(t, index, value):
    """A copy of CPU tensor `t` with `t[index] = value`."""
    t = t.clone()
    t[tuple(index)] = value
    return t


def nan_footprint(ref_with_nan):
    """The receptive field of a poison, structurally: where the float64 reference evaluated with a NaN at the poison's place is
    NaN (NaN goes through every sum, product, maximum and activation of the references; no weight is zero, `assert_no_zero`)."""
    return torch.isnan(ref_with_nan)


def assert_no_zero(w, what=""):
    """inf * w is +-inf for every w, in any summation order, only if no weight is exactly zero."""
    assert int((w == 0).sum()) == 0, (what, "a weight is exactly zero: inf * 0 would make the reference's class depend on it")


def assert_fp32_safe(S, what=""):
    """No finite float64 magnitude sum comes near the fp32 maximum: the kernel's fp32 partial sums (each at most S) stay finite
    wherever the reference does."""
    fin = S[torch.isfinite(S)]
    assert fin.numel() == 0 or float(fin.max()) < 2.0 ** 100, (what, "a finite intermediate reaches", float(fin.max()))


def overflow_ok(ref_poison, what=""):
    """The `overflow` value was chosen well: every float64 reference output is >= 2 x 65504 in magnitude (it overflows fp16 whatever
    the fp32 accumulation order) or <= 0.5 x 65504 (it does not), and at least one overflows."""
    a = ref_poison.abs()
    mid = (a > 0.5 * F16_MAX) & (a < 2.0 * F16_MAX)
    assert not bool(mid.any()), (what, "reference outputs between 0.5 x and 2 x 65504:", int(mid.sum()), "first", float(a[mid][0]))
    assert bool((a >= 2.0 * F16_MAX).any()), (what, "no reference output overflows")


def _bits(t):
    es = t.element_size()
    return t.detach().contiguous().reshape(-1).view(torch.uint8).numpy().reshape(-1, es)


def _first(mask):
    """Index tuple of the first True of a bool tensor, or None."""
    flat = np.flatnonzero(mask.reshape(-1).numpy())
    if flat.size == 0:
        return None, 0
    return tuple(int(v) for v in np.unravel_index(int(flat[0]), tuple(mask.shape))), int(flat.size)


def _fail(rule, what, msg, mask, got_clean, got_poison, ref_poison):
    idx, n = _first(mask)
    raise PoisonError("%s: rule %d, %s: %d of %d elements, first at %s: clean run %r, poisoned run %r, reference %r" % (
        what, rule, msg, n, mask.numel(), list(idx), got_clean[idx].item(), got_poison[idx].item(), ref_poison[idx].item()), rule, idx)


def compare(got_clean, got_poison, ref_clean, ref_poison, footprint, image=None, halo=None, finite_ok=None, what=""):
    """THE RULES (module docstring) on one poisoned run.
    got_clean, got_poison  the kernel's outputs (CPU, storage type, axis 0 = image)
    ref_clean, ref_poison  the float64 reference on the same operands, same shape; with `image` given they, `footprint` and `halo`
                           may cover the poisoned image alone (axis 0 of size 1): rule 3 needs no reference
    footprint              bool, same shape: the poison's receptive field (`nan_footprint`)
    image                  the image the poison sits in; None for an operand every image shares (a shift): rule 3 is then void
    halo                   bool, same shape, or None: the declared positions where a NaN is tolerated
    finite_ok(got, want64, mask) -> bool tensor of `mask`'s shape, True where `got` passes the case's own rule against the float64
                           reference; only read where `mask` is True.  Default: `got` equals the reference rounded to storage."""
    dtype = got_clean.dtype
    assert got_poison.dtype == dtype and tuple(got_clean.shape) == tuple(got_poison.shape), what
    if image is not None:                                                   # rule 3: checked first, on every image, no exception
        other = torch.from_numpy(~(_bits(got_clean) == _bits(got_poison)).all(axis=1)).view(got_clean.shape)
        other[image] = False
        if bool(other.any()):
            _fail(3, what, "an element of another image than %d changed" % image, other, got_clean, got_poison, torch.full(got_clean.shape, math.nan))
        if ref_clean.shape[0] == 1 and got_clean.shape[0] != 1:             # the references cover the poisoned image alone
            try:
                return compare(got_clean[image:image + 1], got_poison[image:image + 1], ref_clean, ref_poison, footprint, 0, halo, finite_ok, what)
            except PoisonError as e:
                raise PoisonError(str(e) + " (image %d)" % image, e.rule, (image,) + tuple(e.index[1:])) from None
    assert tuple(got_clean.shape) == tuple(ref_clean.shape) == tuple(ref_poison.shape), what
    footprint = footprint.expand(got_clean.shape)
    halo = torch.zeros(got_clean.shape, dtype=torch.bool) if halo is None else halo.expand(got_clean.shape)
    same_bits = torch.from_numpy((_bits(got_clean) == _bits(got_poison)).all(axis=1)).view(got_clean.shape)
    got_nan = torch.isnan(got_poison)
    ref_same = (ref_clean == ref_poison) | (torch.isnan(ref_clean) & torch.isnan(ref_poison))
    assert bool(ref_same[~footprint].all()), (what, "the reference itself changes outside the footprint")

    bad = ~footprint & ~halo & ~same_bits                                   # rule 4
    if bool(bad.any()):
        _fail(4, what, "an element outside the receptive field and the declared halo changed", bad, got_clean, got_poison, ref_poison)
    tolerated = halo & got_nan                                              # inside a halo: NaN, or the rules below
    want = ref_poison.to(dtype)
    bad = (classify(got_poison) != classify(want)) & ~tolerated             # rule 1
    if bool(bad.any()):
        idx, _ = _first(bad)
        _fail(1, what, "class %s where the reference is %s" % (CLASS_NAMES[int(classify(got_poison)[idx])], CLASS_NAMES[int(classify(want)[idx])]),
              bad, got_clean, got_poison, ref_poison)
    bad = ref_same & ~same_bits & ~tolerated                                # rule 2, unchanged reference
    if bool(bad.any()):
        _fail(2, what, "the reference is unchanged by the poison but the element is not", bad, got_clean, got_poison, ref_poison)
    changed = ~ref_same & torch.isfinite(want) & ~tolerated                  # rule 2, changed and finite
    if bool(changed.any()):
        ok = (got_poison.double() == want.double()) if finite_ok is None else finite_ok(got_poison, ref_poison, changed)
        bad = changed & ~ok
        if bool(bad.any()):
            _fail(2, what, "finite, changed by the poison and outside the case's rule against the reference", bad, got_clean, got_poison, ref_poison)
