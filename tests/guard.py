"""Guard bands for kernel tests: a kernel writes all of its output and nothing else, and reads nothing but its operands.

A plain helper module like `conv_cases.py` (no fixture, no setting).  Every tensor a guarded case hands to a kernel - operand,
output, workspace - is the middle of one `uint8` buffer of `band + nbytes + band` bytes, all set to one `fill` byte.  The payload
starts 256-byte aligned and its end is NOT padded: the rear band begins at the byte after the payload's last byte, so a
ragged-tail store one element too far, or a workspace one byte smaller than the kernel uses, lands in the band.

* `Guard.place(cpu_tensor)`: an operand; the payload is a copy of the tensor and the CPU copy is kept.
* `Guard.empty(shape, dtype)`: an output or workspace; the payload stays at `fill`.
* `Guard.patch(module, ...)`: for the `with` block the modules' `torch` attribute is a proxy whose `empty`, `empty_like`,
  `zeros`, `zeros_like` and `full` come from the guard when the request is for the guard's device (everything else is `torch`'s
  own), so whatever the production wrappers allocate is guarded at exactly the size they ask for.
* `Guard.check()`: synchronises (a device error ends the session, as `conv_cases._sync`), then both bands of every allocation
  are byte-identical to `fill` and every placed operand equals its CPU copy bit for bit.  A failure is a `GuardError` that names
  the allocation - its order, shape, dtype and the function that asked for it - and the first bad byte: `region` "front" with a
  negative offset from the payload's first byte, "rear" with the offset from the first byte AFTER the payload (0 = the byte
  that follows the payload's last), or "operand" with the offset into the payload.

THE RULE (`two_fills`).  A case runs under two fills, 0xFF and 0x5A.  0xFF.. is NaN in fp16, bf16 and fp32 and -1 in int32;
0x5A.. is a finite float in every type (fp16 0x5A5A = 203.25) and a large positive int32.  Each run must pass `check()`, and
the two results must be bit-identical to each other and to an unguarded call on the same operands, in every returned tensor:
an element left unwritten differs between the fills, and so does a value that leaked in from a band or a workspace field that
was assumed clean.

PLACEMENT (`shifted`).  A guard may be given a placement rule, `shift(dtype, kind, who)` -> bytes: the payload of that allocation
then starts at 256 k + shift instead of 256 k (`kind` is "operand" or "empty", `who` the function that asked, as `describe()`
prints it; the shift is a multiple of the element size and below 256).  No rule - the default - is a shift of 0: the payload
starts 256-byte aligned, as every guard test has it.  `min_placement(requirement)` turns a requirement in bytes,
`requirement(dtype, kind, who)` -> A (a power of two), into the rule "aligned to A and not to 2 A" (shift A; 0 for A >= 256).
THE SECOND RULE: `shifted(run, ..., requirement=)` takes the unguarded aligned call as the reference and runs `run(place)` under
each fill with every operand, output and workspace placed by `min_placement(requirement)`; both runs pass `check()` and both
results equal the reference bit for bit.  A kernel that rounds an address down to its vector width, takes its vector path from
the shape alone or assumes a 256-byte aligned base reads or writes other bytes at such a placement: the bands or the bits show it.

BAND.  At least the largest output tile any planned kernel stores, so that a whole misplaced tile still lands in a band.  The
planner's second-generation layouts (`conv_plan.cpp`: `pp_bn`, `plan_pp_3x3`, `plan_pp_1x1`, `match_gemm_plan`) are 224 pixels
x 256 channels and 448 pixels x 128 channels; the first generation's are 256 pixels (`BM`) x 64 channels.  The largest is
224 x 256 (= 448 x 128) elements of 2 bytes (fp16 / bf16) = 114688 bytes = 112 KiB; the split-K form stores fp32 partial sums
of 224 pixels x 128 channels x 4 bytes = 112 KiB as well.  BAND = 256 KiB per side covers either twice over.
"""
import contextlib
import sys

import numpy as np
import torch

FILLS = (0xFF, 0x5A)
LARGEST_TILE_BYTES = max(224 * 256 * 2, 448 * 128 * 2, 256 * 64 * 2, 224 * 128 * 4)      # see BAND above
BAND = 256 * 1024
assert BAND >= LARGEST_TILE_BYTES
ALIGN = 256


class GuardError(AssertionError):
    def __init__(self, msg, order, region, offset):
        super().__init__(msg)
        self.order, self.region, self.offset = order, region, offset


def _caller():
    """'module.function' of the nearest frame outside this file: the wrapper that asked for the allocation."""
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename == __file__:
        f = f.f_back
    if f is None:
        return "?"
    return "%s.%s" % (f.f_globals.get("__name__", "?").rsplit(".", 1)[-1], f.f_code.co_name)


def _shape(size):
    if len(size) == 1 and not isinstance(size[0], int):
        size = tuple(size[0])
    return tuple(int(v) for v in size)


def _bytes_of(t):
    """The bytes of a CPU tensor as a uint8 numpy array (bf16 has no numpy type: view through uint8)."""
    return t.detach().contiguous().reshape(-1).view(torch.uint8).numpy() if t.numel() else np.zeros(0, np.uint8)


class _Alloc:
    __slots__ = ("order", "raw", "off", "nbytes", "shape", "dtype", "who", "kind", "cpu")

    def describe(self):
        return "allocation #%d (%s %s %s, %d bytes, asked for by %s)" % (
            self.order, self.kind, list(self.shape), str(self.dtype).replace("torch.", ""), self.nbytes, self.who)


class Guard:
    def __init__(self, fill, band=BAND, device="cuda", shift=None):
        if not 0 <= int(fill) <= 255 or int(band) < 1:
            raise ValueError("Guard: fill is one byte, band at least one byte")
        self.fill, self.band, self.device = int(fill), int(band), torch.device(device)
        self.shift = shift                       # the placement rule (module docstring); None: every payload 256-byte aligned
        self.allocs = []

    # -------------------------------------------------------------------------------------------------------------------
    def _alloc(self, shape, dtype, kind, who):
        shape = _shape((shape,)) if not isinstance(shape, int) else (int(shape),)
        esize = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * esize
        shift = int(self.shift(dtype, kind, who)) if self.shift is not None else 0
        if not 0 <= shift < ALIGN or shift % esize:
            raise ValueError("Guard: a placement shift is a multiple of the element size in [0, %d), got %d for %s" % (ALIGN, shift, dtype))
        # (ALIGN - 1 spare bytes: the allocator's own alignment may be weaker than 256; they and the shift lengthen the front band)
        raw = torch.empty((self.band + nbytes + self.band + ALIGN - 1 + shift,), dtype=torch.uint8, device=self.device)
        raw.fill_(self.fill)
        off = self.band + (-(raw.data_ptr() + self.band)) % ALIGN + shift
        raw = raw[:off + nbytes + self.band]
        a = _Alloc()
        a.order, a.raw, a.off, a.nbytes, a.shape, a.dtype, a.who, a.kind, a.cpu = len(self.allocs), raw, off, nbytes, shape, dtype, who, kind, None
        self.allocs.append(a)
        payload = raw[off:off + nbytes].view(dtype).view(shape) if nbytes else torch.empty(shape, dtype=dtype, device=self.device)
        assert nbytes == 0 or payload.data_ptr() % ALIGN == shift
        return a, payload

    def empty(self, shape, dtype, who=None):
        """An output or workspace: the payload stays at `fill`."""
        return self._alloc(shape, dtype, "empty", who or _caller())[1]

    def place(self, cpu_tensor, who=None):
        """An operand: the payload is a copy of `cpu_tensor`, whose bytes `check()` compares it with."""
        t = cpu_tensor.detach().cpu().contiguous().clone()
        a, payload = self._alloc(tuple(t.shape), t.dtype, "operand", who or _caller())
        a.cpu = t
        if t.numel():
            payload.copy_(t)
        return payload

    # -------------------------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def patch(self, *modules):
        """The modules' `torch` attribute is the guard's proxy inside the block; undone on exit."""
        saved = [(m, m.torch) for m in modules]
        proxy = _TorchProxy(self)
        try:
            for m in modules:
                m.torch = proxy
            yield self
        finally:
            for m, t in saved:
                m.torch = t

    # -------------------------------------------------------------------------------------------------------------------
    def _sync(self):
        if self.device.type != "cuda":
            return
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            import pytest
            pytest.exit(f"guard: the GPU reported {e}; stopping the session", returncode=3)

    def _first_bad(self, region):
        bad = np.flatnonzero(region.cpu().numpy() != self.fill)
        return int(bad[0]) if bad.size else -1

    def check(self):
        self._sync()
        for a in self.allocs:
            end = a.off + a.nbytes
            front, rear = a.raw[:a.off], a.raw[end:]
            if bool((front != self.fill).any()):                               # the matching line for "before the payload"
                i = self._first_bad(front)
                raise GuardError("%s: front band written at offset %d (byte 0x%02X, fill 0x%02X)" % (
                    a.describe(), i - a.off, int(front[i]), self.fill), a.order, "front", i - a.off)
            if bool((rear != self.fill).any()):                                # the matching line for "after the payload"
                i = self._first_bad(rear)
                raise GuardError("%s: rear band written at offset %d past the payload's end (byte 0x%02X, fill 0x%02X)" % (
                    a.describe(), i, int(rear[i]), self.fill), a.order, "rear", i)
            if a.cpu is not None and a.nbytes:
                got, want = a.raw[a.off:end].cpu().numpy(), _bytes_of(a.cpu)
                if not np.array_equal(got, want):                              # the matching line for "operand modified"
                    i = int(np.flatnonzero(got != want)[0])
                    raise GuardError("%s: operand modified at offset %d (byte 0x%02X, was 0x%02X)" % (
                        a.describe(), i, int(got[i]), int(want[i])), a.order, "operand", i)


class _TorchProxy:
    """`torch` with the five allocating functions taken from a guard; every other attribute is `torch`'s own."""

    def __init__(self, guard):
        object.__setattr__(self, "_guard", guard)

    def __getattr__(self, name):
        return getattr(torch, name)

    def _mine(self, device):
        return device is not None and torch.device(device).type == self._guard.device.type

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._guard.empty(_shape(size), dtype or torch.get_default_dtype(), _caller())

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        t = self._guard.empty(_shape(size), dtype or torch.get_default_dtype(), _caller())
        return t.zero_() if t.numel() else t

    def full(self, size, fill_value, *, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.full(size, fill_value, dtype=dtype, device=device, **kw)
        if dtype is None:
            dtype = torch.bool if isinstance(fill_value, bool) else torch.int64 if isinstance(fill_value, int) else torch.get_default_dtype()
        t = self._guard.empty(_shape((size,)), dtype, _caller())
        return t.fill_(fill_value) if t.numel() else t

    def empty_like(self, t, *, dtype=None, device=None, **kw):
        device = t.device if device is None else device
        if not self._mine(device):
            return torch.empty_like(t, dtype=dtype, device=device, **kw)
        return self._guard.empty(tuple(t.shape), dtype or t.dtype, _caller())

    def zeros_like(self, t, *, dtype=None, device=None, **kw):
        device = t.device if device is None else device
        if not self._mine(device):
            return torch.zeros_like(t, dtype=dtype, device=device, **kw)
        out = self._guard.empty(tuple(t.shape), dtype or t.dtype, _caller())
        return out.zero_() if out.numel() else out


# -----------------------------------------------------------------------------------------------------------------------
# the rule
# -----------------------------------------------------------------------------------------------------------------------
def _flat(res):
    """Returned tensors as a flat list of CPU tensors (None kept); non-tensors (ints, flags) are kept as they are."""
    if isinstance(res, (tuple, list)):
        out = []
        for r in res:
            out.extend(_flat(r))
        return out
    return [res.detach().cpu() if isinstance(res, torch.Tensor) else res]


def first_difference(a, b):
    """None when two results hold the same bits, else a description of the first difference."""
    if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor):
        return None if (a is None and b is None) or (not isinstance(a, torch.Tensor) and not isinstance(b, torch.Tensor) and a == b) \
            else "%r against %r" % (type(a).__name__, type(b).__name__)
    if a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape):
        return "%s %s against %s %s" % (a.dtype, tuple(a.shape), b.dtype, tuple(b.shape))
    if a.numel() == 0:
        return None
    es = a.element_size()
    ba, bb = _bytes_of(a).reshape(-1, es), _bytes_of(b).reshape(-1, es)
    bad = np.flatnonzero((ba != bb).any(axis=1))
    if bad.size == 0:
        return None
    i = int(bad[0])
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(a.shape)))
    return "%d of %d elements differ, first at %s: %r against %r" % (bad.size, a.numel(), list(idx), a[idx].item(), b[idx].item())


def two_fills(run, modules=(), device="cuda", band=BAND, canon=None, what=""):
    """THE RULE.  `run(place)` launches the op with its operands moved by `place` (CPU tensor -> tensor on `device`) and returns
    a tensor or a (nested) tuple of tensors / None.  It runs unguarded (`place` = a plain copy to `device`), then under each fill with the
    `torch` of `modules` patched; each guarded run passes `check()`, and all three results hold the same bits, tensor by tensor.
    `canon`: applied to each flat list of CPU results before the comparison (an output order the header leaves open).
    Returns the unguarded result as a flat list of CPU tensors."""
    canon = canon or (lambda r: r)
    dev = torch.device(device)
    ref = run(lambda t: t.to(dev, copy=True))          # (a copy on the CPU as well: a kernel that writes its operand must not reach the caller's tensor)
    if dev.type == "cuda":
        Guard(0, 1, dev)._sync()
    ref = canon(_flat(ref))
    got = {}
    for fill in FILLS:
        g = Guard(fill, band, dev)
        with g.patch(*modules):
            res = run(g.place)
        g.check()
        got[fill] = canon(_flat(res))
        assert len(got[fill]) == len(ref), (what, "fill 0x%02X returned %d results, the unguarded call %d" % (fill, len(got[fill]), len(ref)))
    for k in range(len(ref)):
        d = first_difference(got[FILLS[0]][k], got[FILLS[1]][k])
        assert d is None, "%s: result %d differs between fill 0x%02X and fill 0x%02X (unwritten output, or a value read from " \
                          "outside the operands): %s" % (what, k, FILLS[0], FILLS[1], d)
        d = first_difference(got[FILLS[0]][k], ref[k])
        assert d is None, "%s: result %d of the guarded runs differs from the unguarded call: %s" % (what, k, d)
    return ref


# -----------------------------------------------------------------------------------------------------------------------
# the second rule: placement
# -----------------------------------------------------------------------------------------------------------------------
def min_placement(requirement):
    """The placement rule "aligned to A and not to 2 A" for A = `requirement(dtype, kind, who)` bytes (a power of two; an int
    serves for a constant): the payload starts at 256 k + A.  A >= 256 keeps the 256-byte aligned start (a guard cannot promise more)."""
    def shift(dtype, kind, who):
        a = int(requirement(dtype, kind, who)) if callable(requirement) else int(requirement)
        if a < 1 or a & (a - 1):
            raise ValueError("min_placement: a requirement is a power of two, got %d" % a)
        return a if a < ALIGN else 0
    return shift


def shifted(run, modules=(), device="cuda", band=BAND, canon=None, what="", requirement=16):
    """THE SECOND RULE.  `run(place)` as in `two_fills`.  The reference is the unguarded call (`place` = a plain copy to `device`:
    the allocator's own alignment).  Under each fill every operand `run` places, and every output and workspace the patched
    `modules` allocate, starts at the minimum alignment `requirement` gives it (`min_placement`); each run passes `check()` and
    its results hold the reference's bits, tensor by tensor.  Returns the reference as a flat list of CPU tensors."""
    canon = canon or (lambda r: r)
    dev = torch.device(device)
    ref = run(lambda t: t.to(dev, copy=True))
    if dev.type == "cuda":
        Guard(0, 1, dev)._sync()
    ref = canon(_flat(ref))
    for fill in FILLS:
        g = Guard(fill, band, dev, shift=min_placement(requirement))
        with g.patch(*modules):
            res = run(g.place)
        g.check()
        got = canon(_flat(res))
        assert len(got) == len(ref), (what, "fill 0x%02X returned %d results, the aligned call %d" % (fill, len(got), len(ref)))
        for k in range(len(ref)):
            d = first_difference(got[k], ref[k])
            assert d is None, "%s: result %d under fill 0x%02X, every buffer at its minimum alignment, differs from the aligned " \
                              "call: %s" % (what, k, fill, d)
    return ref
