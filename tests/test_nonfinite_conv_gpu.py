"""GPU: one non-finite element into every conv-family kernel; the rules of `poison.py` on what comes out ("Non-finite
values": no swallowing, no finite-but-wrong output, strict batch isolation, the receptive field and nothing else).

Every entry of `conv_cases.CONV_CASES`, `GELU_CASES`, `CENSUS_CASES` and `LINEAR_CASES`, fp16 and bf16, on the Gaussian operands of the bound family
(no weight is exactly zero: asserted).  A case runs once clean, then once per poison: every position of `poison.positions` in x
and, where the case has them, in the residual and in the fused shortcut's input.  The first-layer and stem cases (Cin = 3: one
case per kernel, and the home of the halos below) run all three kinds (NaN, +inf, -inf) at every position.  For the MFMA conv
cases, where several cases share a kernel family, the kind rotates with position, operand, case and type: a case stays at a handful
of launches and the (position, kind) pairs are covered across the table, not per case.  The fp16-only `overflow` kind has a test
of its own below.  The uint8 stem entries cannot carry a poison in the image: their `shift` is poisoned (first and last channel,
all three kinds), an operand all images share, so rule 3 is void there and the footprint is the channel.

Reference: `conv_cases`' float64 references on the poisoned operands, evaluated on the poisoned image alone (the references treat
images independently; rule 3 needs none).  Footprint: the same reference on a one-channel twin of the case (ones weights) with a
NaN at the poison's place.  Where the reference changes and stays finite - relu(-inf) = 0, a pool window that drops a -inf - the
element meets the bound family's one-rounding rule `|y - ref| <= u |ref| + c 2^-24 S` with S taken over the FINITE window members
only (a member that is exactly 0 or -inf contributes no rounding error), so relu(-inf) must be exactly 0; a fused conv + pool
must in addition hold the bits of the two-launch path on the same poisoned operands.

DECLARED HALOS (the first-layer kernels multiply real neighbouring pixels by zero pad weights: inf * 0 = NaN).  A non-finite
input pixel (iy, ix) may turn into NaN, besides its receptive field, the conv positions (and the pool windows holding one):
  conv_small_cin.hip 3x3 s1 (k = kh 16 + kw 4 + c, kw = 3 is the pad tap; the k >= 48 groups re-read row kh = 0, kw = 0 .. 3,
  under zero weights, so a pixel of that row turns its own output into NaN where the reference has +-inf):
      (oy, ox) with ox = ix - 2, oy in iy - 1 .. iy + 1, or oy = iy + 1, ox in ix - 2 .. ix + 1
  conv_small_cin.hip 7x7 s2 and stem_pool.hip (k = kh 32 + kw 4 + c, kw = 7 is the pad tap):
      (oy, ox) with 2 ox + 4 = ix, 2 oy - 3 <= iy <= 2 oy + 3
  stem_s2d.hip (4 x 4 super-pixels of 2 x 2: the taps kh = -1 and kw = -1 carry zero weights):
      (oy, ox) with 2 oy - 4 = iy, 2 ox - 4 <= ix <= 2 ox + 3, or 2 ox - 4 = ix, 2 oy - 4 <= iy <= 2 oy + 3
Every halo lies in the poison's own image (the staged rows of another image are never a pad tap's target: the 3x3 kernel sends
its k >= KTOT groups to row kh = 0 of the SAME pixel); rule 3 is checked without exception and settles it.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_cases as cc  # noqa: E402
import guard  # noqa: E402
import poison  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]
ALL_CASES = cc.CONV_CASES + cc.GELU_CASES + cc.CENSUS_CASES      # (appended: the kind rotation of the earlier entries stays)
POOL_OF = {"pool2": (2, 2, 0), "c3pool2": (2, 2, 0), "stem3": (3, 2, 1), "stem2": (2, 2, 0), "stem3u8": (3, 2, 1), "stem2u8": (2, 2, 0)}


def _reference(case, o):
    """(want, S_eff): the float64 activation (pooled where the op pools) and the magnitude sum of the one-rounding rule, taken over
    the finite members only (module docstring).  Mirrors `conv_cases.case_reference`."""
    if case.op == "ds":
        ref, S = cc.conv_shortcut_ref(o["x"], o["w"], o["shift"], o["xd"], o["wd"], case.ds[1])
    else:
        ref, S = cc.conv_ref(o["x"], o["w"], o["shift"], case.stride, cc.case_pad(case), o.get("r"))
    S = torch.where(torch.isfinite(S), S, torch.zeros_like(S))
    if case.op in POOL_OF:
        act = case.act if case.op in ("pool2", "c3pool2") else cc.ACT_RELU
        return cc.pooled(ref, S, act, *POOL_OF[case.op])
    return cc.act64(ref, case.act), S


def _image(o, b):
    """Operand dict of image b alone."""
    return {k: (v[b:b + 1] if k in ("x", "r", "xd") and v is not None else v) for k, v in o.items()}


def _twin(case, o, operand, index):
    """One-channel twin of the case (ones weights, zero shift) with a NaN at the poison's spatial place: its NaN outputs are the
    receptive field, [1, 1, Ho, Wo]."""
    t = {"x": torch.zeros((1, 1) + tuple(o["x"].shape[2:]), dtype=torch.float64), "w": torch.ones((1, 1, case.k, case.k), dtype=torch.float64),
         "shift": torch.zeros(1), "r": None}
    if o.get("r") is not None:
        t["r"] = torch.zeros((1, 1) + tuple(o["r"].shape[2:]), dtype=torch.float64)
    if o.get("xd") is not None:
        t["xd"], t["wd"] = torch.zeros((1, 1) + tuple(o["xd"].shape[2:]), dtype=torch.float64), torch.ones((1, 1, 1, 1), dtype=torch.float64)
    t[operand][0, 0, index[2], index[3]] = math.nan
    return poison.nan_footprint(_reference(case, t)[0])


def _field(n_out, stride, lo, hi, i):
    """bool [n_out]: outputs o whose input span o stride + lo .. o stride + hi holds input coordinate i."""
    o = torch.arange(n_out) * stride
    return (o + lo <= i) & (i <= o + hi)


def _halo(case, o, index):
    """The declared halo of a non-finite pixel (iy, ix) of x, as bool [1, 1, Ho, Wo] of the case's output, or None."""
    if case.Cin != 3:
        return None
    H, W = o["x"].shape[2:]
    iy, ix = index[2], index[3]
    Hc, Wc = cc._out_hw(H, W, case.k, case.stride, cc.case_pad(case))
    if case.k == 3:                                       # conv_small_cin.hip 3x3
        conv = (_field(Hc, 1, -1, 1, iy).view(-1, 1) & _field(Wc, 1, 2, 2, ix).view(1, -1)) | \
               (_field(Hc, 1, -1, -1, iy).view(-1, 1) & _field(Wc, 1, -1, 2, ix).view(1, -1))
    elif case.op == "stem3" and W % 4 == 0:               # stem_s2d.hip
        rows_ext, cols_ext = _field(Hc, 2, -4, 3, iy).view(-1, 1), _field(Wc, 2, -4, 3, ix).view(1, -1)
        conv = (_field(Hc, 2, -4, -4, iy).view(-1, 1) & cols_ext) | (rows_ext & _field(Wc, 2, -4, -4, ix).view(1, -1))
    else:                                                 # conv_small_cin.hip 7x7 s2, stem_pool.hip: 2 ox + 4 = ix
        conv = _field(Hc, 2, -3, 3, iy).view(-1, 1) & _field(Wc, 2, 4, 4, ix).view(1, -1)
    conv = conv.view(1, 1, Hc, Wc)
    if case.op in POOL_OF:
        return cc.window_max(conv.double(), *POOL_OF[case.op]) > 0
    return conv


def _finite_rule(S, dtype, lip):
    def ok(got, want, mask):
        bound = cc.UNIT[dtype] * want.abs() + lip * cc.C_ACC * cc.EPS32 * S
        return ~mask | ((got.double() - want).abs() <= bound)
    return ok


def _run(case, o, dtype):
    """(output, two-launch output or None) as CPU NCHW tensors."""
    fused_pool = case.op in ("pool2", "c3pool2")
    res = cc.run_case(case, o, dtype, also_unfused=fused_pool)
    return res if fused_pool else (res, None)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_conv_case_propagates(case, dtype):
    o = cc.gpu_operands(case, "gauss", dtype)
    ci, di = ALL_CASES.index(case), DTYPES.index(dtype)
    for key in ("w", "wd"):
        if o.get(key) is not None:           # (a few of 2.4 M fp16 weights of N(0, 2 / (9 * 512)) round to zero: give them a value)
            o[key] = torch.where(o[key] == 0, torch.full_like(o[key], 2.0 ** -10), o[key])
            poison.assert_no_zero(o[key], (case.name, key))
    lip = cc.GELU_LIP if case.act == cc.ACT_GELU else 1.0
    got_c, _ = _run(case, o, dtype)
    clean = {}

    def clean_ref(b):
        if b not in clean:
            clean[b] = _reference(case, _image(o, b) if b is not None else o)
            poison.assert_fp32_safe(clean[b][1], case.name)
            assert bool(torch.isfinite(clean[b][0]).all()), case.name
        return clean[b][0]

    if case.op.endswith("u8"):                            # the image is bytes: poison the shift, which every image shares
        runs = [("shift", "ch%d" % c, (c,), None) for c in (0, case.Cout - 1)]
    else:
        runs = [(op, name, idx, idx[0]) for op in ("x", "r", "xd") if o.get(op) is not None for name, idx in poison.positions(o[op].shape)]
    every_kind = case.Cin == 3                            # first layers and stems: one case per kernel, the halo logic lives here
    runs = [(ri, r, k) for ri, r in enumerate(runs) for k in (poison.KINDS if every_kind else (poison.KINDS[(ri + ci + di) % 3],))]
    for ri, (operand, pname, idx, b), kind in runs:
        what = "%s %s: %s at %s %s of %s" % (case.name, DT_IDS[di], kind, pname, list(idx), operand)
        op_ = dict(o)
        op_[operand] = poison.poisoned(o[operand], idx, poison.poison_value(kind))
        got_p, got_p2 = _run(case, op_, dtype)
        want_p, S = _reference(case, _image(op_, b) if b is not None else op_)
        if operand == "shift":
            foot = torch.zeros(want_p.shape, dtype=torch.bool)
            foot[:, idx[0]] = True
            halo = None
        else:
            foot = _twin(case, o, operand, idx)
            if operand == "r":                            # a residual element reaches its own channel only
                one = torch.zeros(want_p.shape, dtype=torch.bool)
                one[0, idx[1]] = foot[0, 0]
                foot = one
            halo = _halo(case, o, idx) if operand == "x" else None
        poison.compare(got_c, got_p, clean_ref(b), want_p, foot, image=b, halo=halo, finite_ok=_finite_rule(S, dtype, lip), what=what)
        if got_p2 is not None:
            d = guard.first_difference(got_p, got_p2)
            assert d is None, "%s: the fused conv + pool differs from the two-launch path on the poisoned operands: %s" % (what, d)


OVERFLOW_CASES = [c for c in cc.CONV_CASES + cc.CENSUS_CASES if not c.op.endswith("u8")]
OVERFLOW_X, OVERFLOW_W = 32768.0, 8.0


@pytest.mark.parametrize("case", OVERFLOW_CASES, ids=[c.name for c in OVERFLOW_CASES])
def test_conv_case_overflows_fp16(case):
    """The `overflow` kind (fp16 only): a FINITE operand whose products leave fp16's range.  No single fp16 element can do that
    under the Gaussian weights (|w| < 1, |x| <= 65504), so this runs on the exact-integer family with its weights times 8:
    x, w / 8 in {-1, 0, 1}, and x = 32768 at the centre of the middle image of x, then at the first element of the fused
    shortcut's input.  (Not in the residual: it is added with weight 1, and no fp16 value reaches 2 x 65504.)  Every output that sees the element through a nonzero weight is +-262144 plus an integer of magnitude <= 8 * 165 + 16, at least
    2 x 65504: +-inf in fp16 whatever the order of the fp32 sums; every other output is an integer <= 1336, far below 0.5 x 65504,
    exact in fp16 (`poison.overflow_ok` asserts both on the reference).  So every comparison is exact: inf where the reference
    overflows, relu(-262144) = 0, the rounded reference elsewhere in the receptive field, the clean run's bits everywhere else."""
    dtype = torch.float16
    o = cc.exact_case_operands(case)
    for key in ("w", "wd"):
        if o.get(key) is not None:
            o[key] = o[key] * OVERFLOW_W
    got_c, _ = _run(case, o, dtype)
    for operand in [k for k in ("x", "xd") if o.get(k) is not None]:
        name, idx = poison.positions(o[operand].shape)[-1 if operand == "x" else 0]      # (the stride-2 shortcut samples even pixels only)
        b = idx[0]
        what = "%s fp16: %s (%g) at %s %s of %s" % (case.name, poison.OVERFLOW, OVERFLOW_X, name, list(idx), operand)
        op_ = dict(o)
        op_[operand] = poison.poisoned(o[operand], idx, OVERFLOW_X)
        want_c, S_c = _reference(case, _image(o, b))
        want_p, _ = _reference(case, _image(op_, b))
        assert float(S_c.max()) <= OVERFLOW_W * cc.S_MAX_EXACT, what
        pre = cc.conv_shortcut_ref(op_["x"][b:b + 1], op_["w"], op_["shift"], op_["xd"][b:b + 1], op_["wd"], case.ds[1])[0] if case.op == "ds" else \
            cc.conv_ref(op_["x"][b:b + 1], op_["w"], op_["shift"], case.stride, cc.case_pad(case), op_["r"][b:b + 1] if op_.get("r") is not None else None)[0]
        poison.overflow_ok(pre, what)                      # (on the pre-activation: a ReLU or a pool only drops members)
        got_p, got_p2 = _run(case, op_, dtype)
        poison.compare(got_c, got_p, want_c, want_p, _twin(case, o, operand, idx), image=b, what=what)
        if got_p2 is not None:
            d = guard.first_difference(got_p, got_p2)
            assert d is None, "%s: the fused conv + pool differs from the two-launch path: %s" % (what, d)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("lc", cc.LINEAR_CASES, ids=[c.name for c in cc.LINEAR_CASES])
def test_linear_case_propagates(lc, dtype):
    """`linear_mfma` (split-K and not): a row is an image."""
    o = cc.linear_operands(lc, "gauss", dtype)
    li, di = cc.LINEAR_CASES.index(lc), DTYPES.index(dtype)
    poison.assert_no_zero(o["w"], lc.name)
    lip = cc.GELU_LIP if lc.act == cc.ACT_GELU else 1.0

    def reference(ops_, b):
        ref, S = cc.linear_ref(ops_["x"][b:b + 1], ops_["w"], ops_["shift"], ops_["r"][b:b + 1] if ops_["r"] is not None else None)
        return cc.act64(ref, lc.act), torch.where(torch.isfinite(S), S, torch.zeros_like(S))

    got_c = cc.run_linear(lc, o, dtype)
    runs = [(op, name, idx) for op in ("x", "r") if o.get(op) is not None for name, idx in poison.positions(o[op].shape)]
    for ri, (operand, pname, idx) in enumerate(runs):
        kind = poison.KINDS[(ri + li + di) % 3]
        what = "%s %s: %s at %s %s of %s" % (lc.name, DT_IDS[di], kind, pname, list(idx), operand)
        op_ = dict(o)
        op_[operand] = poison.poisoned(o[operand], idx, poison.poison_value(kind))
        got_p = cc.run_linear(lc, op_, dtype)
        want_c, S_c = reference(o, idx[0])
        poison.assert_fp32_safe(S_c, lc.name)
        want_p, S = reference(op_, idx[0])
        foot = torch.ones(want_p.shape, dtype=torch.bool)
        if operand == "r":
            foot = torch.zeros(want_p.shape, dtype=torch.bool)
            foot[0, idx[1]] = True
        poison.compare(got_c, got_p, want_c, want_p, foot, image=idx[0], finite_ok=_finite_rule(S, dtype, lip), what=what)
