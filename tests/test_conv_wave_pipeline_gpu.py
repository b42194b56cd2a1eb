"""The two start-up forms of the layer-1 kernel (`conv3x3_c64_wave_kernel<.., EARLY>`, `frmap_conv_wave_start`) compute the same bits.

Form 0 copies the weight slab piece by piece, passes the barrier and then issues the first tile's halo loads; form 1 (the
default) issues the first tile's halo loads and every piece of the slab at once.  Neither changes an operand, an MFMA or their
order, so every output of form 1 must be `torch.equal` to form 0's, in fp16 and bf16, with and without a residual, with ReLU.
On top of that the exact-integer instrument of `conv_cases.py` ({-1, 0, 1} operands, float64 reference, bit-equal) runs on the
three small shapes under both forms, and two shapes run between guard bands: the early loads of a wave that has no tile go
through an empty descriptor and must read nothing outside the input and write nothing.

Shapes (NHWC, Cin = Cout = 64 unless noted):
  1 x 8 x 8              one tile: seven waves of the only workgroup have none and leave after the barrier
  1 x 16 x 24            six tiles, one per wave, no second round: start-up loads and the final stores only
  3 x 8 x 8, Cout 128    two channel tiles (nt > 0): the second workgroup copies the second slab
  9 x 128 x 128          2304 tiles > 8 x CUs: waves run two rounds, the second one partial and dealt wave-major
  pool2 5 x 8 x 24 x 32  NCH = 1: half a slab, whose last piece only half the threads hold
  pool2 3 x 16 x 16 x 64 POOL with two chunks
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_cases as cc  # noqa: E402
import guard  # noqa: E402
from frmap_amd import _lib, ops  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]
OLD, NEW = 0, (1,)
WAVE = dict(tune=cc.PP_OFF, query=("conv3x3_pp", (0,)))      # first generation: Cin = 64 on 8-aligned maps is the wave kernel


def _case(name, B, H, W, Cout=64, res=False):
    return cc._c(name, cc.IG, "conv", B, H, W, 64, Cout, res=res, act=cc.ACT_RELU, **WAVE)


SMALL = [("one-tile", 1, 8, 8, 64), ("one-round", 1, 16, 24, 64), ("two-ntiles", 3, 8, 8, 128)]
MULTI = ("multi-round", 9, 128, 128, 64)
POOL_CASES = [cc._c("wp-pool-nch1", cc.IG, "pool2", 5, 8, 24, 32, 64, query=("pool2_form", (2,))),
              cc._c("wp-pool-c64", cc.IG, "pool2", 3, 16, 16, 64, 64, query=("pool2_form", (2,)))]


def _with_start(form, fn):
    lib = _lib.load()
    try:
        assert lib.frmap_conv_wave_start(form) == 0
        return fn()
    finally:
        lib.frmap_conv_wave_start(-1)


_operands = {}


def _float_operands(case, dtype):
    """Post-ReLU inputs, Gaussian weights and residual: computed once per (case, dtype), never modified."""
    key = (case.name, dtype)
    if key not in _operands:
        _operands[key] = cc.float_case_operands(case, "relu", dtype)
    return _operands[key]


def _assert_same_bits(case, dtype):
    o = _float_operands(case, dtype)
    d = cc.device_operands(case, o, dtype)
    want = _with_start(OLD, lambda: cc.launch_case(case, d, dtype))
    assert bool(torch.isfinite(want.float()).all()) and float(want.float().abs().max()) > 0, case.name
    for form in NEW:
        got = _with_start(form, lambda: cc.launch_case(case, d, dtype))
        diff = guard.first_difference(got.cpu(), want.cpu())
        assert diff is None, f"{case.name} {dtype}: start-up form {form} differs from form 0: {diff}"


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SMALL, ids=[s[0] for s in SMALL])
def test_small_shapes_same_bits(shape, dtype, res):
    name, B, H, W, Cout = shape
    _assert_same_bits(_case(f"wp-{name}-{int(res)}", B, H, W, Cout, res), dtype)


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_multi_round_same_bits(dtype, res):
    """More tiles than wave slots: every workgroup starts with eight tiles and runs a second, partial, wave-major round."""
    name, B, H, W, Cout = MULTI
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    total = B * (H // 8) * (W // 8)
    assert total > 8 * cus and total % (8 * cus) != 0, (total, cus)
    _assert_same_bits(_case(f"wp-{name}-{int(res)}", B, H, W, Cout, res), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", POOL_CASES, ids=[c.name for c in POOL_CASES])
def test_pool_forms_same_bits(case, dtype):
    """The NCH = 1 and POOL instantiations run the same body."""
    _assert_same_bits(case, dtype)


_exact = {}


def _exact_reference(case):
    if case.name not in _exact:
        o = cc.exact_case_operands(case)
        ref, S, act = cc.case_reference(case, o)
        cc.assert_exact_conditions(o, S, case.name)
        _exact[case.name] = (o, ref, act)
    return _exact[case.name]


@pytest.mark.parametrize("form", (OLD,) + NEW)
@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SMALL, ids=[s[0] for s in SMALL])
def test_small_shapes_exact_integers(shape, dtype, res, form):
    name, B, H, W, Cout = shape
    case = _case(f"wp-exact-{name}-{int(res)}", B, H, W, Cout, res)
    o, ref, act = _exact_reference(case)
    y = _with_start(form, lambda: cc.run_case(case, o, dtype))
    cc.assert_exact(y, ref, act, f"{case.name} start-up form {form}")


@pytest.mark.parametrize("form", NEW)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [SMALL[1], MULTI], ids=[SMALL[1][0], MULTI[0]])
def test_early_start_is_guarded(shape, dtype, form):
    """Both fill bytes; the residual form (every access the kernel can make)."""
    name, B, H, W, Cout = shape
    case = _case(f"wp-{name}-1", B, H, W, Cout, True)
    o = _float_operands(case, dtype)

    def run(place):
        return _with_start(form, lambda: cc.launch_case(case, cc.device_operands(case, o, dtype, place), dtype))

    guard.two_fills(run, [ops], what=f"{case.name} start-up form {form}")

