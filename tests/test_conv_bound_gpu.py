"""GPU: every conv kernel variant against the float64 reference of `conv_cases.py` under the one-rounding rule

    |y - act(ref)| <= u |act(ref)| + C_ACC 2^-24 S        u = 2^-11 (fp16), 2^-8 (bf16), C_ACC = 8 (GELU: the second term x 1.13)

with S the same op on the absolute values of the operands.  The first term is the single final rounding `conv_epilogue` promises,
the second the allowance for fp32 accumulation, set from CPU restatements in `test_conv_cpu.py` and never from a kernel.  The rule
rejects an accumulator rounded to the storage dtype per chunk, split-K halves merged through the storage dtype, an output rounded
before the residual is added and tanh-GELU in place of erf-GELU (each misses by >= 2 x on the CPU emulation).

Every case runs Gaussian inputs and post-ReLU inputs (non-negative, non-zero mean: what the layers really see); one case per kernel
file also runs the fp16 pair x 2^12 / w 2^-12, whose weights are subnormal (MFMA must not flush them).  Each test prints
`CONVBOUND <kernel file> <dtype> <case> <inputs> <worst fraction of the bound>` before it asserts.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_cases as cc  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]


def _check(case, family, dtype):
    o = cc.gpu_operands(case, family, dtype)
    want, S, act = cc.case_reference(case, o)
    y = cc.run_case(case, o, dtype)
    assert y.dtype == dtype
    lip = cc.GELU_LIP if act == cc.ACT_GELU else 1.0
    print(f"CONVBOUND {case.file} {str(dtype)[6:]} {case.name} {family} "
          f"{cc.one_rounding_ratio(y, cc.act64(want, act), S, dtype, lip) if tuple(y.shape) == tuple(want.shape) else float('nan'):.3f}")
    return cc.assert_one_rounding(y, want, S, dtype, act, f"{case.file} {case.name} {family} {str(dtype)[6:]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", [c.name for c in cc.CONV_CASES + cc.GELU_CASES + cc.CENSUS_CASES])
def test_conv_one_rounding(name, dtype):
    case = cc.case_by_name(name)
    for family in ("gauss", "relu"):
        _check(case, family, dtype)


@pytest.mark.parametrize("name", cc.SUBNORMAL_CASES)
def test_conv_subnormal_fp16_weights(name):
    """x 2^12 and w 2^-12: the same products as the Gaussian case with most weights below fp16's smallest normal number.  The rule
    applies unchanged (the reference uses the rounded operands); a kernel or a weight pack that flushes subnormals loses them all."""
    _check(cc.case_by_name(name), "subnormal", torch.float16)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", [c.name for c in cc.LINEAR_CASES])
def test_linear_mfma_one_rounding(name, dtype):
    lc = next(c for c in cc.LINEAR_CASES if c.name == name)
    for family in ("gauss", "relu") + (("subnormal",) if dtype == torch.float16 and name == "linear-res" else ()):
        o = cc.linear_operands(lc, family, dtype)
        ref, S = cc.linear_ref(o["x"], o["w"], o["shift"], o["r"])
        y = cc.run_linear(lc, o, dtype)
        print(f"CONVBOUND linear_mfma {str(dtype)[6:]} {name} {family} "
              f"{cc.one_rounding_ratio(y, cc.act64(ref, lc.act), S, dtype, cc.GELU_LIP if lc.act == cc.ACT_GELU else 1.0):.3f}")
        cc.assert_one_rounding(y, ref, S, dtype, lc.act, f"linear_mfma {name} {family} {str(dtype)[6:]}")
