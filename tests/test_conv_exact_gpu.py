"""GPU: every conv kernel variant on exact-integer operands (`conv_cases.py`): inputs and weights in {-1, 0, 1}, shift and residual
integers in [-8, 8], S <= 256, so that every partial sum in any order, chunking or split-K merge is an integer that fp32, fp16 and
bf16 all hold exactly.  The output must equal the float64 reference bit for bit: a dropped (tap, cin) product, a wrong padding, a
wrong pixel or channel index or a stale LDS slab moves an output by at least 1.

Covers conv_igemm.hip (wave-autonomous, register-prefetch, generic, stride-2 split and its odd-height fallback, the 1x1 kernels,
Linear as 1x1, the first-generation fused shortcut, the fused 2x2 pool's generic and wave forms, linear_mfma with and without
split-K), conv_pp.hip (3x3 with 128 / 256-channel tiles and split-K, interleaved reads on and off, a forced tile of 37 pixels, one
32-channel chunk; stride 2; fused shortcut; 1x1 layouts 1 / 2 / 3, one k-step, an odd k-step count; the fused pool), conv_small_cin.hip,
stem_pool.hip and stem_s2d.hip (fp32 and uint8 entries), each with its path asserted where the library has a query for it, and
the census table (`conv_cases.CENSUS_CASES`: every instantiation the cases above do not reach), each with the kernel instantiation
it launches asserted by name (`ops.conv_plan_key`).  Where two
generations, two layouts or a fused and a two-launch path compute the same layer, their outputs must also agree bit for bit.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_cases as cc  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", [c.name for c in cc.CONV_CASES + cc.CENSUS_CASES])
def test_conv_exact_integers(name, dtype):
    case = cc.case_by_name(name)
    o = cc.gpu_operands(case, "exact", dtype)
    want, S, act = cc.case_reference(case, o)
    assert float(S.max()) <= cc.S_MAX_EXACT
    what = f"{case.file} {name} {str(dtype)[6:]}"
    if case.op in ("pool2", "c3pool2"):
        y, y2 = cc.run_case(case, o, dtype, also_unfused=True)
        cc.assert_exact(y2, want, act, what + " (conv, then maxpool)")
    else:
        y = cc.run_case(case, o, dtype)
    assert y.dtype == dtype
    cc.assert_exact(y, want, act, what)
    if case.op in ("pool2", "c3pool2"):
        assert torch.equal(y, y2), (what, "fused and two-launch paths differ")
    if case.op.endswith("u8"):      # the uint8 entry against the fp32 entry on the table's values
        twin = case._replace(op=case.op[:-2])
        assert torch.equal(y, cc.run_case(twin, o, dtype)), (what, "uint8 and fp32 entries differ")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("a,b", cc.SAME_BITS)
def test_conv_paths_agree_bit_for_bit(a, b, dtype):
    """Two generations / layouts / read placements of one layer on the same exact operands: identical bits, and the right ones."""
    ca, cb = cc.case_by_name(a), cc.case_by_name(b)
    assert (ca.B, ca.H, ca.W, ca.Cin, ca.Cout, ca.k, ca.stride, ca.ds) == (cb.B, cb.H, cb.W, cb.Cin, cb.Cout, cb.k, cb.stride, cb.ds)
    o = cc.gpu_operands(ca, "exact", dtype)
    if o["r"] is not None and not cb.res:
        o["r"] = None
    ca, cb = ca._replace(res=o["r"] is not None, act=cc.ACT_RELU), cb._replace(res=o["r"] is not None, act=cc.ACT_RELU)
    ya, yb = cc.run_case(ca, o, dtype), cc.run_case(cb, o, dtype)
    want, _, act = cc.case_reference(ca, o)
    cc.assert_exact(ya, want, act, f"{a} {str(dtype)[6:]}")
    assert torch.equal(ya, yb), (a, b, dtype, int((ya != yb).sum()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", [c.name for c in cc.LINEAR_CASES if c.act != cc.ACT_GELU])
def test_linear_mfma_exact_integers(name, dtype):
    """`linear_mfma` with the fp32 slabs of split-K (from K = 256 on: the smallest K the dispatcher splits) and without."""
    lc = next(c for c in cc.LINEAR_CASES if c.name == name)
    o = cc.linear_operands(lc, "exact", dtype)
    ref, S = cc.linear_ref(o["x"], o["w"], o["shift"], o["r"])
    assert float(S.max()) <= cc.S_MAX_EXACT
    cc.assert_exact(cc.run_linear(lc, o, dtype), ref, lc.act, f"linear_mfma {name} {str(dtype)[6:]}")
