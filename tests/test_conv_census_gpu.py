"""GPU: the same-bits pairs of the census table (`conv_cases.CENSUS_SAME_BITS`) and the hooks afterwards.

The census cases themselves (`conv_cases.CENSUS_CASES`: one sharp case per kernel instantiation the older tables do not reach, and
the FRMAP_PP_IM / FRMAP_PP_PITCH options on every layout) run where every conv case runs: exact integers
(`test_conv_exact_gpu.py`), the one-rounding bound (`test_conv_bound_gpu.py`), guard bands (`test_guard_conv_gpu.py`) and non-finite
propagation (`test_nonfinite_conv_gpu.py`); `launch_case` asserts the instantiation each one launches (`ops.conv_plan_key`) on this
device's CU count.  Here: two placements of one computation - the LDS-DMA issued between the MFMAs or in the LOAD segments, the
halo rows at the conflict-free pitch or at Wi + 2, fragment reads interleaved or in a burst on a split-K layout where the request
is honoured, the 224 px x 256 ch layout against 448 px x 128 ch - must store the same bits, on exact-integer operands (where the
bits are also the float64 reference's) and on Gaussian ones (where a changed k order would show).  `torch.equal` is the bar.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_cases as cc  # noqa: E402
import guard  # noqa: E402
from frmap_amd import _lib, ops  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]


def _pair(a, b):
    ca, cb = cc.case_by_name(a), cc.case_by_name(b)
    assert (ca.op, ca.B, ca.H, ca.W, ca.Cin, ca.Cout, ca.k, ca.stride, ca.ds) == (cb.op, cb.B, cb.H, cb.W, cb.Cin, cb.Cout, cb.k, cb.stride, cb.ds)
    assert ca.key is not None and cb.key is not None, (a, b)
    return ca, cb._replace(res=ca.res, act=ca.act)      # the second case on the first one's operands and epilogue


@pytest.mark.parametrize("family", ["exact", "gauss"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("a,b", cc.CENSUS_SAME_BITS, ids=["%s=%s" % p for p in cc.CENSUS_SAME_BITS])
def test_census_pairs_store_the_same_bits(a, b, dtype, family):
    ca, cb = _pair(a, b)
    o = cc.gpu_operands(ca, family, dtype)
    ya, yb = cc.run_case(ca, o, dtype), cc.run_case(cb, o, dtype)
    want, S, act = cc.case_reference(ca, o)
    what = f"{a} {str(dtype)[6:]} {family}"
    if family == "exact":
        cc.assert_exact(ya, want, act, what)
    else:
        cc.assert_one_rounding(ya, want, S, dtype, act, what)
    d = guard.first_difference(ya.contiguous(), yb.contiguous())
    assert torch.equal(ya, yb), f"{what}: {ca.key} and {cb.key} ({b}) differ: {d}"


def test_the_declined_request_runs_the_burst_read_kernel():
    """`pp-splitk-ri1` asks for interleaved reads at six halo pieces; the planner declines, and its launch is `pp-splitk-ri0`'s."""
    a, b = cc.case_by_name("pp-splitk-ri0"), cc.case_by_name("pp-splitk-ri1")
    assert (a.ri, b.ri) == (0, 1) and cc.planned_key(a) == cc.planned_key(b) == a.key == b.key == "conv3x3_pp_kernel<7,2,6,2>"


def test_every_hook_is_back_at_its_default():
    """After the cases above no hook is left set: default queries answer as planned, the options that are off by default are off."""
    lib = _lib.load()
    assert lib.frmap_conv3x3_pp_tile_px(256, 14, 14, 256, 256, 1, 0, 0, 0, 0) == 196      # 224 x 256: not filled
    assert lib.frmap_conv3x3_pp_layout(256, 14, 14, 256, 256) == 1
    # IM, RI and pitch off, the shortcut form on, the wave kernel's early start on
    assert ops.conv_plan_key(256, 14, 14, 256, 256) == "conv3x3_pp_kernel<7,2,3,1>"
    assert ops.conv_plan_key(256, 14, 14, 256, 256, fuse=ops.FUSE_SHORTCUT, ds=(28, 28, 128, 2)) == "conv3x3_pp_kernel<7,2,3,1,DS>"
    assert ops.conv_plan_key(256, 56, 56, 64, 64) == "conv3x3_c64_wave_kernel<2,EARLY>"
    # pitch: 20x12 maps in 216-pixel tiles have 21 halo rows, 18.4 KB at Wp = 14 (three 8 KB pieces) and 26.3 KB at the
    # conflict-free pitch of 20 (NHP class 5): the key tells the two apart
    assert ops.conv_plan_key(256, 20, 12, 128, 256) == "conv3x3_pp_kernel<7,2,3,1>"
    assert cc.planned_key(cc._c("pitch-on", cc.PP, "conv", 256, 20, 12, 128, 256, pitch=1)) == "conv3x3_pp_kernel<7,2,5,1>"
    assert ops.conv_plan_key(256, 20, 12, 128, 256) == "conv3x3_pp_kernel<7,2,3,1>"
