"""GPU: stream order and graph replay of the conv family (`stream_cases.py`).

Every entry of `conv_cases.CONV_CASES` and `CENSUS_CASES` (exact-integer operands, the fused-pool ops with their two-launch twin),
`GELU_CASES` (float operands) and `LINEAR_CASES`, in fp16 and bf16, under the late rule and the capture rule.  `cc.run_case` and
`cc.run_linear` wait for the device and read back with `.cpu()` inside the closure - nothing could be late when they return and
neither can be captured - so the closures here are built from `cc.device_operands` + `cc.launch_case(sync=False)` (and from
`ops.linear_mfma` as `cc.run_linear` calls it), which return device tensors: same operands, same path assertions, same launches.
The two weight packers are mirrored from `test_guard_conv_gpu.py` as they are.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_cases as cc  # noqa: E402
import stream_cases as sc  # noqa: E402
import test_guard_conv_gpu as tg  # noqa: E402
from frmap_amd import _lib, ops  # noqa: E402

DTYPES, DT_IDS = tg.DTYPES, tg.DT_IDS
MIRRORED = ["test_pack_conv_weight_is_guarded", "test_pack_conv_weight_c3_is_guarded"]
RULES = {"late": sc.late_rule, "captured": sc.capture_rule}

for _name in MIRRORED:
    globals()[_name.replace("_is_guarded", "_late")] = sc.mirror_late(tg, _name)
    globals()[_name.replace("_is_guarded", "_captured")] = sc.mirror_capture(tg, _name)


def _conv_run(case, o, dtype, also_unfused=False):
    return lambda place: cc.launch_case(case, cc.device_operands(case, o, dtype, place), dtype, also_unfused, sync=False)


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", cc.CONV_CASES + cc.CENSUS_CASES, ids=[c.name for c in cc.CONV_CASES + cc.CENSUS_CASES])
def test_conv_case(case, dtype, rule):
    o = cc.gpu_operands(case, "exact", dtype)
    RULES[rule](_conv_run(case, o, dtype, also_unfused=case.op in ("pool2", "c3pool2")), [ops], what=case.name)


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", cc.GELU_CASES, ids=[c.name for c in cc.GELU_CASES])
def test_gelu_case(case, dtype, rule):
    o = cc.gpu_operands(case, "gauss", dtype)
    RULES[rule](_conv_run(case, o, dtype), [ops], what=case.name)


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("lc", cc.LINEAR_CASES, ids=[c.name for c in cc.LINEAR_CASES])
def test_linear_case(lc, dtype, rule):
    """`cc.run_linear` without its wait and its read-back; the split-K cases take their workspace from the wrapper."""
    o = cc.linear_operands(lc, "gauss" if lc.act == cc.ACT_GELU else "exact", dtype)
    assert (_lib.load().frmap_linear_mfma_workspace_bytes(lc.M, lc.K, lc.N) > 0) == lc.split, (lc.name, "split-K")

    def run(place):
        wpk = ops.pack_conv_weight(place(o["w"].float().view(lc.N, lc.K, 1, 1)), dtype)
        r = place(o["r"].to(dtype)) if o.get("r") is not None else None
        return ops.linear_mfma(place(o["x"].to(dtype)), wpk, place(o["shift"].float()), lc.N, lc.act, r)
    RULES[rule](run, [ops], what=lc.name)


def test_stream_report(capsys):
    assert sc.CALLS["late"] > 0 and sc.CALLS["capture"] > 0
    with capsys.disabled():
        print("\n[test_stream_conv_gpu] " + sc.report(MIRRORED))
