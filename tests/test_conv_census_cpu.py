"""CPU: the census of conv kernel instantiations.  Every instantiation the launchers can dispatch has a key
(`ops.conv_plan_keys`, csrc/conv_plan.cpp: KEY_ROWS); the launchers dispatch through tables of {key, bf16 kernel, fp16 kernel}.
This file runs the planner (no GPU) on every conv-family case of every GPU case table, under the case's own hooks, and holds that

* the library's self-check passes: every key selects a plan that has this key, both data types have a kernel of their own for it;
* every case that names a key gets that key from the planner, and every conv-family case of the sharp tables names one;
* the keys reached by the EXACT-INTEGER family (`test_conv_exact_gpu.py`: CONV_CASES + CENSUS_CASES) are all keys that exist, minus
  EXACT_EXCLUSIONS, which may name no second-generation kernel; the same for the ONE-ROUNDING family, whose tables run in fp16 and
  in bf16 alike (`test_conv_bound_gpu.py`: CONV_CASES + GELU_CASES + CENSUS_CASES; `test_conv_fill_gpu.py`);
* the operands of every census case meet the conditions that make the two instruments sharp: S <= 256 with every (tap, cin)
  position in at least two channels, and the `slack <= 1` condition of `assert_one_rounding` on the float64 reference.

The planner's inputs here are 256 CUs (what the library assumes without a device) and the default environment; what holds on the
device is `launch_case`'s assertion of the same key just before each launch.  The test prints the table key -> cases (DESIGN.md,
"Census of conv instantiations").
"""
import os

import pytest
import torch

import big_cases as bc
import conv_cases as cc
import test_conv_fill_gpu as fill
from frmap_amd import _lib, ops

# keys no exact-integer case runs, each with its reason.  (GELU is an argument of the epilogue, not an instantiation: no key is
# GELU-only.  The wave kernel's start-up form 0 runs exact cases of its own in the census table.)
EXACT_EXCLUSIONS = {}
BOUND_EXCLUSIONS = {}
SECOND_GENERATION = ("conv3x3_pp_kernel", "conv3x3s2_pp_kernel", "conv1x1_pp_kernel")


@pytest.fixture(scope="module", autouse=True)
def default_environment():
    assert _lib.lib_available(), "libfrmap_hip.so not built (run __graft_entry__.build())"
    set_ = sorted(k for k in os.environ if k.startswith(("FRMAP_CONV_", "FRMAP_PP_", "FRMAP_POOL_", "FRMAP_WAVE_", "FRMAP_DS_", "FRMAP_BATCH_")))
    assert not set_, ("the census is about the planner's default environment", set_)


def _conv(cases):
    return [c for c in cases if c.op in cc.CONV_OPS]


@pytest.fixture(scope="module")
def census():
    """[(table, case name, planned key)] of every conv-family case, in table order; the fill table with both of its runs."""
    rows = []
    for table, cases in (("CONV_CASES", cc.CONV_CASES), ("GELU_CASES", cc.GELU_CASES), ("CENSUS_CASES", cc.CENSUS_CASES)):
        rows += [(table, c.name, cc.planned_key(c)) for c in _conv(cases)]
    for entry in fill.FILL_CASES:
        first, aligned = fill.fill_runs(entry)
        rows += [("FILL_CASES", first.name, cc.planned_key(first)), ("FILL_CASES aligned", aligned.name, cc.planned_key(aligned))]
    for case, _, kernel in bc.BIG_CONV:
        if case.op in cc.CONV_OPS:
            rows.append(("BIG_CONV", case.name, cc.planned_key(case._replace(B=bc.conv_batch(case)))))
    return rows


def _reached(census, tables):
    return {key for table, _, key in census if table in tables}


def test_keys_and_the_launch_tables_agree():
    keys = ops.conv_plan_keys()
    assert len(keys) == len(set(keys)) == 52, len(keys)
    ops.conv_plan_selfcheck()
    for family, n in (("conv_igemm_kernel", 7), ("conv1x1_kernel", 3), ("conv3x3_c64_wave_kernel", 6), ("conv3x3_fast_kernel", 2),
                      ("conv3x3s2_split_kernel", 1), ("conv3x3s2_fast_kernel", 1), ("conv3x3_pp_kernel", 24), ("conv3x3s2_pp_kernel", 5),
                      ("conv1x1_pp_kernel", 3)):
        assert sum(k.split("<")[0] == family for k in keys) == n, family


def test_the_query_refuses_what_the_launchers_refuse():
    assert ops.conv_plan_key(1, 8, 8, 48, 64) == "" and b"Cin=48" in _lib.load().frmap_last_error()
    assert ops.conv_plan_key(1, 7, 7, 64, 64, fuse=ops.FUSE_POOL2) == ""            # odd sizes: no pooled form
    assert ops.conv_plan_key(1, 8, 8, 64, 64, k=5) == ""
    with pytest.raises(ValueError):
        ops.conv_plan_key(1, 8, 8, 64, 64, fuse=4)
    with pytest.raises(ValueError):
        ops.conv_plan_key(1, 8, 8, 64, 64, stride=2, fuse=ops.FUSE_POOL2)


def test_every_case_gets_the_key_it_names(census):
    named = {}
    for cases in (cc.CONV_CASES, cc.GELU_CASES, cc.CENSUS_CASES):
        for c in cases:
            assert (c.key is not None) == (c.op in cc.CONV_OPS), (c.name, "conv-family cases name their key, the others have none")
            named[c.name] = c.key
    for entry in fill.FILL_CASES:
        first, aligned = fill.fill_runs(entry)
        named[first.name] = first.key
        named[("aligned", aligned.name)] = aligned.key
    keys = set(ops.conv_plan_keys())
    for table, name, key in census:
        assert key in keys, (table, name, key)
        if table == "BIG_CONV":
            kernel = next(k for c, _, k in bc.BIG_CONV if c.name == name)
            assert key.split("<")[0] == kernel, (name, key, kernel)
        else:
            want = named[("aligned", name) if table == "FILL_CASES aligned" else name]
            assert want is not None and key == want, (table, name, "the planner says", key, "the table says", want)
    assert len({c.name for c in cc.CONV_CASES + cc.GELU_CASES + cc.CENSUS_CASES}) == len(cc.CONV_CASES + cc.GELU_CASES + cc.CENSUS_CASES)


def test_the_declined_request_keeps_the_burst_read_kernel():
    """Interleaved reads at six split-K halo pieces would spill: `pp-splitk-ri1` gets the key of `pp-splitk-ri0`; at four pieces the
    request is honoured."""
    a, b = cc.case_by_name("pp-splitk-ri0"), cc.case_by_name("pp-splitk-ri1")
    assert (a.ri, b.ri) == (0, 1) and cc.planned_key(a) == cc.planned_key(b) == "conv3x3_pp_kernel<7,2,6,2>"
    assert cc.planned_key(cc.case_by_name("cx-splitk4-ri1")) == "conv3x3_pp_kernel<7,2,4,2,RI>"


def test_sharp_cases_reach_every_instantiation(census):
    keys = set(ops.conv_plan_keys())
    by_key = {}
    for table, name, key in census:
        by_key.setdefault(key, []).append(name + {"FILL_CASES": " (fill)", "FILL_CASES aligned": " (fill, aligned)", "BIG_CONV": " (big)"}.get(table, ""))
    print("\nkey -> cases")
    for key in ops.conv_plan_keys():
        print("  %-40s %s" % (key, ", ".join(by_key.get(key, ["-"]))))
    for what, tables, excluded in (("exact-integer", ("CONV_CASES", "CENSUS_CASES"), EXACT_EXCLUSIONS),
                                   ("one-rounding", ("CONV_CASES", "GELU_CASES", "CENSUS_CASES", "FILL_CASES"), BOUND_EXCLUSIONS)):
        assert set(excluded) <= keys and not [k for k in excluded if k.startswith(SECOND_GENERATION)], (what, excluded)
        got = _reached(census, tables)
        assert not (got & set(excluded)), (what, "excluded, yet reached", sorted(got & set(excluded)))
        missing = sorted(keys - set(excluded) - got)
        assert not missing, "no %s case runs %s" % (what, ", ".join(missing))
    # every pair of the same-bits table runs two different instantiations, or says why not
    for a, b in cc.CENSUS_SAME_BITS:
        ka, kb = cc.case_by_name(a).key, cc.case_by_name(b).key
        assert ka != kb or cc.case_by_name(b).pitch == 1, (a, b, ka)


_refs = {}


def _reference(case, family, dtype):
    key = (case.name, family, dtype)
    if key not in _refs:
        o = cc.exact_case_operands(case) if family == "exact" else cc.float_case_operands(case, family, dtype)
        _refs[key] = (o,) + cc.case_reference(case, o)
    return _refs[key]


@pytest.mark.parametrize("case", cc.CENSUS_CASES, ids=[c.name for c in cc.CENSUS_CASES])
def test_census_operands_keep_both_instruments_sharp(case):
    o, want, S, act = _reference(case, "exact", None)      # (a pooled op: S is the window maximum, its largest value the conv's)
    cc.assert_exact_conditions(o, S, case.name)
    for dtype in (torch.float16, torch.bfloat16):
        for family in ("gauss", "relu") + (("subnormal",) if case.name in cc.SUBNORMAL_CASES and dtype == torch.float16 else ()):
            _, want, S, act = _reference(case, family, dtype)
            cc.assert_sharp(cc.act64(want, act), S, dtype, f"{case.name} {family} {str(dtype)[6:]}")


def test_a_new_pp_instantiation_runs_subnormal_weights():
    new = [n for n in cc.SUBNORMAL_CASES if n.startswith("cx-")]
    assert new and all(cc.case_by_name(n).file == cc.PP for n in new), new
