"""CPU: the conv planner (csrc/conv_plan.cpp).  The library's answers to its public layout / form / supported queries over the
sweep of tools/conv_plan_table.py equal, row for row, the table of the commit before the planner was gathered into one file
(tests/golden/conv_plan_parent.npz: 61,128 shapes x 10 answers); and the planner as a stand-alone program under the address /
undefined-behaviour sanitizers (tools/conv_plan_check.cpp) plans every layer of the sweep within the kernels' limits and agrees
with those answers."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_plan_parent.npz")

_spec = importlib.util.spec_from_file_location("conv_plan_table", os.path.join(ROOT, "tools", "conv_plan_table.py"))
cpt = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cpt)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in ("main", "hooks")}


def test_golden_file_is_the_sweep(golden):
    assert os.path.getsize(GOLDEN) < 100 * 1024
    rows = cpt.settings()
    assert golden["main"].shape == (2 * len(cpt.TUNINGS) * len(cpt.shapes()), len(cpt.COLUMNS)) and golden["main"].dtype == np.uint8
    assert golden["hooks"].shape == (len(cpt.HOOKS) * len(cpt.shapes(True)), len(cpt.COLUMNS))
    assert len(rows) == len(golden["main"]) + len(golden["hooks"]) and len(cpt.shapes()) == 5 * 16 * 9 * 6


def test_library_answers_equal_the_parent_table_and_hooks_are_reset(golden):
    """Every answer of every query, exactly; afterwards the hooks are unset: a default query answers as in the default rows."""
    from frmap_amd import _lib
    assert _lib.lib_available(), "libfrmap_hip.so not built (run __graft_entry__.build())"
    lib = _lib.load()
    got = cpt.table(lib)
    rows = cpt.settings()
    off = 0
    for block in ("main", "hooks"):
        want = golden[block]
        assert got[block].shape == want.shape
        bad = np.nonzero((got[block] != want).any(axis=1))[0]
        assert bad.size == 0, [(rows[off + i], "parent", want[i].tolist(), "library", got[block][i].tolist()) for i in bad[:10]]
        # every column still takes every value it takes in the file (an all-zero table would equal nothing, but say so by column)
        for c, name in enumerate(cpt.COLUMNS):
            assert set(np.unique(got[block][:, c]).tolist()) == set(np.unique(want[:, c]).tolist()), (block, name)
        off += len(want)
    # the hooks are reset: the sweep's first block is batch-invariant off, tuning (-1, -1, -1), and a fresh query repeats it
    n = len(cpt.shapes())
    for i in range(0, n, 97):
        _, inv, tune, hook, B, H, W, Ci, Co = rows[i]
        assert (inv, tune, hook) == (0, (-1, -1, -1), None)
        assert list(cpt.answers(lib, B, H, W, Ci, Co)) == golden["main"][i].tolist(), rows[i]
    # ... and one by one: forcing the second generation off and on through the hook changes an answer, unsetting restores it
    shape = (256, 14, 14, 256, 256)
    assert lib.frmap_conv3x3_pp_layout(*shape) == 1
    lib.frmap_conv_pp_tuning(0, -1, -1)
    assert lib.frmap_conv3x3_pp_layout(*shape) == 0
    lib.frmap_conv_pp_tuning(-1, -1, -1)
    assert lib.frmap_conv3x3_pp_layout(*shape) == 1


SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _gpu_present():
    import torch
    return torch.cuda.is_available()


def _records(golden, cus=256):
    """The sweep as tools/conv_plan_check.cpp reads it: cus inv enable px bn pitch ds B H W Cin Cout a0 .. a9."""
    lines = []
    tables = np.concatenate([golden["main"], golden["hooks"]])
    for (block, inv, tune, hook, B, H, W, Ci, Co), a in zip(cpt.settings(), tables.tolist()):
        pitch = hook[1] if hook and hook[0] == "frmap_conv_pp_pitch" else -1
        ds = hook[1] if hook and hook[0] == "frmap_conv_pp_ds" else -1
        lines.append(" ".join(map(str, (cus, inv, *tune, pitch, ds, B, H, W, Ci, Co, *a))))
    return "\n".join(lines) + "\n"


def _build_checker(tmp_path):
    """tools/conv_plan_check.cpp built with the sanitizers: (path of the program, the environment to run it in)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link an empty program with -fsanitize=address,undefined: no sanitizer runtimes installed")
    exe = str(tmp_path / "conv_plan_check")
    csrc = os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN_FLAGS, "-I" + csrc, os.path.join(ROOT, "tools", "conv_plan_check.cpp"),
           "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("FRMAP_")}   # the table was made with the default environment
    return exe, env


@pytest.mark.skipif(_gpu_present(), reason="a sanitizer build is host-only work: nothing of it runs on a machine with a GPU")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to build the stand-alone sanitizer program with")
def test_planner_is_sanitizer_clean_and_plans_within_the_kernels_limits(tmp_path, golden):
    """tools/conv_plan_check.cpp (its own `main` over csrc/conv_plan.cpp, nothing else) built with -fsanitize=address,undefined
    (runtimes linked statically) and run directly on the whole sweep: no sanitizer report, every plan within the LDS, halo and grid
    limits, a shortcut / pooled plan exactly where the library says so, the candidates' answers the library's (a second compiler:
    the library is built by hipcc).  Decided before any work: not on a machine with a GPU, and only where g++ can link an empty
    program with the sanitizers."""
    exe, env = _build_checker(tmp_path)
    own = subprocess.run([exe], input="", capture_output=True, text=True, env=env)
    assert own.returncode == 0 and "0 failed checks" in own.stdout, own.stdout + own.stderr
    run = subprocess.run([exe], input=_records(golden), capture_output=True, text=True, env=env)
    fails = [ln for ln in run.stdout.splitlines() if ln.startswith("FAIL")]
    assert run.returncode == 0 and not fails and run.stderr == "", "\n".join(fails[:20]) + run.stderr[-2000:]
    last = run.stdout.splitlines()[-1]
    n = len(golden["main"]) + len(golden["hooks"])
    assert last.startswith("conv_plan_check: %d records," % n) and last.endswith(" 0 failed checks"), last
    plans = [ln for ln in run.stdout.splitlines() if ln.startswith("plan ")]
    kernels = {ln.split(": ", 1)[1].split(" ", 1)[0] for ln in plans}
    assert kernels == {"conv_igemm_kernel", "conv1x1_kernel", "conv3x3_c64_wave_kernel", "conv3x3_fast_kernel", "conv3x3s2_split_kernel",
                       "conv3x3s2_fast_kernel", "conv3x3_pp_kernel", "conv3x3s2_pp_kernel", "conv1x1_pp_kernel"}, kernels


def _big_records():
    """The layers of the large-tensor tests (tests/big_cases.py) at their batch, as `conv_plan_check big` reads them, with the kernel
    each must get; then layers at the limits themselves: maps of one and two pixels, whose M is exactly 2^31 - 1 and 2^31 in the
    program's sweep, and images past the per-image limits of the wave and register-prefetch kernels."""
    import big_cases as bc
    recs = []
    for case, _, kernel in bc.BIG_CONV:
        if kernel is None:
            continue
        tune = case.tune if case.tune is not None else (-1, -1, -1)
        fuse, ds = (1 if case.res else 0), (0, 0, 0, 0)
        if case.op == "ds":
            fuse, ds = 2, (2 * case.H, 2 * case.W, case.ds[0], case.ds[1])
        elif case.op == "pool2":
            fuse = 3
        recs.append(((*tune, bc.conv_batch(case), case.H, case.W, case.Cin, case.Cout, case.k, case.stride, case.k // 2, fuse, *ds), kernel))
    off = (0, -1, -1)
    recs += [
        ((*off, 7, 1, 1, 128, 128, 1, 1, 0, 0, 0, 0, 0, 0), "conv1x1_kernel"),            # M = B: 2^31 - 1 in the sweep
        ((*off, 7, 1, 2, 128, 128, 1, 1, 0, 1, 0, 0, 0, 0), "conv1x1_kernel"),            # M = 2 B: 2^31 at B = 2^30
        ((-1, -1, -1, 7, 1, 1, 2048, 512, 1, 1, 0, 0, 0, 0, 0, 0), None),
        # one image of 2^31 bytes: not the wave kernel.  (Cin = 64 and H < 32768 need W >= 512 for that, where the generic fit the
        # cascade demands in front of the wave kernel already fails: the wave kernel's own per-image check cannot decide a layer)
        ((*off, 1, 32760, 512, 64, 64, 3, 1, 1, 0, 0, 0, 0, 0), "none"),
        ((*off, 1, 32760, 16, 1024, 64, 3, 1, 1, 1, 0, 0, 0, 0), "conv_igemm_kernel"),    # three of them past 2^31: no register prefetch
        ((*off, 1, 32760, 16, 1024, 64, 3, 2, 1, 0, 0, 0, 0, 0), "conv3x3s2_split_kernel"),
    ]
    return recs


@pytest.mark.skipif(_gpu_present(), reason="a sanitizer build is host-only work: nothing of it runs on a machine with a GPU")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to build the stand-alone sanitizer program with")
def test_planner_at_large_batches_computes_in_range_and_refuses_past_the_limit(tmp_path):
    """`conv_plan_check big`: every layer of the large-tensor tests gets the kernel its case names at its batch; over the sweep (input
    past 2^31, 2^32, 2^33 bytes; M just under, at and past 2^31) no int of a plan overflows (UBSan) or differs from its 64-bit
    value, and from M = 2^31 on there is no plan."""
    exe, env = _build_checker(tmp_path)
    recs = _big_records()
    text = "\n".join(" ".join(map(str, r)) for r, _ in recs) + "\n"
    run = subprocess.run([exe, "big"], input=text, capture_output=True, text=True, env=env)
    fails = [ln for ln in run.stdout.splitlines() if ln.startswith("FAIL")]
    assert run.returncode == 0 and not fails and run.stderr == "", "\n".join(fails[:20]) + run.stderr[-2000:]
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("big ")]
    assert len(lines) == len(recs)
    for ln, (r, kernel) in zip(lines, recs):
        assert kernel is None or ln[2] == kernel, (r, "planned", ln[2], "the case names", kernel)
    last = run.stdout.splitlines()[-1]
    assert last.startswith("conv_plan_check: %d large-batch records," % len(recs)) and last.endswith(" 0 failed checks"), last
