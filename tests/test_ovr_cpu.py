"""CPU: the one-vs-rest rank counts - the rule in numpy (`evaluate.ovr_rank_rule`) on six hand-built rows with every integer
written out, `evaluate.ovr_metrics` against sklearn (`roc_curve` + `auc` and the binary `average_precision_score` per class,
`roc_auc_score(multi_class='ovr')` and the multiclass `average_precision_score`) at 1e-12, the project's bar for sklearn parity,
NaN where a class has no positive or no negative, the kernel's host twin (`ops.ovr_rank_counts_host`: the header the kernel
compiles) against the numpy rule word for word over the sweep of tools/ovr_rank_check.cpp, split / order / merge invariance, that
program under the address and undefined-behaviour sanitizers, and the C ABI of the new entry points with their alignment rows."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ovr_cases as oc
from frmap_amd import _lib, evaluate, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------------
def test_hand_built_rows_every_integer_written_out():
    a, b, e, why = evaluate.ovr_rank_rule(oc.HAND_SCORES, oc.HAND_LABELS)
    assert a.dtype == b.dtype == e.dtype == np.uint64
    assert a.tolist() == oc.HAND["ge_same"] and b.tolist() == oc.HAND["ge_other"] and e.tolist() == oc.HAND["eq_other"]
    assert why.tolist() == oc.HAND["why"]
    stored = evaluate.ovr_stored_labels(oc.HAND_SCORES, oc.HAND_LABELS)
    assert stored.dtype == np.int32 and stored.tolist() == oc.HAND["stored"]
    # the twin on the same rows
    store, lab = oc.store_of(oc.HAND_SCORES, oc.HAND_LABELS)
    assert store.shape == (3, 6) and np.array_equal(lab, stored)
    ta, tb, te = ops.ovr_rank_counts_host(store, lab)
    assert ta.tolist() == oc.HAND["ge_same"] and tb.tolist() == oc.HAND["ge_other"] and te.tolist() == oc.HAND["eq_other"]
    # the metrics of these integers
    m = evaluate.ovr_metrics(stored, a, b, e, 3, ["a", "b", "c"])
    assert (m["rows"], m["ignored"], m["nonfinite"]) == (4, 1, 1)
    for k, name in enumerate("abc"):
        got = m["per_class"][name]
        assert got["support"] == oc.HAND["support"][k]
        for field in ("roc_auc", "average_precision"):
            want = oc.HAND[field][k]
            assert (np.isnan(got[field]) and np.isnan(want)) or abs(got[field] - want) <= 1e-15, (name, field, got[field], want)
    assert np.isnan(m["roc_auc"]) and np.isnan(m["pr_auc"])                  # class c has no sample
    # a label of -2 handed in as a raw label is out of range: ignored by the rule, whatever the store's own code means
    assert evaluate.ovr_rank_rule(oc.HAND_SCORES, stored)[3].tolist() == [0, 0, 0, 0, 1, 1]


# ---------------------------------------------------------------------------------------------------------------------------------
# metrics against sklearn
# ---------------------------------------------------------------------------------------------------------------------------------
SKLEARN_CASES = [("softmax", 64, 3), ("softmax", 265, 36), ("softmax", 1000, 10), ("eighths", 64, 3), ("eighths", 265, 36), ("eighths", 1000, 10)]


@pytest.mark.parametrize("kind,N,C", SKLEARN_CASES)
def test_metrics_against_sklearn(kind, N, C):
    from sklearn.metrics import average_precision_score, roc_auc_score
    z, y = (oc.softmax_rows if kind == "softmax" else oc.multinomial_rows)(31, N, C)
    assert len(np.unique(y)) == C
    a, b, e, why = evaluate.ovr_rank_rule(z, y)
    assert not why.any() and int(a.min()) >= 1
    if kind == "eighths":                                                    # most rows tie with a row of another class
        assert int((e > 0).sum()) > N // 2
    m = evaluate.ovr_metrics(y, a, b, e, C)
    roc, ap = oc.sklearn_per_class(z, y, C)
    got_roc = np.array([m["per_class"][str(c)]["roc_auc"] for c in range(C)])
    got_ap = np.array([m["per_class"][str(c)]["average_precision"] for c in range(C)])
    worst = max(float(np.abs(got_roc - roc).max()), float(np.abs(got_ap - ap).max()))
    print("\novr_metrics %s N=%d C=%d: worst per-class difference from sklearn %.3g" % (kind, N, C, worst))
    assert worst <= 1e-12
    assert [m["per_class"][str(c)]["support"] for c in range(C)] == np.bincount(y, minlength=C).tolist()
    # the two calls of the reference's metric block, on the same values (fp32 softmax rows sum to 1 within the call's own tolerance)
    want_roc = roc_auc_score(y, z.astype(np.float64), multi_class="ovr")
    want_ap = average_precision_score(y, z.astype(np.float64))
    print("ovr_metrics %s N=%d C=%d: roc_auc %.17g (sklearn %.17g), pr_auc %.17g (sklearn %.17g)" % (kind, N, C, m["roc_auc"], want_roc,
                                                                                                   m["pr_auc"], want_ap))
    assert abs(m["roc_auc"] - want_roc) <= 1e-12 and abs(m["pr_auc"] - want_ap) <= 1e-12
    assert (m["rows"], m["ignored"], m["nonfinite"]) == (N, 0, 0)


def test_binary_case_against_sklearn():
    from sklearn.metrics import average_precision_score, roc_auc_score
    z, y = oc.softmax_rows(5, 64, 2)
    a, b, e, _ = evaluate.ovr_rank_rule(z, y)
    m = evaluate.ovr_metrics(y, a, b, e, 2)
    for c in (0, 1):
        assert abs(m["per_class"][str(c)]["roc_auc"] - roc_auc_score(y == c, z[:, c])) <= 1e-12
        assert abs(m["per_class"][str(c)]["average_precision"] - average_precision_score(y == c, z[:, c])) <= 1e-12


def test_nan_where_a_class_has_no_positive_or_no_negative():
    z, y = oc.softmax_rows(7, 40, 4)
    y = np.where(y == 2, 1, y)                                               # class 2 has no positive
    a, b, e, _ = evaluate.ovr_rank_rule(z, y)
    m = evaluate.ovr_metrics(y, a, b, e, 4)
    assert np.isnan(m["per_class"]["2"]["roc_auc"]) and np.isnan(m["per_class"]["2"]["average_precision"]) and m["per_class"]["2"]["support"] == 0
    assert all(np.isfinite(m["per_class"][k]["roc_auc"]) and np.isfinite(m["per_class"][k]["average_precision"]) for k in "013")
    assert np.isnan(m["roc_auc"]) and np.isnan(m["pr_auc"])
    # one class only: no negative, so no ROC; the precision is 1 at every positive
    y1 = np.zeros(40, np.int32)
    a, b, e, _ = evaluate.ovr_rank_rule(z, y1)
    assert not b.any() and not e.any() and int(a.max()) <= 40
    m = evaluate.ovr_metrics(y1, a, b, e, 4)
    assert np.isnan(m["per_class"]["0"]["roc_auc"]) and m["per_class"]["0"]["average_precision"] == 1.0 and np.isnan(m["roc_auc"])
    # nothing counted at all
    m = evaluate.ovr_metrics(np.array([-1, -2], np.int32), [0, 0], [0, 0], [0, 0], 3)
    assert (m["rows"], m["ignored"], m["nonfinite"]) == (0, 1, 1) and np.isnan(m["roc_auc"]) and np.isnan(m["pr_auc"])
    empty = evaluate.OvrScores(3, 4, device="cpu").metrics()
    assert empty["rows"] == 0 and np.isnan(empty["pr_auc"]) and sorted(empty["per_class"]) == ["0", "1", "2"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the twin against the rule
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", oc.SWEEP_C)
def test_twin_equals_the_rule_word_for_word(C):
    for N in oc.SWEEP_N:
        for kind in oc.KINDS:
            z, y = oc.rows(17, N, C, kind)
            want = evaluate.ovr_rank_rule(z, y)
            store, lab = oc.store_of(z, y, N + 3)                            # three rows of capacity past n: never read
            got = ops.ovr_rank_counts_host(store, lab, N)
            for k, name in enumerate(("ge_same", "ge_other", "eq_other")):
                assert got[k].dtype == np.uint64 and got[k].shape == (N,)
                assert np.array_equal(got[k], want[k]), (C, N, kind, name, np.nonzero(got[k] != want[k])[0][:8])
            declined = want[3] != 0
            assert not got[0][declined].any() and not got[1][declined].any() and not got[2][declined].any()
            assert np.array_equal(lab[:N] < 0, declined) and ((lab[:N] == -1) == (want[3] == 1)).all()
            if N >= 64:
                assert (want[3] == 0).any() and (want[3] == 1).any() and (want[3] == 2).any()
            if kind == "equal" and N:
                ok = ~declined
                support = np.bincount(y[ok], minlength=C)
                assert np.array_equal(got[0][ok], support[y[ok]].astype(np.uint64))
                assert np.array_equal(got[1][ok], (ok.sum() - support[y[ok]]).astype(np.uint64)) and np.array_equal(got[2][ok], got[1][ok])


def test_special_values_twin_and_rule():
    for C in (1, 3, 65):
        z, y = oc.special_rows(3, 257, C)
        want = evaluate.ovr_rank_rule(z, y)
        got = ops.ovr_rank_counts_host(*oc.store_of(z, y))
        assert all(np.array_equal(g, w) for g, w in zip(got, want[:3])) and not want[3].any()
        # what a bit-pattern compare or a flush to zero would give differs: the case is sharp
        if C > 1:
            flushed = np.where(np.abs(z) < np.finfo(F32).tiny, F32(0), z)
            assert any(not np.array_equal(f, w) for f, w in zip(evaluate.ovr_rank_rule(flushed, y)[:3], want[:3]))


def test_split_order_and_merge_invariance():
    C = 36
    z, y = oc.rows(23, oc.B_FULL, C, "quantised")
    want = evaluate.ovr_rank_rule(z, y)
    # order: a permutation of the rows gives the permuted integers, for the rule and for the twin
    perm = np.random.default_rng(9).permutation(oc.B_FULL)
    back = evaluate.ovr_rank_rule(z[perm], y[perm])
    twin = ops.ovr_rank_counts_host(*oc.store_of(z[perm], y[perm]))
    for k in range(3):
        assert np.array_equal(back[k], want[k][perm]) and np.array_equal(twin[k], want[k][perm])
    # split and merge: stores filled in pieces (the numpy statement of three appends) hold the same bits as one filled at once
    whole_store, whole_lab = oc.store_of(z, y)
    parts = [oc.store_of(z[lo:hi], y[lo:hi]) for lo, hi in zip((0,) + oc.SPLIT, oc.SPLIT + (oc.B_FULL,))]
    assert np.array_equal(np.concatenate([p[0] for p in parts], axis=1).view(np.uint32), whole_store.view(np.uint32))
    assert np.array_equal(np.concatenate([p[1] for p in parts]), whole_lab)
    a, b = evaluate.OvrScores(C, 8, device="cpu"), evaluate.OvrScores(C, 300, device="cpu")
    for acc, (lo, hi) in ((a, (0, 100)), (b, (100, oc.B_FULL))):             # (filled by hand: `update` is the GPU's business)
        acc._reserve(hi - lo)
        s, l = oc.store_of(z[lo:hi], y[lo:hi])
        acc.store[:, :hi - lo] = torch.from_numpy(s)
        acc.labels[:hi - lo] = torch.from_numpy(l)
        acc.rows = hi - lo
    assert a.capacity == 100 and b.capacity == 300
    a.merge(b)
    assert a.rows == oc.B_FULL and a.capacity == 259
    got = ops.ovr_rank_counts_host(a.store.numpy(), a.labels.numpy(), a.rows)
    assert all(np.array_equal(g, w) for g, w in zip(got, want[:3]))
    assert np.array_equal(a.store[:, :a.rows].numpy().view(np.uint32), whole_store.view(np.uint32))
    assert a.reset().rows == 0
    with pytest.raises(ValueError, match="classes"):
        a.merge(evaluate.OvrScores(C + 1, 8, device="cpu"))
    with pytest.raises(ValueError):
        evaluate.OvrScores(0, 8, device="cpu")
    assert evaluate.OvrScores(3, 4, device="cpu").update(torch.zeros((0, 3)), torch.zeros((0,), dtype=torch.int64)).rows == 0   # no-op, no GPU


def test_twin_and_launchers_refuse_bad_arguments():
    store, lab = oc.store_of(oc.HAND_SCORES, oc.HAND_LABELS)
    with pytest.raises(ValueError, match="n exceeds capacity"):
        ops.ovr_rank_counts_host(store, lab, 7)
    with pytest.raises(ValueError, match="n is negative"):
        ops.ovr_rank_counts_host(store, lab, -1)
    with pytest.raises(ValueError):
        ops.ovr_rank_counts_host(store, lab[:5])
    assert all(len(v) == 0 for v in ops.ovr_rank_counts_host(store, lab, 0))
    # the launchers' refusals come before any HIP call: host dummy pointers serve (and nothing is written)
    lib = _lib.load()
    buf = np.zeros(4096, np.uint8)
    p = (buf.ctypes.data + 255) // 256 * 256
    big = 2 ** 26 - 3
    for args, word in (((p, p, 0, 4, p, p, 8, 0), "B = 0"), ((p, p, big, 4, p, p, 2 ** 40, 0), "B = "), ((p, p, 1, 0, p, p, 8, 0), "C = 0"),
                       ((p, p, 1, 4, p, p, 8, -1), "first = -1"), ((p, p, 3, 4, p, p, 8, 6), "capacity"),
                       ((p, p, 1, 4, p, p, 2 ** 62, 2 ** 62), "capacity"), ((p + 2, p, 1, 4, p, p, 8, 0), "scores must be 4-byte aligned"),
                       ((p, p, 1, 4, p, p + 1, 8, 0), "store_labels must be 4-byte aligned"), ((p, p, 1, 4, 0, p, 8, 0), "null pointer")):
        assert lib.frmap_ovr_append(*args, None) == -1, word
        msg = lib.frmap_last_error().decode()
        assert msg.startswith("ovr_append: ") and word in msg, (word, msg)
    for args, word in (((p, p, 0, 8, 4, p, p, p), "n = 0"), ((p, p, 2 ** 31, 2 ** 32, 4, p, p, p), "n = "), ((p, p, 9, 8, 4, p, p, p), "capacity"),
                       ((p, p, 1, 8, 0, p, p, p), "C = 0"), ((p, p, 1, 8, 2 ** 24, p, p, p), "C = "),
                       ((p, p, 1, 8, 4, p + 4, p, p), "ge_same_out must be 8-byte aligned"),
                       ((p, p, 1, 8, 4, p, p, p + 4), "eq_other_out must be 8-byte aligned"), ((p, p + 2, 1, 8, 4, p, p, p), "store_labels must be 4-byte aligned"),
                       ((p, p, 1, 8, 4, p, 0, p), "null pointer")):
        assert lib.frmap_ovr_rank_counts(*args, None) == -1, word
        msg = lib.frmap_last_error().decode()
        assert msg.startswith("ovr_rank_counts: ") and word in msg, (word, msg)
    assert not buf.any()


# ---------------------------------------------------------------------------------------------------------------------------------
# the check program under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="a sanitizer build is host-only work: nothing of it runs on a machine with a GPU")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to build the stand-alone sanitizer program with")
def test_twin_is_sanitizer_clean_as_a_stand_alone_program(tmp_path):
    """tools/ovr_rank_check.cpp (its own `main`, ovr_twin.h and ovr_rule.h) built with -fsanitize=address,undefined (runtimes linked
    statically) and run directly: it sweeps the grid of `ovr_cases` on stores of exactly the size the call is given, with declined
    rows and unread rows past n, and exits 0."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link an empty program with -fsanitize=address,undefined: no sanitizer runtimes installed")
    exe = str(tmp_path / "ovr_rank_check")
    csrc = os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc")
    built = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN_FLAGS, "-I" + csrc,
                            os.path.join(ROOT, "tools", "ovr_rank_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdin=subprocess.DEVNULL, capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
    n = len(oc.SWEEP_N) * len(oc.SWEEP_C) * len(oc.KINDS)
    assert run.stdout.splitlines()[-2:] == ["%d cases" % n, "self check passed"], run.stdout[-500:]
    src = open(os.path.join(ROOT, "tools", "ovr_rank_check.cpp")).read()
    for name, grid in (("Ns", oc.SWEEP_N), ("Cs", oc.SWEEP_C)):              # the program's grid is this module's
        assert "%s[] = {%s}" % (name, ", ".join(str(v) for v in grid)) in src, name


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ovr_entry_points_are_declared_bound_and_element_aligned():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_ovr_append", 9), ("frmap_ovr_rank_counts", 9), ("frmap_ovr_rank_counts_host", 8)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % sym, header)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
        assert hasattr(_lib.load(), sym)
    assert _lib.load().frmap_abi_version() == _lib.ABI_VERSION
    rows = _lib.ALIGNMENT["frmap_ovr_append"]
    assert list(rows) == ["scores", "labels", "store", "store_labels"] and all(v == ("element", 4) for v in rows.values())
    rows = _lib.ALIGNMENT["frmap_ovr_rank_counts"]
    assert list(rows) == ["store", "store_labels", "ge_same_out", "ge_other_out", "eq_other_out"]
    assert {a: v for a, v in rows.items()} == {"store": ("element", 4), "store_labels": ("element", 4), "ge_same_out": ("element", 8),
                                               "ge_other_out": ("element", 8), "eq_other_out": ("element", 8)}
    assert "frmap_ovr_rank_counts_host" not in _lib.ALIGNMENT
    build = open(os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc", "build.sh")).read()
    assert " ovr_rank.hip " in build
    for h in ("ovr_rule.h", "ovr_twin.h"):
        assert os.path.isfile(os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc", h))
    for name in ("ovr_append", "ovr_rank_counts", "ovr_rank_counts_host"):
        assert callable(getattr(ops, name))
    for name in ("OvrScores", "ovr_rank_rule", "ovr_stored_labels", "ovr_metrics", "evaluate_stream"):
        assert callable(getattr(evaluate, name))
    import inspect
    assert inspect.signature(evaluate.evaluate_stream).parameters["auc"].default is False
    with pytest.raises(RuntimeError):
        ops.ovr_append(torch.zeros((2, 3)), torch.zeros((2,), dtype=torch.int32), torch.zeros((3, 4)), torch.zeros((4,), dtype=torch.int32), 0)
