"""CPU: the classification tally - the rule in numpy (`evaluate.tally_rule`) on a hand-built case with every integer written out,
the bin-edge formula against `np.linspace`, the kernel's host twin (`ops.classify_tally_host`: the header the kernel compiles)
against the numpy rule word for word over the sweep of tools/classify_tally_check.cpp, split / order / merge invariance, that
program under the address and undefined-behaviour sanitizers, `evaluate.metrics_from_tally` against sklearn and against the
reference's own functions (tests/golden/advanced_metrics.json, written by tools/gen_tally_golden.py), and the C ABI of the new
entry points with their alignment rows."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import tally_cases as tc
from frmap_amd import _lib, evaluate, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------------
def test_hand_built_rows_every_integer_written_out():
    nan = np.nan
    z = np.array([[0.0, 3.0, 1.0, 2.0],        # correct: label 1 is the maximum
                  [0.0, 3.0, 1.0, 2.0],        # wrong: label 2, two classes above it
                  [5.0, 1.0, 5.0, 0.0],        # a tie won by the lower index: pred 0, label 0, rank 0
                  [5.0, 1.0, 5.0, 0.0],        # the target (2) tied with an earlier class: pred 0, rank 1
                  [9.0, 9.0, 9.0, 9.0],        # label -1: ignored whatever the logits are
                  [0.0, nan, 1.0, 2.0]], F32)  # a NaN: nonfinite
    y = np.array([1, 2, 0, 2, -1, 3], np.int32)
    conf = np.array([0.625, 0.625, 0.25, 1.0, nan, nan], F32)          # bins of 4 edges (0, 1/3, 2/3, 1): 1, 1, 0, 3
    loss = np.array([0.5, 2.25, 1.0, 70000.0, nan, nan], F32)          # 70000 is clamped to 65536
    pred, rank, why = evaluate.tally_row_rule(z, y)
    assert pred.tolist() == [1, 1, 0, 0, -1, -1] and rank.tolist() == [0, 2, 0, 1, -1, -1] and why.tolist() == [0, 0, 0, 0, 1, 2]
    state, p2, r2 = evaluate.tally_rule(z, y, conf, loss, ranks=2, n_bins=4, confusion=True)
    assert p2.tolist() == pred.tolist() and r2.tolist() == rank.tolist()
    want = [4, 1, 1, 2, (2 ** 23) + 9 * 2 ** 22 + 2 ** 24 + 65536 * 2 ** 24, 0, 0, 0,     # rows ignored nonfinite correct loss_q
            2, 2,                                                       # rank_hist [rank 0, rank >= 1]
            1, 1, 2, 0,                                                 # support
            2, 2, 0, 0,                                                 # predicted
            1, 1, 0, 0,                                                 # hit
            1, 2, 0, 1,                                                 # bin_count
            1, 1, 0, 0,                                                 # bin_correct
            2 ** 30, 2 * 5 * 2 ** 29, 0, 2 ** 32,                       # bin_conf_q
            1, 0, 0, 0,                                                 # confusion, label 0
            0, 1, 0, 0,                                                 # label 1
            1, 1, 0, 0,                                                 # label 2
            0, 0, 0, 0]                                                 # label 3
    assert state.tolist() == want
    lay = evaluate.tally_layout(4, 2, 4, True)
    assert lay["words"] == len(want) and lay["confusion"] == slice(34, 50) and lay["rank_hist"] == slice(8, 10)
    # the twin on the same rows
    s2, p3, r3 = ops.classify_tally_host(z, y, np.nan_to_num(conf), np.nan_to_num(loss), None, 2, 4, True)
    assert s2.tolist() == want and p3.tolist() == pred.tolist() and r3.tolist() == rank.tolist()
    # the float64 row values of the counted rows
    _, _, c64, l64 = evaluate.tally_rows_reference(z, y)
    s = np.exp(-3.0) + 1 + np.exp(-2.0) + np.exp(-1.0)
    assert abs(c64[0] - 1 / s) < 1e-15 and abs(l64[0] - np.log(s)) < 1e-15 and abs(l64[1] - (np.log(s) + 2.0)) < 1e-15
    assert np.isnan(c64[4:]).all() and np.isnan(l64[4:]).all()


def test_edge_formula_is_linspace_bit_for_bit():
    for n in range(1, 1025):
        e = evaluate.tally_edges(n)
        assert e.dtype == np.float64 and np.array_equal(e, np.linspace(0, 1, n)), n
    # and the bin is np.digitize - 1 with the quirk: n_bins edges, so only 1.0 reaches the last bin
    c = np.array([0.0, 0.1, 1 / 9, 0.5, 0.99999994, 1.0])
    assert (np.digitize(c, evaluate.tally_edges(10)) - 1).tolist() == [0, 0, 1, 4, 8, 9]


# ---------------------------------------------------------------------------------------------------------------------------------
# the twin against the rule
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", tc.SWEEP_C)
def test_twin_equals_the_rule_word_for_word(C):
    for R in tc.SWEEP_R:
        for nb in tc.SWEEP_BINS:
            for keep in (False, True):
                z, y, conf, loss = tc.host_rows(17, tc.B_FULL, C, nb)
                want, pred, rank = evaluate.tally_rule(z, y, conf, loss, R, nb, keep)
                got, p2, r2 = ops.classify_tally_host(z, y, conf, loss, None, R, nb, keep)
                assert got.shape == (ops.classify_tally_words(C, R, nb, keep),) == (evaluate.tally_layout(C, R, nb, keep)["words"],)
                assert np.array_equal(got, want), (C, R, nb, keep, np.nonzero(got != want)[0][:8])
                assert np.array_equal(p2, pred) and np.array_equal(r2, rank)
                assert want[0] > 0 and want[1] > 0 and want[2] > 0 and want[0] + want[1] + want[2] == tc.B_FULL
                lay = ops.classify_tally_layout(C, R, nb, keep)
                assert {k: v for k, v in evaluate.tally_layout(C, R, nb, keep).items() if k != "words"} == lay
                if (R, nb) != (6, 10):
                    continue
                # three launches (1 + 100 + 158 rows) = one launch of 259 = the rows reversed
                st = None
                for lo, hi in zip((0,) + tc.SPLIT, tc.SPLIT + (tc.B_FULL,)):
                    st, _, _ = ops.classify_tally_host(z[lo:hi], y[lo:hi], conf[lo:hi], loss[lo:hi], st, R, nb, keep)
                assert np.array_equal(st, want)
                back, _, _ = ops.classify_tally_host(z[::-1], y[::-1], conf[::-1], loss[::-1], None, R, nb, keep)
                assert np.array_equal(back, want)


def test_merge_of_two_states_is_the_tally_of_the_concatenation():
    C = 65
    z, y, conf, loss = tc.host_rows(23, tc.B_FULL, C, 10)
    whole, _, _ = ops.classify_tally_host(z, y, conf, loss)
    a, b = evaluate.ClassificationTally(C, device="cpu"), evaluate.ClassificationTally(C, device="cpu")
    assert a.confusion and a.state.dtype == torch.int64 and a.state.numel() == whole.size
    for tally, sl in ((a, slice(0, 100)), (b, slice(100, None))):
        st, _, _ = ops.classify_tally_host(z[sl], y[sl], conf[sl], loss[sl])
        tally.state.copy_(torch.from_numpy(st.view(np.int64)))
    a.merge(b)
    assert np.array_equal(a.state.numpy().view(np.uint64), whole)
    counts = a.counts()
    assert counts["rows"] == int(whole[0]) and counts["confusion"].shape == (C, C) and int(counts["confusion"].sum()) == counts["rows"]
    with pytest.raises(ValueError, match="layouts differ"):
        a.merge(evaluate.ClassificationTally(C, ranks=7, device="cpu"))
    assert int(a.reset().state.abs().sum()) == 0
    assert not evaluate.ClassificationTally(2049, device="cpu").confusion and evaluate.ClassificationTally(2048, device="cpu").confusion
    with pytest.raises(ValueError):
        evaluate.ClassificationTally(4097, confusion=True, device="cpu")
    assert evaluate.ClassificationTally(3, device="cpu").update(torch.zeros((0, 3)), torch.zeros((0,), dtype=torch.int64)) is not None   # no-op, no GPU


def test_twin_refuses_bad_arguments_and_leaves_the_state():
    z, y = np.zeros((2, 4), F32), np.array([0, 1], np.int32)
    ok = np.array([0.5, 0.5], F32)
    st = np.zeros(ops.classify_tally_words(4), np.uint64)
    for conf, loss, word in ((np.array([0.5, 1.5], F32), ok, "row_conf"), (ok, np.array([0.5, np.nan], F32), "row_loss"),
                             (ok, np.array([-1.0, 0.5], F32), "row_loss")):
        with pytest.raises(ValueError, match=word):
            ops.classify_tally_host(z, y, conf, loss, st)
        assert not st.any()
    lib = _lib.load()
    assert lib.frmap_classify_tally_words(0, 6, 10, 1) == 0 and lib.frmap_classify_tally_words(4, 0, 10, 1) == 0
    assert lib.frmap_classify_tally_words(4, 1025, 10, 1) == 0 and lib.frmap_classify_tally_words(4, 6, 0, 0) == 0
    assert lib.frmap_classify_tally_words(4, 6, 1025, 0) == 0 and lib.frmap_classify_tally_words(4097, 6, 10, 1) == 0
    assert lib.frmap_classify_tally_words(4097, 6, 10, 0) == 8 + 6 + 3 * 4097 + 30
    assert lib.frmap_classify_tally_words(4096, 1024, 1024, 1) == 8 + 1024 + 3 * 4096 + 3 * 1024 + 4096 * 4096
    # the launcher's refusals come before any HIP call: host dummy pointers serve (and nothing is written)
    buf = np.zeros(4096, np.uint8)
    p = (buf.ctypes.data + 255) // 256 * 256
    for args, word in (((p, p, 0, 4, 6, 10, 1, p, 0, 0, 0, 0), "B = 0"), ((p, p, 2 ** 26 - 3, 4, 6, 10, 1, p, 0, 0, 0, 0), "B = "),
                       ((p, p, 1, 0, 6, 10, 1, p, 0, 0, 0, 0), "C = 0"), ((p, p, 1, 4, 0, 10, 1, p, 0, 0, 0, 0), "R = 0"),
                       ((p, p, 1, 4, 1025, 10, 1, p, 0, 0, 0, 0), "R = 1025"), ((p, p, 1, 4, 6, 0, 1, p, 0, 0, 0, 0), "n_bins = 0"),
                       ((p, p, 1, 4, 6, 1025, 1, p, 0, 0, 0, 0), "n_bins = 1025"), ((p, p, 1, 4097, 6, 10, 1, p, 0, 0, 0, 0), "keep_confusion"),
                       ((p + 2, p, 1, 4, 6, 10, 1, p, 0, 0, 0, 0), "logits must be 4-byte aligned"),
                       ((p, p, 1, 4, 6, 10, 1, p + 4, 0, 0, 0, 0), "state must be 8-byte aligned"),
                       ((p, p, 1, 4, 6, 10, 1, p, 0, 0, p + 1, 0), "row_conf_out must be 4-byte aligned"),
                       ((p, 0, 1, 4, 6, 10, 1, p, 0, 0, 0, 0), "null pointer")):
        assert lib.frmap_classify_tally(*args, None) == -1, word
        msg = lib.frmap_last_error().decode()
        assert msg.startswith("classify_tally: ") and word in msg, (word, msg)
    assert not buf.any()


# ---------------------------------------------------------------------------------------------------------------------------------
# the check program under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="a sanitizer build is host-only work: nothing of it runs on a machine with a GPU")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to build the stand-alone sanitizer program with")
def test_twin_is_sanitizer_clean_as_a_stand_alone_program(tmp_path):
    """tools/classify_tally_check.cpp (its own `main`, tally_twin.h and tally_rule.h, nothing else) built with
    -fsanitize=address,undefined (runtimes linked statically) and run directly: it sweeps the grid of `tally_cases` on rows with
    labels out of range and non-finite logits, asserts every index it forms inside the state, and exits 0."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link an empty program with -fsanitize=address,undefined: no sanitizer runtimes installed")
    exe = str(tmp_path / "classify_tally_check")
    csrc = os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc")
    built = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN_FLAGS, "-I" + csrc,
                            os.path.join(ROOT, "tools", "classify_tally_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdin=subprocess.DEVNULL, capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
    n = len(tc.SWEEP_C) * len(tc.SWEEP_R) * len(tc.SWEEP_BINS) * 2
    assert run.stdout.splitlines()[-2:] == ["%d cases" % n, "self check passed"], run.stdout[-500:]
    src = open(os.path.join(ROOT, "tools", "classify_tally_check.cpp")).read()
    for name, grid in (("Cs", tc.SWEEP_C), ("Rs", tc.SWEEP_R), ("NBs", tc.SWEEP_BINS)):      # the program's grid is this module's
        assert "%s[] = {%s}" % (name, ", ".join(str(v) for v in grid)) in src, name


# ---------------------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------------------
def _counts_of(y_true, y_pred, C, conf=None, n_bins=10):
    """The integers a tally of these labels / predictions holds, through the rule: one-hot logits reproduce the predictions."""
    n = len(y_true)
    z = np.zeros((n, C), F32)
    z[np.arange(n), y_pred] = 1.0
    conf = np.full(n, 0.5, F32) if conf is None else np.asarray(conf, F32)
    state, pred, _ = evaluate.tally_rule(z, y_true, conf, np.zeros(n, F32), 6, n_bins, True)
    assert np.array_equal(pred, y_pred)
    return evaluate.tally_counts(state, C, 6, n_bins, True)


def test_metrics_against_sklearn():
    from sklearn.metrics import accuracy_score, confusion_matrix, f1_score, precision_score, recall_score
    rng = np.random.default_rng(5)
    C, n = 9, 400
    y = rng.integers(0, C, n)
    y[y == 3] = 4                                   # class 3 absent from the labels
    p = np.where(rng.random(n) < 0.6, y, rng.integers(0, C, n))
    p[p == 6] = 7                                   # class 6 never predicted
    assert 3 in p and 6 in y
    m = evaluate.metrics_from_tally(_counts_of(y.astype(np.int32), p.astype(np.int32), C))
    kw = dict(average="weighted", zero_division=0)
    for name, want in (("accuracy", accuracy_score(y, p)), ("precision", precision_score(y, p, **kw)), ("recall", recall_score(y, p, **kw)),
                       ("f1", f1_score(y, p, **kw))):
        assert abs(m[name] - want) <= 1e-12, (name, m[name], want)
    assert np.array_equal(np.array(m["confusion"]["matrix"]), confusion_matrix(y, p, labels=list(range(C))))
    assert m["per_class"]["3"] == {"precision": 0.0, "recall": 0.0, "f1": 0.0, "support": 0, "accuracy": 0.0}
    assert m["per_class"]["6"]["precision"] == 0.0 and m["per_class"]["6"]["support"] == int((y == 6).sum())
    assert m["top_k"][1] == m["accuracy"] and sorted(m["top_k"]) == [1, 2, 3, 4, 5] and all(m["top_k"][k] <= m["top_k"][k + 1] for k in range(1, 5))
    assert m["loss"] == 0.0 and m["rows"] == n and m["ignored"] == 0 and m["nonfinite"] == 0


def test_metrics_of_an_empty_tally_are_nan_and_do_not_raise():
    for keep in (True, False):
        counts = evaluate.tally_counts(np.zeros(evaluate.tally_layout(5, 6, 10, keep)["words"], np.uint64), 5, 6, 10, keep)
        m = evaluate.metrics_from_tally(counts, ["a", "b", "c", "d", "e"])
        for name in ("accuracy", "precision", "recall", "f1", "loss"):
            assert np.isnan(m[name]), name
        assert all(np.isnan(v) for v in m["top_k"].values()) and np.isnan(m["calibration"]["expected_calibration_error"])
        assert m["calibration"]["maximum_calibration_error"] == 0.0 and m["calibration"]["bin_counts"] == [0.0] * 10
        assert (m["confusion"] is None) == (not keep) and m["per_class"]["c"]["support"] == 0
    # only declined rows: the same
    z = np.array([[0.0, np.inf], [0.0, 1.0]], F32)
    state, _, _ = evaluate.tally_rule(z, np.array([0, 2], np.int32), np.zeros(2, F32), np.zeros(2, F32))
    m = evaluate.metrics_from_tally(evaluate.tally_counts(state, 2))
    assert np.isnan(m["accuracy"]) and m["rows"] == 0 and m["ignored"] == 1 and m["nonfinite"] == 1


def _close(got, want, tol, path=""):
    """Nested dicts / lists: integers and strings exact, floats to `tol`."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), (path, sorted(got), sorted(want))
        for k in want:
            _close(got[k], want[k], tol, path + "/" + str(k))
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), (path, got, want)
        for i, (g, w) in enumerate(zip(got, want)):
            _close(g, w, tol, "%s[%d]" % (path, i))
    elif isinstance(want, float):
        assert abs(float(got) - want) <= tol, (path, got, want)
    else:
        assert got == want and type(got) is type(want), (path, got, want)


def test_metrics_against_the_reference_goldens():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "advanced_metrics.json")))
    C, nb, names = g["num_classes"], g["n_bins"], g["class_names"]
    z, y = np.array(g["logits"], F32), np.array(g["labels"], np.int32)
    conf = np.array(g["confidences"], F32)
    assert z.shape == (200, 7) and 5 not in y and 2 in y
    assert tc.edge_distance(conf.astype(np.float64), nb).min() >= 1e-5 and g["edge_gap"] >= 1e-5
    state, pred, _ = evaluate.tally_rule(z, y, conf, np.zeros(len(y), F32), 6, nb, True)
    assert pred.tolist() == g["predictions"] and 2 not in pred and 5 in pred
    m = evaluate.metrics_from_tally(evaluate.tally_counts(state, C, 6, nb, True), names)
    ref = g["reference"]
    _close(m["per_class"], {k: {f: v for f, v in d.items() if f != "roc_auc"} for k, d in ref["per_class"].items()}, 1e-12, "per_class")
    _close(m["confusion"], ref["confusion"], 1e-12, "confusion")
    cal, want = m["calibration"], ref["calibration"]
    assert cal["bin_counts"] == want["bin_counts"] and cal["n_bins"] == want["n_bins"] == nb
    _close(cal["bin_accuracies"], want["bin_accuracies"], 1e-12, "bin_accuracies")
    # the reference averages fp32 confidences in fp32 (at most log2 N + 1 roundings of 2^-24 on values <= 1); the 2^32 fixed
    # point adds at most 2^-33 per row
    _close(cal["bin_confidences"], want["bin_confidences"], 1e-6, "bin_confidences")
    for name in ("expected_calibration_error", "maximum_calibration_error"):
        assert abs(cal[name] - want[name]) <= 1e-6, (name, cal[name], want[name])


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_tally_entry_points_are_declared_bound_and_element_aligned():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_classify_tally_words", 4), ("frmap_classify_tally", 13), ("frmap_classify_tally_host", 12)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % sym, header)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
        assert hasattr(_lib.load(), sym)
    assert _lib.ABI_VERSION == 10 and _lib.load().frmap_abi_version() == 10
    rows = _lib.ALIGNMENT["frmap_classify_tally"]
    assert list(rows) == ["logits", "labels", "state", "row_pred_out", "row_rank_out", "row_conf_out", "row_loss_out"]
    assert all(cls == "element" for cls, _ in rows.values())
    assert {a: n for a, (_, n) in rows.items()} == {"logits": 4, "labels": 4, "state": 8, "row_pred_out": 4, "row_rank_out": 4,
                                                    "row_conf_out": 4, "row_loss_out": 4}
    assert "frmap_classify_tally_host" not in _lib.ALIGNMENT and "frmap_classify_tally_words" not in _lib.ALIGNMENT
    build = open(os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc", "build.sh")).read()
    assert " classify_tally.hip " in build
    for h in ("tally_rule.h", "tally_twin.h"):
        assert os.path.isfile(os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc", h))
    for name in ("classify_tally", "classify_tally_layout", "classify_tally_words", "classify_tally_host"):
        assert callable(getattr(ops, name))
    for name in ("ClassificationTally", "tally_rule", "tally_rows_reference", "metrics_from_tally", "evaluate_stream"):
        assert callable(getattr(evaluate, name))
    with pytest.raises(ValueError, match="siamese"):
        evaluate.evaluate_stream(None, "siamese", [])
