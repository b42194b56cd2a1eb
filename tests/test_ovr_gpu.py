"""GPU: the score store and the pair count (`ops.ovr_append`, `ops.ovr_rank_counts`, csrc/ovr_rank.hip) against the rule of
`evaluate.ovr_rank_rule`.

* Append: the store equals `scores.T` bit for bit and the stored labels follow the rule, B in {1, 5, 64, 65, 259} x C in
  {1, 2, 36, 63, 64, 65, 129, 1000} at `first` in {0, 1, 77}; everything outside the appended rows is untouched.
* Counts: equal to the numpy rule on the device's own stored bits and word for word to the host twin, over the N x C x kind grid
  of the CPU sweep, plus 4096 rows of one class, a class with no positive, scores quantised to 1/4, +-0.0 / denormals / FLT_MAX
  and declined rows interleaved.
* Invariance under the split into appends, the order of the rows, `merge`, a second run and growth past the capacity.
* Guard bands and placement at element alignment for both launches, one store past 4 GiB, and `evaluate_stream(auc=True)`
  against `evaluate_model` and sklearn.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import big_cases as bc  # noqa: E402
import guard  # noqa: E402
import ovr_cases as oc  # noqa: E402
import frmap_amd  # noqa: E402
from frmap_amd import evaluate, ops  # noqa: E402

DEV = "cuda"
F32 = np.float32
SENTINEL_BITS, SENTINEL_LABEL = 0x7FC12345, 123456          # a NaN pattern no score holds, a label no row holds


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _fresh(C, cap):
    store = torch.full((C, cap), SENTINEL_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    return store, torch.full((cap,), SENTINEL_LABEL, dtype=torch.int32, device=DEV)


def _filled(z, y, cap=None, cuts=()):
    """A device store holding the rows of z / y at [0, N), appended in the pieces `cuts` names."""
    N, C = z.shape
    store, lab = _fresh(C, max(N, 1) if cap is None else cap)
    for lo, hi in zip((0,) + tuple(cuts), tuple(cuts) + (N,)):
        if hi > lo:
            ops.ovr_append(t(z[lo:hi]).to(DEV), t(y[lo:hi]).to(DEV), store, lab, lo)
    return store, lab


def _counts(store, lab, n):
    out = ops.ovr_rank_counts(store, lab, n)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy().view(np.uint64) for o in out)


def _check_counts(store, lab, n, what):
    """The device's counts against the numpy rule on the device's own stored bits, and against the twin word for word."""
    got = _counts(store, lab, n)
    s, l = store.cpu().numpy(), lab.cpu().numpy()
    want = evaluate.ovr_rank_rule(s[:, :n].T, l[:n])
    twin = ops.ovr_rank_counts_host(s, l, n)
    for k, name in enumerate(("ge_same", "ge_other", "eq_other")):
        assert np.array_equal(got[k], want[k]), (what, name, np.nonzero(got[k] != want[k])[0][:8], got[k][:8], want[k][:8])
        assert np.array_equal(got[k], twin[k]), (what, name, "twin")
    return got, want[3]


# ---------------------------------------------------------------------------------------------------------------------------------
# append
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 5, 64, 65, 259))
@pytest.mark.parametrize("C", (1, 2, 36, 63, 64, 65, 129, 1000))
def test_append_writes_the_transpose_the_labels_and_nothing_else(C, B):
    z, y = oc.rows(41, B, C, "continuous")
    want_lab = evaluate.ovr_stored_labels(z, y)
    for first in (0, 1, 77):
        cap = first + B + 5
        store, lab = _fresh(C, cap)
        ops.ovr_append(t(z).to(DEV), t(y).to(DEV), store, lab, first)
        torch.cuda.synchronize()
        s, l = store.cpu().numpy().view(np.uint32), lab.cpu().numpy()
        assert np.array_equal(s[:, first:first + B], np.ascontiguousarray(z.T).view(np.uint32)), (C, B, first)
        assert np.array_equal(l[first:first + B], want_lab), (C, B, first)
        outside = np.ones(cap, bool)
        outside[first:first + B] = False
        assert (s[:, outside] == SENTINEL_BITS).all() and (l[outside] == SENTINEL_LABEL).all(), (C, B, first)
    if B >= 64:
        assert (want_lab == -1).any() and (want_lab == -2).any() and (want_lab >= 0).any()


def test_append_refuses_what_the_header_says():
    store, lab = _fresh(4, 8)
    z, y = torch.zeros((3, 4), device=DEV), torch.zeros((3,), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="capacity"):
        ops.ovr_append(z, y, store, lab, 6)
    with pytest.raises(ValueError, match="first"):
        ops.ovr_append(z, y, store, lab, -1)
    with pytest.raises(ValueError, match="scores"):
        ops.ovr_append(z[:, :3], y, store, lab, 0)
    with pytest.raises(ValueError, match="contiguous"):
        ops.ovr_append(z, y, store[:, ::2], lab[::2], 0)
    with pytest.raises(RuntimeError):
        ops.ovr_append(z.cpu(), y.cpu(), store, lab, 0)                       # host tensors: no CPU fallback
    torch.cuda.synchronize()
    assert bool((store.view(torch.int32) == SENTINEL_BITS).all()) and bool((lab == SENTINEL_LABEL).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# counts
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", oc.SWEEP_C)
def test_counts_equal_the_rule_and_the_twin_over_the_sweep(C):
    for N in oc.SWEEP_N:
        for kind in oc.KINDS:
            z, y = oc.rows(17, N, C, kind)
            store, lab = _filled(z, y, N + 3)                                # three rows of capacity past n: sentinels, never read
            got, why = _check_counts(store, lab, N, (C, N, kind))
            declined = why != 0
            assert not got[0][declined].any() and not got[1][declined].any() and not got[2][declined].any()
            if N >= 64:
                assert declined.any() and (~declined).any() and int(got[0][~declined].min()) >= 1


def test_4096_rows_of_one_class_take_every_add():
    N = 4096
    rng = np.random.default_rng(3)
    for C in (1, 2):
        z = (rng.integers(0, 7, (N, C)) * 0.125).astype(F32)                 # seven values: long runs of ties inside the class
        y = np.zeros(N, np.int32)
        store, lab = _filled(z, y)
        (a, b, e), why = _check_counts(store, lab, N, ("one class", C))
        assert not why.any() and not b.any() and not e.any()                 # every N_c is 0
        col = z[:, 0]
        assert np.array_equal(a, np.array([(col >= v).sum() for v in col], np.uint64)) and int(a.max()) == N
        m = evaluate.ovr_metrics(lab.cpu().numpy(), a, b, e, C)
        assert np.isnan(m["per_class"]["0"]["roc_auc"]) and m["per_class"]["0"]["average_precision"] == 1.0


def test_a_class_with_no_positive_quantised_scores_and_special_values():
    # a class with no positive, scores quantised to 1/4: most pairs tie
    z, y = oc.rows(29, 1025, 3, "quantised")
    y = np.where(y == 1, 2, y).astype(np.int32)
    (a, b, e), why = _check_counts(*_filled(z, y), 1025, "no positive of class 1")
    ok = why == 0
    # two classes of about half the counted rows each, five equally likely values: a row ties with about a tenth of the counted
    # rows across classes; half of that expectation is asked for
    assert int((e[ok] > 0).sum()) > ok.sum() * 9 // 10 and int(e.sum()) > int(ok.sum()) ** 2 // 20
    m = evaluate.ovr_metrics(evaluate.ovr_stored_labels(z, y), a, b, e, 3)
    assert m["per_class"]["1"]["support"] == 0 and np.isnan(m["per_class"]["1"]["roc_auc"]) and np.isfinite(m["per_class"]["0"]["roc_auc"])
    # +-0.0, denormals and FLT_MAX in every column
    for C in (1, 3, 65):
        z, y = oc.special_rows(3, 257, C)
        _, why = _check_counts(*_filled(z, y), 257, ("special", C))
        assert not why.any()
    # the hand-built rows, every integer written out
    (a, b, e), why = _check_counts(*_filled(oc.HAND_SCORES, oc.HAND_LABELS), 6, "hand")
    assert a.tolist() == oc.HAND["ge_same"] and b.tolist() == oc.HAND["ge_other"] and e.tolist() == oc.HAND["eq_other"]


def test_declined_rows_take_part_in_nobodys_count():
    C = 36
    z0, y0 = oc.softmax_rows(11, 200, C)
    base = _counts(*_filled(z0, y0), 200)
    extra = np.full((6, C), 0.999, F32)                                      # scores that would outrank everything, were they counted
    extra[2, 7], extra[3, 35], extra[4, 0] = np.nan, np.inf, -np.inf
    ye = np.array([-1, C, 3, 3, 3, 2 ** 31 - 1], np.int32)
    at = [0, 7, 20, 33, 150, 200]
    z, y = np.insert(z0, at, extra, axis=0), np.insert(y0, at, ye)
    where = np.array([p + k for k, p in enumerate(at)])
    store, lab = _filled(z, y)
    got, why = _check_counts(store, lab, 206, "declined")
    assert lab.cpu().numpy()[where].tolist() == [-1, -1, -2, -2, -2, -1] and why[where].all()
    keep = np.ones(206, bool)
    keep[where] = False
    for k in range(3):
        assert not got[k][where].any() and np.array_equal(got[k][keep], base[k])
    m = evaluate.ovr_metrics(lab.cpu().numpy(), *got, C)
    assert (m["rows"], m["ignored"], m["nonfinite"]) == (200, 3, 3)
    tally = evaluate.ClassificationTally(C).update(t(z).to(DEV), t(y)).counts()     # the tally fed the same batch agrees
    assert (tally["rows"], tally["ignored"], tally["nonfinite"]) == (200, 3, 3)


# ---------------------------------------------------------------------------------------------------------------------------------
# invariance
# ---------------------------------------------------------------------------------------------------------------------------------
def test_split_order_merge_repeat_and_growth():
    C = 36
    z, y = oc.rows(23, oc.B_FULL, C, "quantised")
    once, lab1 = _filled(z, y)
    split, lab3 = _filled(z, y, cuts=oc.SPLIT)                               # 1 + 64 + 194 rows
    assert torch.equal(once.view(torch.int32), split.view(torch.int32)) and torch.equal(lab1, lab3)
    want = _counts(once, lab1, oc.B_FULL)
    again = _counts(once, lab1, oc.B_FULL)
    three = _counts(split, lab3, oc.B_FULL)
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(want, again, three))
    perm = np.random.default_rng(9).permutation(oc.B_FULL)
    moved = _counts(*_filled(z[perm], y[perm]), oc.B_FULL)
    assert all(np.array_equal(m, w[perm]) for m, w in zip(moved, want))
    # OvrScores: growth past the capacity keeps every earlier row; merge is the concatenation
    acc = evaluate.OvrScores(C, capacity=8, device=DEV)
    for lo, hi in zip((0,) + oc.SPLIT, oc.SPLIT + (oc.B_FULL,)):
        acc.update(t(z[lo:hi]).to(DEV), t(y[lo:hi].astype(np.int64)))
    assert acc.rows == oc.B_FULL and acc.capacity >= oc.B_FULL
    assert torch.equal(acc.store[:, :acc.rows].contiguous().view(torch.int32), once.view(torch.int32)) and torch.equal(acc.labels[:acc.rows], lab1)
    labs, a, b, e = acc.rank_counts()
    assert np.array_equal(labs, lab1.cpu().numpy()) and all(np.array_equal(g, w) for g, w in zip((a, b, e), want))
    left = evaluate.OvrScores(C, 100, device=DEV).update(t(z[:100]).to(DEV), t(y[:100]))
    right = evaluate.OvrScores(C, 300, device=DEV).update(t(z[100:]).to(DEV), t(y[100:]))
    merged = left.merge(right).rank_counts()
    assert np.array_equal(merged[0], labs) and all(np.array_equal(g, w) for g, w in zip(merged[1:], want))
    _same(left.metrics(), evaluate.ovr_metrics(labs, *want, C))
    assert left.reset().rows == 0 and all(len(v) == 0 for v in left.rank_counts())
    # a wide label must not wrap into the range
    wide = evaluate.OvrScores(3, 4, device=DEV).update(torch.zeros((2, 3), device=DEV), torch.tensor([2 ** 32 + 1, 1]))
    assert wide.labels[:2].cpu().tolist() == [-1, 1]


# ---------------------------------------------------------------------------------------------------------------------------------
# guard bands and placement
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,B", [(65, 37), (1000, 5), (3, 1025)])
def test_guard_bands_and_placement(C, B):
    z, y = oc.rows(19, B, C, "quantised")
    z, y = t(z), t(y)

    def run(place):
        # scores and labels placed; the store, its labels (capacity = B: fully written) and the three outputs allocated by the
        # patched modules: all between bands
        acc = evaluate.OvrScores(C, B, device=DEV).update(place(z), place(y))
        return (acc.store, acc.labels) + tuple(ops.ovr_rank_counts(acc.store, acc.labels, B))
    ref = guard.two_fills(run, [ops, evaluate], what="ovr_append + ovr_rank_counts")
    assert len(ref) == 5 and ref[0].shape == (C, B) and ref[2].dtype == torch.int64
    want = evaluate.ovr_rank_rule(z.numpy(), y.numpy())
    assert all(np.array_equal(r.numpy().view(np.uint64), w) for r, w in zip(ref[2:], want))
    # every buffer aligned to its element size and not to twice it
    elem = lambda dtype, kind, who: torch.empty((), dtype=dtype).element_size()
    again = guard.shifted(run, [ops, evaluate], what="ovr at element alignment", requirement=elem)
    assert all(guard.first_difference(a, b) is None for a, b in zip(ref, again))


# ---------------------------------------------------------------------------------------------------------------------------------
# offsets past 4 GiB
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_store_past_4_gib():
    """C = 1100 columns of 2^20 rows: 4.6 GB, allocated and not filled.  300 rows appended at the end of every column, the labels of
    all other rows set to -1, the count run over the whole capacity: the counts of the 300 rows are the rule's on those rows."""
    C, cap, B = 1100, 2 ** 20, 300
    first = cap - B
    assert C * cap * 4 > 2 ** 32 and (C - 1) * cap > 2 ** 30
    bc.need_memory(bc.estimate_bytes([C * cap * 4, cap * 4, 3 * cap * 8, 4 * cap * 8]), "ovr-big")
    store = lab = out = None
    try:
        store = torch.empty((C, cap), dtype=torch.float32, device=DEV)
        lab = torch.empty((cap,), dtype=torch.int32, device=DEV)
        lab.fill_(-1)
        rng = np.random.default_rng(13)
        z = (rng.integers(0, 5, (B, C)) * 0.25).astype(F32)                  # five values: ties within and across classes
        y = rng.integers(0, C, B).astype(np.int32)
        y[::3] = np.where(np.arange(len(y[::3])) % 2 == 0, 0, C - 1)         # a third of the rows share the first and the last column
        y[5], z[9, C - 1] = C, np.inf
        ops.ovr_append(t(z).to(DEV), t(y).to(DEV), store, lab, first)
        out = ops.ovr_rank_counts(store, lab, cap)
        torch.cuda.synchronize()
        for c in (0, 1, C // 2, C - 2, C - 1):                               # the last columns lie past 4 GiB
            assert np.array_equal(store[c, first:].cpu().numpy().view(np.uint32), np.ascontiguousarray(z[:, c]).view(np.uint32)), c
        assert lab[first:].cpu().tolist() == evaluate.ovr_stored_labels(z, y).tolist() and bool((lab[:first] == -1).all())
        want = evaluate.ovr_rank_rule(z, y)
        assert want[3].tolist().count(1) == 1 and want[3].tolist().count(2) == 1
        for k in range(3):
            assert not bool(out[k][:first].any()), k
            assert np.array_equal(out[k][first:].cpu().numpy().view(np.uint64), want[k]), k
    finally:
        del store, lab, out
        bc.release()


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _same(a, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (path, list(a), list(b))
        for k in a:
            _same(a[k], b[k], path + "/" + str(k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, w) in enumerate(zip(a, b)):
            _same(x, w, "%s[%d]" % (path, i))
    elif isinstance(a, float) and np.isnan(a):
        assert isinstance(b, float) and np.isnan(b), path
    else:
        assert a == b and type(a) is type(b), (path, a, b)


@pytest.mark.parametrize("mt", ["cnn", "arcface"])
def test_evaluate_stream_with_auc_against_evaluate_model(mt, calibrated_sd):
    from frmap_amd import synth
    C, n = 36, 75                                                           # batches of 32, 32 and 11
    m = frmap_amd.get_model(mt, C)
    m.load_state_dict(calibrated_sd(mt))
    m = m.to(DEV).eval().set_compute_dtype(torch.float16)
    x = synth.randn(77, (n, 3, 64, 64), "tally-eval")
    lab = torch.from_numpy(oc.all_classes(np.random.default_rng(78), n, C).astype(np.int64))   # every class has a sample: sklearn defines both
    batches = [(x[lo:lo + 32], lab[lo:lo + 32]) for lo in range(0, n, 32)]
    res = evaluate.evaluate_model(m, mt, batches)
    plain = evaluate.evaluate_stream(m, mt, batches)
    got = evaluate.evaluate_stream(m, mt, batches, auc=True)
    print("\nevaluate_stream(auc=True) %s: roc_auc %.17g (evaluate_model %.17g), pr_auc %.17g (evaluate_model %.17g)"
          % (mt, got["roc_auc"], res["metrics"]["roc_auc"], got["pr_auc"], res["metrics"]["pr_auc"]))
    assert np.isfinite(res["metrics"]["roc_auc"]) and np.isfinite(res["metrics"]["pr_auc"])
    assert abs(got["roc_auc"] - res["metrics"]["roc_auc"]) <= 1e-12 and abs(got["pr_auc"] - res["metrics"]["pr_auc"]) <= 1e-12
    # per class: sklearn on the probabilities `ops.softmax_argmax` gave evaluate_model
    probs = np.array(res["probabilities"], F32)
    roc, ap = oc.sklearn_per_class(probs, lab.numpy(), C)
    for c in range(C):
        entry = got["per_class"][str(c)]
        assert abs(entry["roc_auc"] - roc[c]) <= 1e-12 and abs(entry["average_precision"] - ap[c]) <= 1e-12, (c, entry, roc[c], ap[c])
    # auc=False: the dict from before this feature - and auc=True adds to it, changing nothing
    assert "roc_auc" not in plain and "pr_auc" not in plain
    assert all(sorted(v) == ["accuracy", "f1", "precision", "recall", "support"] for v in plain["per_class"].values())
    stripped = {k: v for k, v in got.items() if k not in ("roc_auc", "pr_auc")}
    stripped["per_class"] = {k: {f: v for f, v in d.items() if f not in ("roc_auc", "average_precision")} for k, d in got["per_class"].items()}
    _same(stripped, plain)
    # labels that leave classes empty: NaN, where evaluate_model's metric block reports NaN
    few = torch.from_numpy(np.random.default_rng(78).integers(0, C, n))
    assert len(np.unique(few.numpy())) < C
    acc = evaluate.OvrScores(C, n, device=DEV).update(t(probs).to(DEV), few).metrics()
    ref = evaluate.classification_metrics(few.numpy(), np.array(res["predictions"]), probs.astype(np.float64))
    assert np.isnan(ref["roc_auc"]) and np.isnan(acc["roc_auc"]) and np.isnan(ref["pr_auc"]) and np.isnan(acc["pr_auc"])
