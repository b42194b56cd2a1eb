"""CPU: the exact verification counts' contract (`frmap_verify_counts[_packed]`, `ops.verify_counts`), pinned by a numpy reference,
the metric derivation of `evaluate.metrics_from_counts` against sklearn / a numpy restatement, the label-histogram totals and the
new C symbols' declarations.

The reference (`ref_verify_counts`, also used by `test_verify_gpu.py`): d2 by `exact_d2` of `test_match_topk_cpu.py` (fp32
elements (a - b) + 1e-6, squares summed in float64), dist = fp32(sqrt(d2)), accepted at t iff dist <= t (NaN / inf never)."""
import os
import re

import numpy as np
import pytest

from frmap_amd import _lib, evaluate

from test_match_topk_cpu import exact_d2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pair_dists(a, labels_a, b=None, labels_b=None, a_row0=None):
    """(dist fp32 [n], genuine bool [n]) of the counted pairs."""
    a = np.asarray(a, np.float32)
    la = np.asarray(labels_a).reshape(-1)
    if b is None:
        b, lb, a_row0 = a, la, 0
    else:
        b, lb = np.asarray(b, np.float32), np.asarray(labels_b).reshape(-1)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return np.zeros(0, np.float32), np.zeros(0, bool)
    d2 = exact_d2(a, b)
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(d2).astype(np.float32)
    gen = la[:, None] == lb[None, :]
    if a_row0 is not None:
        i = np.arange(a.shape[0])[:, None] + a_row0
        j = np.arange(b.shape[0])[None, :]
        keep = i < j
        return dist[keep], gen[keep]
    return dist.reshape(-1), gen.reshape(-1)


def ref_verify_counts(a, labels_a, thresholds, b=None, labels_b=None, a_row0=None):
    """int64 [2, T]: genuine / impostor pairs with dist <= t_k."""
    dist, gen = pair_dists(a, labels_a, b, labels_b, a_row0)
    t = np.asarray(thresholds, np.float32)
    out = np.zeros((2, t.shape[0]), np.int64)
    for c, sel in enumerate((gen, ~gen)):
        d = np.sort(dist[sel][np.isfinite(dist[sel])])
        out[c] = np.searchsorted(d, t, side="right")
    return out


def test_reference_counts_small_case():
    a = np.zeros((4, 4), np.float32)
    a[1, 0] = 1.0
    a[2, 0] = 3.0
    a[3, 0] = np.nan
    lab = np.array([0, 0, 1, 1])
    t = np.array([0.5, 1.0, 2.0, 3.0], np.float32)
    d01 = np.float32(np.sqrt(exact_d2(a[:1], a[1:2])[0, 0]))
    assert d01 <= 1.0 + 1e-6
    c = ref_verify_counts(a, lab, t)
    # pairs: (0,1) genuine ~1, (0,2) impostor ~3, (0,3) NaN, (1,2) impostor ~2, (1,3) NaN, (2,3) NaN genuine
    assert c[0].tolist() == [0, int(d01 <= 1.0), 1, 1]
    d02 = np.float32(np.sqrt(exact_d2(a[:1], a[2:3])[0, 0]))
    d12 = np.float32(np.sqrt(exact_d2(a[1:2], a[2:3])[0, 0]))
    assert c[1].tolist() == [0, 0, int(d12 <= 2.0), int(d12 <= 3.0) + int(d02 <= 3.0)]
    # shards over a_row0 sum to the whole; cross mode counts every ordered pair, the diagonal included
    full = ref_verify_counts(a, lab, t)
    parts = ref_verify_counts(a[:2], lab[:2], t, a, lab, a_row0=0) + ref_verify_counts(a[2:], lab[2:], t, a, lab, a_row0=2)
    assert (parts == full).all()
    cross = ref_verify_counts(a, lab, t, a, lab)
    assert cross[0, 0] == 3                                          # (0,0) (1,1) (2,2) at ~2e-6
    assert cross[1, -1] == 3                                         # (0,2) (1,2) (2,1); (2,0) is 3 + 1e-6 > 3


def test_pair_totals_from_label_histograms():
    rng = np.random.default_rng(3)
    la = rng.integers(0, 7, 50)
    lb = rng.integers(0, 9, 31)
    G, I = evaluate.pair_totals(la)
    gen = la[:, None] == la[None, :]
    iu = np.triu_indices(50, 1)
    assert G == int(gen[iu].sum()) and I == len(iu[0]) - G
    G, I = evaluate.pair_totals(la, lb)
    gen = la[:, None] == lb[None, :]
    assert G == int(gen.sum()) and I == gen.size - G
    assert evaluate.pair_totals([]) == (0, 0)
    assert evaluate.pair_totals([5]) == (0, 0)


def _case(seed, n=120, d=16, ids=12):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((ids, d)).astype(np.float32)
    lab = rng.integers(0, ids, n)
    x = (centres[lab] + 0.6 * rng.standard_normal((n, d))).astype(np.float32)
    return x, lab


def test_roc_auc_equals_sklearn_on_the_full_grid():
    from sklearn.metrics import roc_auc_score
    x, lab = _case(11)
    dist, gen = pair_dists(x, lab)
    grid = np.unique(dist[np.isfinite(dist)])
    counts = ref_verify_counts(x, lab, grid)
    G, I = evaluate.pair_totals(lab)
    m = evaluate.metrics_from_counts(grid, counts, G, I)
    assert m["genuine_pairs"] == int(gen.sum()) and m["impostor_pairs"] == int((~gen).sum())
    assert abs(m["roc_auc"] - roc_auc_score(gen.astype(int), -dist.astype(np.float64))) <= 1e-12


def test_eer_and_tar_at_far_match_a_numpy_restatement():
    x, lab = _case(12)
    dist, gen = pair_dists(x, lab)
    grid = np.unique(dist)
    counts = ref_verify_counts(x, lab, grid)
    G, I = evaluate.pair_totals(lab)
    targets = (0.5, 1e-1, 1e-2, 1e-3, 1e-4)
    m = evaluate.metrics_from_counts(grid, counts, G, I, far_targets=targets)
    gd, idist = np.sort(dist[gen]), np.sort(dist[~gen])
    tar = np.array([(gd <= t).mean() for t in grid])
    far = np.array([(idist <= t).mean() for t in grid])
    assert np.array_equal(m["tar"], tar) and np.array_equal(m["far"], far)
    frr = 1 - tar
    k = int(np.argmax(far >= frr))
    assert far[k] >= frr[k] and (k == 0 or far[k - 1] < frr[k - 1])
    w = (frr[k - 1] - far[k - 1]) / ((far[k] - far[k - 1]) - (frr[k] - frr[k - 1]))
    assert abs(m["eer"] - (far[k - 1] + w * (far[k] - far[k - 1]))) <= 1e-12
    assert abs(m["eer_threshold"] - (grid[k - 1] + w * (float(grid[k]) - float(grid[k - 1])))) <= 1e-9
    for f in targets:
        ok = [i for i in range(len(grid)) if far[i] <= f]
        want = (float(grid[ok[-1]]), float(tar[ok[-1]])) if ok else None
        assert m["tar_at_far"][f] == want, f
    acc = (counts[0] + (I - counts[1])) / (G + I)
    assert m["best_accuracy"] == acc.max() and m["best_threshold"] == float(grid[int(np.argmax(acc))])


def test_metrics_edge_cases():
    t = np.array([0.0, 1.0], np.float32)
    m = evaluate.metrics_from_counts(t, np.zeros((2, 2), np.int64), 0, 5)
    assert np.isnan(m["roc_auc"]) and np.isnan(m["eer"])
    m = evaluate.metrics_from_counts(t, np.array([[1, 2], [0, 0]]), 2, 3, far_targets=(0.0,))
    assert m["tar_at_far"][0.0] == (1.0, 1.0) and m["roc_auc"] == 1.0


def test_default_grid_covers_every_distance():
    import torch
    x, lab = _case(13)
    x[5] = np.nan
    t = evaluate.default_thresholds(torch.from_numpy(x))
    assert t.dtype == np.float32 and 1 <= len(t) <= 1024 and (np.diff(t) > 0).all() and t[0] == 0.0
    dist, _ = pair_dists(x, lab)
    assert dist[np.isfinite(dist)].max() <= t[-1]


def test_verify_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_verify_workspace_bytes", 4), ("frmap_verify_counts", 14), ("frmap_verify_counts_packed", 16)):
        m = re.search(r"\b" + sym + r"\s*\(([^;]*)\);", header)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
    assert _lib.ABI_VERSION == 10


def test_ops_exposes_the_threshold_limit():
    from frmap_amd import ops
    assert ops.VERIFY_MAX_THRESHOLDS >= 1024
    with pytest.raises(ValueError):
        ops.verify_thresholds([0.5, 0.5], "cpu")
    with pytest.raises(ValueError):
        ops.verify_thresholds([float("nan")], "cpu")
    with pytest.raises(ValueError):
        ops.verify_thresholds([-1.0], "cpu")
    with pytest.raises(ValueError):
        ops.verify_thresholds([], "cpu")
    with pytest.raises(ValueError):
        ops.verify_thresholds(np.arange(ops.VERIFY_MAX_THRESHOLDS + 1, dtype=np.float32), "cpu")
    assert ops.verify_thresholds([0.0, 1.0], "cpu").tolist() == [0.0, 1.0]
