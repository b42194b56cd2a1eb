"""Shared code of the one-vs-rest rank-count tests (`test_ovr_cpu.py`, `test_ovr_gpu.py`).  A plain helper module like
`tally_cases.py` and `guard.py` (no fixture, no setting).

* `SWEEP_*`: the grid of tools/ovr_rank_check.cpp (N x C x the three kinds of score).
* `rows(seed, N, C, kind)`: scores and labels for the sweep - continuous (no ties to speak of), quantised to 1/4 (most pairs
  tie) or all equal - with declined rows interleaved: labels -1, C and 2^31 - 1, a NaN, an inf and a -inf under valid labels,
  and a row that is both out of range and non-finite (ignored, not nonfinite).
* `softmax_rows` / `multinomial_rows`: probability rows with every class present, for the comparison with sklearn: float32
  softmax rows, and rows of eighths that sum to exactly 1 and tie in every row.
* `special_rows`: +-0.0, denormals and FLT_MAX in every column.
* `store_of`: the class-major store and the stored labels `frmap_ovr_append` would write, in numpy.
* `HAND`: six rows with every integer written out.
"""
import numpy as np

from frmap_amd import evaluate

SWEEP_N = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1025)
SWEEP_C = (1, 2, 3, 36, 65)
KINDS = ("continuous", "quantised", "equal")
SPLIT = (1, 65)                     # 1 + 64 + 194 rows
B_FULL = 259
F32 = np.float32
FLT_MAX = np.finfo(F32).max
DENORMAL = F32(1e-45)               # the smallest positive fp32 denormal

# r0, r1: class 0, tied within the class at 0.5; r2 ties with them across classes; column 1 sets +0.0 against -0.0 (equal) and a
# denormal against 0 (not equal); r4 is ignored whatever its scores are, r5 holds a NaN
HAND_SCORES = np.array([[0.5, -0.0, 0.0],
                        [0.5, DENORMAL, 0.25],
                        [0.5, 0.0, -0.0],
                        [DENORMAL, -0.0, 0.75],
                        [9.0, 9.0, 9.0],
                        [0.0, np.nan, 1.0]], F32)
HAND_LABELS = np.array([0, 0, 1, 1, -1, 2], np.int32)
HAND = {"ge_same": [2, 2, 2, 2, 0, 0], "ge_other": [1, 1, 2, 2, 0, 0], "eq_other": [1, 1, 1, 1, 0, 0], "why": [0, 0, 0, 0, 1, 2],
        "stored": [0, 0, 1, 1, -1, -2],
        # class 0: 2 positives, 2 negatives, one negative tied with both: (2 + 2 / 2) / 4; precision 2 / 3 at both positives
        # class 1: both negatives at or above both positives, one of them tied with each: (0 + 2 / 2) / 4; precision 2 / 4
        "roc_auc": [0.75, 0.25, np.nan], "average_precision": [2.0 / 3.0, 0.5, np.nan], "support": [2, 2, 0]}


def rows(seed, N, C, kind):
    rng = np.random.default_rng([seed, N, C, KINDS.index(kind)])
    if kind == "continuous":
        z = rng.standard_normal((N, C)).astype(F32)
    elif kind == "quantised":
        z = (rng.integers(0, 5, (N, C)) * 0.25).astype(F32)
    else:
        z = np.full((N, C), 0.375, F32)
    y = rng.integers(0, C, N).astype(np.int32)
    i = np.arange(N)
    y[i % 11 == 3] = -1
    y[i % 11 == 5] = C
    y[i % 11 == 6] = 2 ** 31 - 1
    for k, v in ((7, np.nan), (8, np.inf), (9, -np.inf)):
        at = np.nonzero(i % 11 == k)[0]
        z[at, rng.integers(0, C, len(at))] = v
    both = i % 22 == 14
    y[both] = -5
    z[both, 0] = np.nan
    return z, y


def all_classes(rng, N, C):
    """N >= C labels in which every class occurs."""
    assert N >= C
    return rng.permutation(np.arange(N) % C).astype(np.int32)


def softmax_rows(seed, N, C):
    rng = np.random.default_rng([seed, N, C])
    y = all_classes(rng, N, C)
    z = rng.standard_normal((N, C)) * 1.5
    z[np.arange(N), y] += 1.0
    p = np.exp(z - z.max(axis=1, keepdims=True))
    return (p / p.sum(axis=1, keepdims=True)).astype(F32), y


def multinomial_rows(seed, N, C, parts=8):
    """Rows of multiples of 1 / parts that sum to exactly 1: ties in every row and down every column."""
    rng = np.random.default_rng([seed, N, C, parts])
    y = all_classes(rng, N, C)
    p = np.full(C, 1.0 / C)
    z = np.stack([rng.multinomial(parts, p) for _ in range(N)]).astype(F32) / F32(parts)
    assert (z.sum(axis=1) == 1.0).all()
    return z, y


def special_rows(seed, N, C):
    rng = np.random.default_rng([seed, N, C, 99])
    pool = np.array([0.0, -0.0, DENORMAL, -DENORMAL, 2 * DENORMAL, FLT_MAX, -FLT_MAX, np.finfo(F32).tiny, 1.0], F32)
    z = pool[rng.integers(0, len(pool), (N, C))]
    return z, rng.integers(0, C, N).astype(np.int32)


def store_of(scores, labels, capacity=None):
    """(store float32 [C, capacity], stored labels int32 [capacity]) holding the rows at [0, N): what the append writes; the rest
    of the store is NaN and the rest of the labels 7 (rows >= n must not be read)."""
    z = np.asarray(scores, F32)
    N, C = z.shape
    cap = max(N, 1) if capacity is None else int(capacity)
    store = np.full((C, cap), np.nan, F32)
    store[:, :N] = z.T
    stored = np.full(cap, 7, np.int32)
    stored[:N] = evaluate.ovr_stored_labels(z, labels)
    return store, stored


def sklearn_per_class(scores, labels, C):
    """(roc_auc [C] through roc_curve + auc, average precision [C] through the binary average_precision_score)."""
    from sklearn.metrics import auc, average_precision_score, roc_curve
    y = np.asarray(labels)
    roc, ap = np.zeros(C), np.zeros(C)
    for c in range(C):
        fpr, tpr, _ = roc_curve(y == c, scores[:, c])
        roc[c] = auc(fpr, tpr)
        ap[c] = average_precision_score(y == c, scores[:, c])
    return roc, ap
