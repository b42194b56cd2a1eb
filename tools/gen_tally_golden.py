#!/usr/bin/env python3
"""Write tests/golden/advanced_metrics.json: the reference's own `expected_calibration_error`, `calculate_per_class_metrics` and
`create_enhanced_confusion_matrix` (src/advanced_metrics.py) on seeded inputs, for `tests/test_tally_cpu.py` to hold
`evaluate.metrics_from_tally` against.  Runs only where the reference tree is present (`oracle.ref_loader.available()`); each
function is compiled on its own from the reference's source by `oracle.ref_loader.load_reference_function` - the module around
them imports pandas and the reference's package - with numpy, a logger, the typing names and the four sklearn functions they
use in the namespace.  The file holds numbers only.

Inputs: N = 200 samples, C = 7 classes, fp32 logits from a seeded generator with the target raised; class 5 never occurs in the
labels (but is predicted), class 2 is never predicted (but occurs in the labels), so every class is in sklearn's label union and
the reference's matrix is 7 x 7.  The scores are the fp32 softmax of the logits and the predictions their first arg-max.  No
confidence may lie within 1e-5 of a bin edge (asserted): the goldens must not depend on the last bits of a softmax."""
import json
import logging
import os
import sys
import typing

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

N, C, N_BINS, SEED = 200, 7, 10, 20251019
ABSENT, NEVER_PREDICTED = 5, 2


def inputs():
    rng = np.random.default_rng(SEED)
    y = rng.integers(0, C - 1, N)
    y = np.where(y >= ABSENT, y + 1, y).astype(np.int64)              # 0 ... 6 without 5
    z = (rng.standard_normal((N, C)) * 2.0).astype(np.float32)
    z[np.arange(N), y] += np.float32(1.5)
    z[:, NEVER_PREDICTED] -= np.float32(100.0)
    e = np.exp(z - z.max(axis=1, keepdims=True), dtype=np.float32)
    score = (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)
    pred = score.argmax(axis=1).astype(np.int64)
    assert np.array_equal(pred, z.argmax(axis=1))
    return z, y, score, pred


def clean(v):
    """Tuples to lists, numpy scalars to Python numbers, NaN to None: what JSON can hold."""
    if isinstance(v, dict):
        return {str(k): clean(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [clean(x) for x in v]
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return None if np.isnan(v) else float(v)
    return v


def main():
    if not ref_loader.available():
        sys.exit("the reference tree is not present: nothing to generate from")
    from sklearn.metrics import auc, confusion_matrix, precision_recall_fscore_support, roc_curve
    src = os.path.join(os.path.dirname(ref_loader.REF_FILE), "advanced_metrics.py")
    ns = {"np": np, "logger": logging.getLogger("gen_tally_golden"), "auc": auc, "confusion_matrix": confusion_matrix,
          "precision_recall_fscore_support": precision_recall_fscore_support, "roc_curve": roc_curve}
    ns.update({k: getattr(typing, k) for k in ("Dict", "List", "Tuple", "Optional", "Union", "Any")})
    fn = {name: ref_loader.load_reference_function(src, name, ns)
          for name in ("expected_calibration_error", "calculate_per_class_metrics", "create_enhanced_confusion_matrix")}
    z, y, score, pred = inputs()
    names = ["c%d" % i for i in range(C)]
    assert ABSENT not in y and ABSENT in pred and NEVER_PREDICTED in y and NEVER_PREDICTED not in pred
    assert set(y.tolist()) | set(pred.tolist()) == set(range(C))
    conf = score[np.arange(N), pred]
    edge_gap = float(np.abs(conf.astype(np.float64)[:, None] - np.linspace(0, 1, N_BINS)[None, :]).min())
    assert edge_gap >= 1e-5, edge_gap
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # (the one-vs-rest ROC of a class without samples)
        out = {"calibration": fn["expected_calibration_error"](y, pred, score, N_BINS),
               "per_class": fn["calculate_per_class_metrics"](y, pred, score, names),
               "confusion": fn["create_enhanced_confusion_matrix"](y, pred, names)}
    doc = {"n": N, "num_classes": C, "n_bins": N_BINS, "seed": SEED, "class_names": names, "edge_gap": edge_gap,
           "logits": [[float(v) for v in row] for row in z], "labels": y.tolist(), "predictions": pred.tolist(),
           "confidences": [float(v) for v in conf], "reference": clean(out)}
    path = os.path.join(ROOT, "tests", "golden", "advanced_metrics.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, allow_nan=False)
        f.write("\n")
    print("wrote %s (%d bytes), smallest distance of a confidence to a bin edge %.3g" % (path, os.path.getsize(path), edge_gap))


if __name__ == "__main__":
    main()
