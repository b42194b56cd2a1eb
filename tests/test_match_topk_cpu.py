"""CPU: the exact top-k search's contract (`frmap_match_topk[_packed]`, `ops.match_topk`, `matching.search_batch` /
`compare_faces_topk`) pinned by a numpy reference, `Gallery` label numbering, and the new C symbols' declarations.

The reference (`ref_topk`, also used by `test_match_topk_gpu.py`): elements (a - g) + 1e-6 in fp32, squares summed in float64,
rows with a NaN / inf distance never listed, order (d2, row) by `np.lexsort`; identity mode keeps per label the min d2 and the
first row attaining it."""
import os
import re

import numpy as np
import torch

from frmap_amd import _lib, matching
from oracle import face_oracle as fo

import match_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exact_d2(probes, gal):
    """[P, G] float64: fp32 ((a - g) + 1e-6), squares summed in float64 (one probe at a time: bounded memory)."""
    a = np.asarray(probes, dtype=np.float32)
    g = np.asarray(gal, dtype=np.float32).reshape(-1, a.shape[1])
    out = np.empty((a.shape[0], g.shape[0]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(a.shape[0]):
            diff = (a[p][None, :] - g) + np.float32(1e-6)
            out[p] = (diff.astype(np.float64) ** 2).sum(axis=1)
    return out


def ref_topk(probes, gal, k, labels=None):
    """(idx int64 [P, k], dist float64 [P, k], label int64 [P, k]) as the C ABI documents them."""
    d2 = exact_d2(probes, gal)
    P, G = d2.shape
    idx = np.full((P, k), -1, dtype=np.int64)
    dist = np.full((P, k), np.inf, dtype=np.float64)
    lab = np.full((P, k), -1, dtype=np.int64)
    rows = np.arange(G)
    for p in range(P):
        ok = np.isfinite(d2[p])
        r, d = rows[ok], d2[p][ok]
        order = np.lexsort((r, d))
        if labels is None:
            sel = r[order][:k]
        else:
            ls = np.asarray(labels)[r][order]
            _, first = np.unique(ls, return_index=True)       # first position of each label in (d2, row) order
            sel = r[order][np.sort(first)][:k]
            lab[p, :len(sel)] = np.asarray(labels)[sel]
        idx[p, :len(sel)] = sel
        dist[p, :len(sel)] = np.sqrt(d2[p][sel])
    return idx, dist, lab


def test_reference_k1_is_the_reference_loop():
    for G, D, kind in mc.CASES:
        probes, gal, notes = mc.build_case(G, D, kind, 4242 + G + D)
        ref_idx, ref_dist = mc.reference_top1(fo, probes, gal)
        idx, dist, _ = ref_topk(probes.numpy(), gal.numpy(), 1)
        assert idx[:, 0].tolist() == ref_idx.tolist(), (G, D, kind)
        assert np.all(np.abs(dist[:, 0] - ref_dist.numpy()) <= 2e-6 + 1e-6 * ref_dist.numpy()), (G, D, kind)


def test_reference_entry_and_identity_semantics():
    D = 8
    base = np.zeros((1, D), dtype=np.float32)
    gal = np.zeros((9, D), dtype=np.float32)
    gal[0, 0] = 3.0           # label 0, far
    gal[1, 0] = 1.0           # label 1
    gal[2, 0] = 1.0           # label 1, bit-identical duplicate of row 1 (tie -> lower row)
    gal[3, 0] = 2.0           # label 2
    gal[4, 0] = np.nan        # label 3, never listed
    gal[5, 0] = 0.5           # label 0, its nearest row
    gal[6, 0] = 2.0           # label 4, ties label 2 (its row 3 is lower)
    gal[7, 0] = np.inf        # label 3, never listed
    gal[8, 0] = 0.5           # label 0 again: same distance as row 5, higher row
    labels = np.array([0, 1, 1, 2, 3, 0, 4, 3, 0])
    idx, dist, _ = ref_topk(base, gal, 8)
    assert idx[0].tolist() == [5, 8, 1, 2, 3, 6, 0, -1]                # NaN / inf rows padded away
    assert np.isinf(dist[0, -1]) and dist[0, 0] == dist[0, 1]
    idx, dist, lab = ref_topk(base, gal, 6, labels)
    assert idx[0].tolist() == [5, 1, 3, 6, -1, -1]                     # k > identities with a finite distance
    assert lab[0].tolist() == [0, 1, 2, 4, -1, -1]
    idx, _, lab = ref_topk(base, gal, 2, labels)
    assert idx[0].tolist() == [5, 1] and lab[0].tolist() == [0, 1]
    idx, dist, lab = ref_topk(base, np.zeros((0, D), np.float32), 3, np.zeros(0, np.int64))
    assert idx[0].tolist() == [-1, -1, -1] and np.isinf(dist).all()


def test_gallery_label_numbering_and_append():
    names = ["alice", "bob", "alice", "carol", "bob", "random3", "random3"]
    g = matching.Gallery(names, torch.randn(len(names), 16), device="cpu")
    assert g.label_names == ["alice", "bob", "carol", "random3"]
    assert g.label_ids == [0, 1, 0, 2, 1, 3, 3]
    assert g.labels.dtype == torch.int32 and g.labels.tolist() == [0, 1, 0, 2, 1, 3, 3]
    assert g.append("dave", torch.randn(16)) == 7
    assert g.append("bob", torch.randn(16)) == 8
    assert g.labels.tolist() == [0, 1, 0, 2, 1, 3, 3, 4, 1] and g.label_names[4] == "dave"
    for _ in range(40):                                   # past the buffer's capacity: labels follow the rows
        g.append("erin", torch.randn(16))
    assert len(g.labels) == len(g) == 49 and g.labels[-1].item() == 5
    assert all(g.label_names[lab] == n for lab, n in zip(g.labels.tolist(), g.names))
    g2 = matching.Gallery.from_refs([], device="cpu")
    assert g2.labels.tolist() == [] and g2.label_names == []


def test_reference_gallery_names_hold_a_duplicate():
    import json
    refs = json.load(open(os.path.join(ROOT, "tests", "golden", "face_references.json")))
    names = [r["name"] for r in refs] if isinstance(refs, list) else refs["names"]
    g = matching.Gallery(names, torch.zeros(len(names), 4), device="cpu")
    assert names.count("random3") == 2 and g.label_names.count("random3") == 1
    assert len(g.label_names) == len(set(names))


def test_topk_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_match_topk_workspace_bytes", 4), ("frmap_match_topk", 12), ("frmap_match_topk_packed", 14),
                       ("frmap_model_search_workspace_bytes", 6), ("frmap_model_embed_and_search", 19)):
        m = re.search(r"\b" + sym + r"\s*\(([^;]*)\);", header)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
    assert _lib.ABI_VERSION == 10
