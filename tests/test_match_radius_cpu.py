"""CPU: the exact threshold search's contract (`frmap_match_radius[_packed]`, `ops.match_radius`, `matching.search_radius` /
`duplicate_pairs` / `cluster_embeddings`) pinned by a numpy reference, the host logic behind the matching functions, and the new
C symbols' declarations.

The reference (`ref_radius`, also used by `test_match_radius_gpu.py`): d2 by `exact_d2` of `test_match_topk_cpu.py` (fp32 elements
(a - b) + 1e-6, squares summed in float64) exactly as `pair_dists` of `test_verify_cpu.py` forms it, dist = fp32(sqrt(d2)), a counted
pair is accepted iff dist <= fp32(thresh) (NaN / inf never).

Knife-edges: the device sums the squares in float64 in another order than numpy, so the two d2 can differ by a few 2^-53.  A pair
could be decided differently only if fp32(sqrt(d2 (1 - 2^-40))) <= t and fp32(sqrt(d2 (1 + 2^-40))) <= t differ (2^-40: ample for
the ~2^-44 that summing 1000 squares in any order can move a float64 sum).  The tests allow ZERO such pairs at every (input,
threshold) they use: `knife_edges` is asserted here for the moderate-size inputs and by the GPU tests for every comparison they make."""
import os
import re

import numpy as np
import torch

from frmap_amd import _lib, matching

import radius_cases as rc
from test_match_topk_cpu import exact_d2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def counted_d2(a, b=None, a_row0=None, labels=None, which="all"):
    """(i int64 [n], j int64 [n], d2 float64 [n]) of the counted pairs, sorted by (i, j).  ``labels``: (labels_a, labels_b), or
    one array in self mode over ``a`` (b=None)."""
    a = np.asarray(a, np.float32)
    if b is None:
        b, a_row0 = a, 0
        if labels is not None and not isinstance(labels, tuple):
            labels = (labels, labels)
    b = np.asarray(b, np.float32)
    P, Q = a.shape[0], b.shape[0]
    if P == 0 or Q == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float64)
    d2 = exact_d2(a, b)
    i = np.arange(P)[:, None]
    j = np.arange(Q)[None, :]
    keep = np.ones((P, Q), bool) if a_row0 is None else (i + a_row0 < j)
    if which != "all":
        same = np.asarray(labels[0]).reshape(-1)[:, None] == np.asarray(labels[1]).reshape(-1)[None, :]
        keep &= same if which == "same" else ~same
    ii, jj = np.nonzero(keep)                                # row-major: sorted by (i, j)
    return ii.astype(np.int64), jj.astype(np.int64), d2[ii, jj]


def knife_edges(d2, thresh):
    """How many pairs a 2^-40 relative change of d2 would move across the threshold."""
    t = np.float32(thresh)
    with np.errstate(invalid="ignore"):
        lo = np.sqrt(d2 * (1.0 - 2.0 ** -40)).astype(np.float32) <= t
        hi = np.sqrt(d2 * (1.0 + 2.0 ** -40)).astype(np.float32) <= t
    return int((lo != hi).sum())


def ref_radius(a, b, thresh, a_row0=None, labels=None, which="all", want_knife=False):
    """(pairs int64 [n, 2] sorted by (i, j), dists fp32 [n]) of the accepted pairs (and the knife-edge count)."""
    i, j, d2 = counted_d2(a, b, a_row0, labels, which)
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(d2).astype(np.float32)
    ok = np.isfinite(dist) & (dist <= np.float32(thresh))
    out = np.stack((i[ok], j[ok]), axis=1), dist[ok]
    return out + (knife_edges(d2, thresh),) if want_knife else out


def test_reference_small_case():
    a = np.zeros((4, 4), np.float32)
    a[1, 0] = 1.0
    a[2, 0] = 3.0
    a[3, 0] = np.nan
    lab = np.array([0, 0, 1, 1])
    e = np.float64(np.float32(1e-6))
    # |(a_i - a_j) + eps|^2 by hand: the first element carries the difference, the other three eps
    d01 = np.float32(np.sqrt(np.float64(np.float32(-1.0) + np.float32(1e-6)) ** 2 + 3 * e * e))
    d12 = np.float32(np.sqrt(np.float64(np.float32(-2.0) + np.float32(1e-6)) ** 2 + 3 * e * e))
    d02 = np.float32(np.sqrt(np.float64(np.float32(-3.0) + np.float32(1e-6)) ** 2 + 3 * e * e))
    assert d01 < 1.0 and d12 < 2.0 and d02 < 3.0             # (x - y) + eps with x < y: just inside
    pairs, dists = ref_radius(a, None, 2.0)
    assert pairs.tolist() == [[0, 1], [1, 2]] and dists.tolist() == [d01, d12] and dists.dtype == np.float32
    pairs, dists = ref_radius(a, None, 3.0)
    assert pairs.tolist() == [[0, 1], [0, 2], [1, 2]] and dists.tolist() == [d01, d02, d12]      # NaN row 3 never listed
    assert ref_radius(a, None, 3.0, labels=lab, which="same")[0].tolist() == [[0, 1]]
    assert ref_radius(a, None, 3.0, labels=lab, which="different")[0].tolist() == [[0, 2], [1, 2]]
    assert ref_radius(a, None, float(np.nextafter(d01, np.float32(0))))[0].shape == (0, 2)       # one fp32 step below the nearest pair
    assert ref_radius(a, None, float(d01))[0].tolist() == [[0, 1]]
    # shards over a_row0 partition the whole (i indexes the shard)
    s0 = ref_radius(a[:2], a, 3.0, a_row0=0)[0]
    s2 = ref_radius(a[2:], a, 3.0, a_row0=2)[0]
    assert s0.tolist() == [[0, 1], [0, 2], [1, 2]] and s2.shape == (0, 2)
    s1 = ref_radius(a[1:3], a, 3.0, a_row0=1)[0]
    assert s1.tolist() == [[0, 2]]                                                              # row 1 of a = row 0 of the shard
    # cross mode: every ordered pair, the diagonal included; (2, 0) is 3 + 1e-6 > 3
    cross = ref_radius(a, a, 3.0)[0]
    assert cross.tolist() == [[0, 0], [0, 1], [0, 2], [1, 0], [1, 1], [1, 2], [2, 1], [2, 2]]
    assert ref_radius(a[:0], a, 3.0)[0].shape == (0, 2) and ref_radius(a, a[:0], 3.0)[0].shape == (0, 2)


def test_no_knife_edges_and_the_accepted_counts_clustered():
    x, _ = rc.clustered(**rc.CLUSTERED_3000)
    i, j, d2 = counted_d2(x)
    assert d2.shape[0] == 3000 * 2999 // 2
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(d2).astype(np.float32)
    for t, accepted in rc.CLUSTERED_3000_ACCEPTED:
        assert knife_edges(d2, t) == 0, t
        assert int((dist <= np.float32(t)).sum()) == accepted, t
    for t in (0.3, 0.6):                                     # (why the tests do not use these: they accept nothing)
        assert int((dist <= np.float32(t)).sum()) == 0


def test_no_knife_edges_and_the_accepted_counts_near_duplicates():
    x = rc.near_duplicates()
    assert x.shape == (1039, 512)
    i, j, d2 = counted_d2(x)
    dist = np.sqrt(d2).astype(np.float32)
    for t, accepted in rc.NEAR_DUPLICATES_ACCEPTED:
        assert knife_edges(d2, t) == 0, t
        assert int((dist <= np.float32(t)).sum()) == accepted, t
    t21 = np.sort(dist)[20]
    assert abs(float(t21) - np.sqrt(512.0) * 1e-6) < 1e-10   # the distance of bit-identical rows
    below = np.nextafter(t21, np.float32(0))
    assert knife_edges(d2, t21) == 0 and knife_edges(d2, below) == 0
    assert int((dist <= t21).sum()) == 22 and int((dist <= below).sum()) == 0


def test_union_find_equals_scipy_components():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    x, _ = rc.clustered(77, 400, 64, 50)
    for t in (0.45, 0.55, 1.2):
        pairs, _ = ref_radius(x, None, t)
        got = matching.components_of_pairs(400, pairs)
        assert got.dtype == np.int64 and got.shape == (400,)
        g = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(400, 400))
        ncomp, lab = connected_components(g, directed=False)
        assert got.max() + 1 == ncomp
        # same partition ...
        assert len(set(zip(got.tolist(), lab.tolist()))) == ncomp
        # ... numbered by each component's lowest row: first appearances are 0, 1, 2, ...
        _, first = np.unique(got, return_index=True)
        assert (np.diff(first) > 0).all() and got[0] == 0
        assert (got[first] == np.arange(ncomp)).all()
    assert matching.components_of_pairs(3, np.zeros((0, 2), np.int64)).tolist() == [0, 1, 2]
    assert matching.components_of_pairs(0, np.zeros((0, 2), np.int64)).shape == (0,)
    assert matching.components_of_pairs(5, [[3, 4], [1, 3], [0, 2]]).tolist() == [0, 1, 0, 1, 1]
    # shuffled edge order and reversed edges: the same answer
    pairs, _ = ref_radius(x, None, 0.55)
    perm = np.random.default_rng(1).permutation(len(pairs))
    assert (matching.components_of_pairs(400, pairs[perm][:, ::-1]) == matching.components_of_pairs(400, pairs)).all()


def test_csr_segments_are_ordered_by_distance_then_row():
    rng = np.random.default_rng(5)
    B, n = 9, 200
    i = rng.integers(0, B - 2, n)                            # probes B - 2 and B - 1 stay empty
    j = rng.permutation(1000)[:n]
    d = rng.choice(np.float32([0.0, 2.2e-5, 0.1, 0.1000001, 0.5, 3e19]), n).astype(np.float32)     # many ties on the distance
    counts = np.bincount(i, minlength=B).astype(np.int32)
    perm = rng.permutation(n)
    off, rows, dists = matching.csr_by_dist(torch.from_numpy(np.stack((i, j), 1)[perm].astype(np.int32)),
                                            torch.from_numpy(d[perm]), torch.from_numpy(counts))
    assert off.dtype == torch.int64 and off.tolist() == [0] + np.cumsum(counts).tolist()
    for p in range(B):
        sel = np.nonzero(i == p)[0]
        order = sel[np.lexsort((j[sel], d[sel]))]
        assert rows[off[p]:off[p + 1]].tolist() == j[order].tolist(), p
        assert dists[off[p]:off[p + 1]].tolist() == d[order].tolist(), p
    off, rows, dists = matching.csr_by_dist(torch.zeros((0, 2), dtype=torch.int32), torch.zeros(0), torch.zeros(3, dtype=torch.int32))
    assert off.tolist() == [0, 0, 0, 0] and rows.shape == (0,) and dists.shape == (0,)


def test_compare_faces_all_sentinels_never_raise():
    assert matching.compare_faces_all(None, [{"name": "a", "embedding": torch.zeros(1, 4)}], 1.0) == []
    assert matching.compare_faces_all(torch.zeros(1, 4), [], 1.0) == []
    assert matching.compare_faces_all(torch.zeros(1, 4), None, 1.0) == []


def test_radius_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_match_radius_workspace_bytes", 3), ("frmap_match_radius", 18), ("frmap_match_radius_packed", 20)):
        m = re.search(r"\b" + sym + r"\s*\(([^;]*)\);", header)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
    assert _lib.ABI_VERSION == 10
    from frmap_amd import ops
    import inspect
    sig = inspect.signature(ops.match_radius)
    assert list(sig.parameters)[:3] == ["a", "thresh", "b"]
    for kw in ("labels_a", "labels_b", "which", "a_row0", "prepared", "capacity", "return_rescored"):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY, kw
