"""GPU: exact threshold search (`ops.match_radius`, both paths: the exact scan and the split-fp16 GEMM with its exact re-score)
equals the numpy reference `ref_radius` of `test_match_radius_cpu.py` exactly: pairs as sets, distances bit for bit, counts and
totals, no tolerance; and the matching functions built on it (`search_radius`, `compare_faces_all`, `duplicate_pairs`,
`cluster_embeddings`).  Every comparison against the reference first asserts that its (input, threshold) has no knife-edge pair
(`knife_edges`), so a difference can never be blamed on the float64 summation order."""
import json
import os

import numpy as np
import pytest
import torch

from frmap_amd import _lib, matching, ops, synth

import match_cases as mc
import radius_cases as rc
from test_match_radius_cpu import ref_radius

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(x, dtype=None):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x if dtype is None else np.asarray(x, dtype))).to(DEV)


def _run(a, thresh, b=None, la=None, lb=None, which="all", a_row0=None, packed=False, **kw):
    """`ops.match_radius` on host arrays -> host arrays (pairs int64 [n, 2], dists fp32 [n], counts int64 [P], ...)."""
    ad, bd = _t(a), _t(b)
    prep = ops.match_prepare(ad if bd is None else bd) if packed else None
    out = ops.match_radius(ad, thresh, bd, labels_a=_t(la, np.int32), labels_b=_t(lb, np.int32), which=which, a_row0=a_row0,
                           prepared=prep, **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy().astype(np.int64) if o.dtype != torch.float32 else o.cpu().numpy() for o in out)


def _same(got, want, P, what=""):
    """got = (pairs, dists, counts) sorted by (i, j) equals the reference (pairs, dists): sets, bits, counts."""
    gp, gd, gc = got[:3]
    wp, wd = want
    assert gp.shape == wp.shape, (what, gp.shape, wp.shape)
    assert len(set(map(tuple, gp.tolist()))) == len(gp), what                      # every pair once
    assert (gp == wp).all(), what                                                    # (both sorted by (i, j): equal as sets)
    assert gd.dtype == np.float32 and (gd.view(np.int32) == wd.view(np.int32)).all(), what
    assert (gc == np.bincount(wp[:, 0], minlength=P)).all() and gc.sum() == len(wp), what


def _check(a, thresh, b=None, la=None, lb=None, which="all", a_row0=None, paths=(False, True), monkeypatch=None, what=""):
    labels = None if la is None else (la, la if b is None else lb)
    wp, wd, knife = ref_radius(a, b, thresh, a_row0, labels, which, want_knife=True)
    assert knife == 0, (what, thresh, knife)
    resc = {}
    for pk in paths:
        if pk:
            monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
        got = _run(a, thresh, b, la, lb, which, a_row0, packed=pk, return_rescored=True)
        if pk:
            monkeypatch.undo()
        _same(got, (wp, wd), a.shape[0], (what, pk))
        resc[pk] = int(got[3][0])
    assert resc.get(False, 0) == 0                                                   # the scan re-scores nothing: it scores everything
    return wp, wd, resc


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 500, 3000])
def test_scan_self_sizes(n):
    x, _ = rc.clustered(n, n, 128, max(1, n // 6))
    wp, _, _ = _check(x, 0.5, paths=(False,), what=n)
    assert n < 63 or 0 < len(wp) < n * (n - 1) // 2


@pytest.mark.parametrize("D", [32, 128, 512, 1000])
def test_scan_cross_dims(D):
    a, _ = rc.clustered(D, 70, D, 9)
    b, _ = rc.clustered(D, 130, D, 9, noise=0.3)     # (same seed: the same centres, other rows)
    b[:9] = a[:9]
    wp, _, _ = _check(a, 0.5, b, paths=(False,), what=D)
    assert 9 <= len(wp) < 70 * 130


@pytest.mark.parametrize("D", [32, 128, 512])
@pytest.mark.parametrize("mode", ["self", "cross"])
def test_packed_equals_reference(monkeypatch, D, mode):
    x, lab = rc.clustered(7 + D, 600, D, 40)
    if mode == "self":
        wp, _, resc = _check(x, 0.5, monkeypatch=monkeypatch, what=(D, mode))
        pairs = 600 * 599 // 2
    else:
        b, _ = rc.clustered(7 + D, 300, D, 40, noise=0.3)       # (same seed: the same centres, other rows)
        wp, _, resc = _check(x, 0.5, b, monkeypatch=monkeypatch, what=(D, mode))
        pairs = 600 * 300
    assert 0 < len(wp) < pairs
    assert len(wp) <= resc[True] < pairs             # every accepted pair is re-scored; the certain rejects are not


def test_near_duplicates_at_the_listed_thresholds(monkeypatch):
    x = rc.near_duplicates()
    for t, accepted in rc.NEAR_DUPLICATES_ACCEPTED:
        wp, _, _ = _check(x, t, monkeypatch=monkeypatch, what=t)
        assert len(wp) == accepted
    _, wd = ref_radius(x, None, 1e-4)
    t21 = np.sort(wd)[20]                            # the distance of bit-identical rows: 22 pairs sit exactly on it
    wp, wd, _ = _check(x, float(t21), monkeypatch=monkeypatch, what="t21")
    assert len(wp) == 22 and (wd == t21).all()
    wp, _, _ = _check(x, float(np.nextafter(t21, np.float32(0))), monkeypatch=monkeypatch, what="below t21")
    assert len(wp) == 0


def test_nan_inf_and_huge_rows(monkeypatch):
    x, lab = rc.clustered(5, 520, 64, 30)
    x[3] = np.nan
    x[100, 7] = np.inf
    x[200] *= 3e19          # fp32 norm^2 overflows, the float64 d2 of two such rows does not
    x[201] = x[200] * 1.0000001
    for t in (0.5, 1e3, 1e13, 3e19, float(np.finfo(np.float32).max)):
        wp, wd, _ = _check(x, t, monkeypatch=monkeypatch, what=t)
        assert not np.isin(wp, [3, 100]).any() and np.isfinite(wd).all()
        if t >= 1e13:
            assert [200, 201] in wp.tolist()
    # cross mode, the bad rows on either side
    _check(x[:150], 0.5, x, monkeypatch=monkeypatch, what="cross A")
    _check(x[150:260], 3e19, x[:120], monkeypatch=monkeypatch, what="cross B")


def test_edge_cases(monkeypatch):
    x, lab = rc.clustered(8, 300, 64, 20)
    wp, _, _ = _check(x, 0.0, monkeypatch=monkeypatch, what="t = 0")
    assert len(wp) == 0                                                  # even a row against itself is sqrt(D) * 1e-6 away
    wp, _, _ = _check(x, 0.0, x, monkeypatch=monkeypatch, what="t = 0, cross")
    assert len(wp) == 0
    e = np.zeros((0, 64), np.float32)
    for got, P in ((_run(e, 0.5), 0), (_run(e, 0.5, x), 0), (_run(x, 0.5, e), 300), (_run(x[:0], 0.5, x, a_row0=300), 0)):
        assert got[0].shape == (0, 2) and got[1].shape == (0,) and got[2].shape == (P,) and (got[2] == 0).all()
    monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
    got = _run(x[:0], 0.5, x, a_row0=300, packed=True)
    assert got[0].shape == (0, 2) and got[2].shape == (0,)
    got = _run(e, 0.5, x, packed=True, capacity=4)
    assert got[3].tolist() == [0]


def test_shards_partition_the_whole(monkeypatch):
    x, _ = rc.clustered(21, 900, 128, 50)
    wp, wd, _ = _check(x, 0.5, monkeypatch=monkeypatch, what="whole")
    whole = {tuple(p): d for p, d in zip(wp.tolist(), wd.view(np.int32).tolist())}
    assert len(whole) > 0
    for packed in (False, True):
        monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
        seen = {}
        for r0 in (0, 300, 600):
            gp, gd, gc = _run(x[r0:r0 + 300], 0.5, x, a_row0=r0, packed=packed)
            assert ((gp[:, 0] >= 0) & (gp[:, 0] < 300)).all() and (gc == np.bincount(gp[:, 0], minlength=300)).all()
            for (i, j), d in zip(gp.tolist(), gd.view(np.int32).tolist()):
                assert (i + r0, j) not in seen, (packed, r0, i, j)            # disjoint
                seen[(i + r0, j)] = d
        monkeypatch.undo()
        assert seen == whole, packed


def test_filters_and_agreement_with_verify_counts(monkeypatch):
    x, lab = rc.clustered(13, 700, 128, 40)
    b, lb = rc.clustered(13, 400, 128, 40, noise=0.4)
    lab, lb = lab.copy(), lb.copy()
    lab[::3] = (lab[::3] + 1) % 40                   # mislabel a third of the rows: near pairs of different labels exist too
    lb[::3] = (lb[::3] + 1) % 40
    for t in (0.5, 0.62):
        for args in ((x, t, None, lab, None), (x, t, b, lab, lb)):
            a_, t_, b_, la_, lb_ = args
            sets = {}
            for which in ("all", "same", "different"):
                wp, _, _ = _check(a_, t_, b_, la_, lb_, which=which, monkeypatch=monkeypatch, what=(t, which))
                sets[which] = set(map(tuple, wp.tolist()))
            assert sets["same"] | sets["different"] == sets["all"] and not (sets["same"] & sets["different"])
            assert sets["same"] and sets["different"]
            for packed in (False, True):
                monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
                ad, bd = _t(a_), _t(b_)
                prep = ops.match_prepare(ad if bd is None else bd) if packed else None
                vc = ops.verify_counts(ad, _t(la_), [t_], bd, _t(lb_), prepared=prep).cpu().numpy()
                same = _run(a_, t_, b_, la_, lb_, which="same", packed=packed)
                diff = _run(a_, t_, b_, la_, lb_, which="different", packed=packed)
                monkeypatch.undo()
                assert len(same[0]) == vc[0, 0] and len(diff[0]) == vc[1, 0], (t, packed)
    # which="all" needs no labels; "same" / "different" do
    with pytest.raises(ValueError):
        ops.match_radius(_t(x), 0.5, which="same")


def test_capacity(monkeypatch):
    x, _ = rc.clustered(17, 800, 128, 40)
    wp, wd, knife = ref_radius(x, None, 0.5, want_knife=True)
    assert knife == 0 and len(wp) > 100
    want = {tuple(p): d for p, d in zip(wp.tolist(), wd.view(np.int32).tolist())}
    counts = np.bincount(wp[:, 0], minlength=800)
    for packed in (False, True):
        monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
        cap = len(wp) // 2
        gp, gd, gc, total = _run(x, 0.5, packed=packed, capacity=cap)
        assert total.tolist() == [len(wp)] and (gc == counts).all()                  # exact whatever the capacity
        assert gp.shape == (cap, 2) and gd.shape == (cap,)
        got = list(map(tuple, gp.tolist()))
        assert len(set(got)) == cap                                                  # distinct ...
        assert all(want.get(p) == d for p, d in zip(got, gd.view(np.int32).tolist()))   # ... members of the reference, with their distance
        gp, gd, gc, total = _run(x, 0.5, packed=packed, capacity=0)                  # count only
        assert gp.shape == (0, 2) and total.tolist() == [len(wp)] and (gc == counts).all()
        gp, gd, gc, total = _run(x, 0.5, packed=packed, capacity=len(wp) + 7)        # room to spare: slots past the total are not written
        assert total.tolist() == [len(wp)]
        assert {tuple(p): d for p, d in zip(gp[:len(wp)].tolist(), gd[:len(wp)].view(np.int32).tolist())} == want
        monkeypatch.undo()
    # straight at the C entry point: capacity 0 with null lists
    lib = _lib.load()
    xd = _t(x)
    cnt = torch.empty(800, dtype=torch.int32, device=DEV)
    tot = torch.empty(1, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.frmap_match_radius_workspace_bytes(800, 800, 128), dtype=torch.uint8, device=DEV)
    assert lib.frmap_match_radius(xd.data_ptr(), 0, 800, xd.data_ptr(), 0, 800, 128, 0, 0.5, 0, cnt.data_ptr(), tot.data_ptr(), 0, 0, 0, 0,
                                  ws.data_ptr(), 0) == 0
    torch.cuda.synchronize()
    assert tot.item() == len(wp) and (cnt.cpu().numpy() == counts).all()


def test_search_radius_agrees_with_search_batch(monkeypatch):
    monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
    x, lab = rc.clustered(51, 600, 512, 30)
    g = matching.Gallery([f"id{v}" for v in lab], torch.from_numpy(x), DEV)
    probes = g.matrix[:40] + 0.01 * synth.unit_rows(52, 40, 512, "rad_probe").to(DEV)
    for t in (0.4, 0.5):
        off, rows, dists = matching.search_radius(probes, g, t)
        idx, dist, _ = matching.search_batch(probes, g, 16)
        off, rows, dists, idx, dist = off.cpu(), rows.cpu(), dists.cpu(), idx.cpu(), dist.cpu()
        assert off.dtype == torch.int64 and off.shape == (41,) and off[0] == 0 and off[-1] == rows.shape[0] == dists.shape[0]
        compared = 0
        for p in range(40):
            seg = slice(int(off[p]), int(off[p + 1]))
            n = seg.stop - seg.start
            if n <= 16:
                keep = dist[p] <= np.float32(t)
                assert rows[seg].tolist() == idx[p][keep].tolist(), (t, p)
                assert torch.equal(dists[seg], dist[p][keep]), (t, p)
                compared += n > 0
            else:
                assert rows[seg][:16].tolist() == idx[p].tolist() and torch.equal(dists[seg][:16], dist[p])
        assert compared >= 5, (t, compared)
    # a single D-vector, a refs list, an empty gallery
    off, rows, dists = matching.search_radius(probes[0], g, 0.5)
    assert off.shape == (2,)
    off, rows, dists = matching.search_radius(probes[:3], [], 0.5)
    assert off.tolist() == [0, 0, 0, 0] and rows.shape == (0,)


def test_compare_faces_all_on_the_reference_gallery():
    z = json.load(open(os.path.join(ROOT, "tests", "golden", "face_references.json")))
    names, emb = z["names"], torch.tensor(z["embeddings"], dtype=torch.float32).reshape(len(z["names"]), -1)
    assert len(names) == 7
    refs = [{"name": n, "embedding": emb[i:i + 1].to(DEV)} for i, n in enumerate(names)]
    named = unknown = 0
    for i in range(len(names)):
        probe = (emb[i] + 0.01 * synth.unit_rows(990 + i, 1, emb.shape[1], "tk_ref")[0]).to(DEV)
        for thresh in (1.0, 0.05, 0.005, float("inf")):
            first = matching.compare_faces(probe, refs, thresh)
            lst = matching.compare_faces_all(probe, refs, thresh)
            print("compare_faces_all", i, thresh, first, lst[:1])
            if first[2] is None:
                assert lst == []
                unknown += 1
            else:
                assert lst[0] == first
                assert [(x[1], x[2]) for x in lst] == sorted((x[1], x[2]) for x in lst) and all(x[1] <= thresh for x in lst)
                assert all(x[0] == names[x[2]] for x in lst)
                named += 1
        assert len(matching.compare_faces_all(probe, refs, float("inf"))) == 7
    assert named and unknown
    assert matching.compare_faces_all(None, refs, 1.0) == [] and matching.compare_faces_all(probe, [], 1.0) == []
    assert matching.compare_faces_all(probe, refs, float("nan")) == [] and matching.compare_faces_all(probe, refs, -1.0) == []


def test_cluster_embeddings_equals_union_find_over_the_reference(monkeypatch):
    x, _ = rc.clustered(61, 700, 128, 60)
    for t in (0.45, 0.55):
        wp, _, knife = ref_radius(x, None, t, want_knife=True)
        assert knife == 0
        want = matching.components_of_pairs(700, wp)
        got = matching.cluster_embeddings(torch.from_numpy(x).to(DEV), t)
        assert got.dtype == torch.int64 and (got.numpy() == want).all()
        assert 1 < want.max() + 1 < 700


def test_duplicate_pairs_finds_the_planted_groups():
    probes, gal, notes = mc.build_case(1000, 512, "unit", 99)
    g = matching.Gallery([f"id{i % 97}" for i in range(1000)], gal, DEV)
    assert g.prepared is not None                                       # 1000 rows: the gallery's own pack, the GEMM path
    gn = gal.numpy()
    # the planted structure, from the case's own construction: each group's four members, and the bit-identical rows
    members = {}
    for kind, gi, m in notes:
        if kind == "equal":
            members.setdefault(gi, []).append(m)
    _, inv, cnt = np.unique(gn, axis=0, return_inverse=True, return_counts=True)
    ident = np.nonzero(cnt[inv.reshape(-1)] > 1)[0].tolist()
    assert len(ident) == 3 and len(members) == len(mc.SEPARATIONS) and all(len(m) == 4 for m in members.values())
    among = lambda rows: {(u, v) for u in rows for v in rows if u < v}

    def check(t, want):
        wp, wd, knife = ref_radius(gn, None, t, want_knife=True)
        assert knife == 0, t
        pairs, dists = matching.duplicate_pairs(g, t)
        assert pairs.dtype == torch.int32 and pairs.cpu().tolist() == wp.tolist() and (pairs[:, 0] < pairs[:, 1]).all(), t
        assert (dists.cpu().numpy().view(np.int32) == wd.view(np.int32)).all(), t
        assert set(map(tuple, wp.tolist())) == want, t

    # bit-identical rows: exactly the pairs at the smallest distance there is, sqrt(512) * 1e-6
    _, wd = ref_radius(gn, None, 1e-4)
    t0 = float(wd.min())
    assert abs(t0 - np.sqrt(512.0) * 1e-6) < 1e-10
    check(t0, among(ident))
    # at four times a group's separation (two copies lie up to two separations apart, and F.pairwise_distance's eps adds
    # sqrt(512) * 1e-6 in quadrature): that group and the tighter ones, whole; the next group (ten times as wide) not at all
    for k in range(1, len(mc.SEPARATIONS)):
        want = among(ident)
        for gi in range(k + 1):
            want |= among(members[gi])
        check(4 * mc.SEPARATIONS[k], want)
    # which: identities are the names
    same, _ = matching.duplicate_pairs(g, 2e-3, which="same")
    diff, _ = matching.duplicate_pairs(g, 2e-3, which="different")
    both, _ = matching.duplicate_pairs(g, 2e-3)
    lab = g.labels.cpu().numpy()
    assert all(lab[i] == lab[j] for i, j in same.cpu().tolist()) and all(lab[i] != lab[j] for i, j in diff.cpu().tolist())
    assert sorted(same.cpu().tolist() + diff.cpu().tolist()) == both.cpu().tolist() and len(both) == 27
    # a plain tensor with labels
    p2, _ = matching.duplicate_pairs(g.matrix, 2e-3, which="different", labels=g.labels)
    assert torch.equal(p2, diff)
    with pytest.raises(ValueError):
        matching.duplicate_pairs(g, 2e-3, labels=g.labels)


def test_graph_capture_replays_on_new_inputs(monkeypatch):
    monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
    gal, _ = rc.clustered(41, 700, 128, 40)
    probes = [rc.clustered(41, 300, 128, 40, noise=n)[0] for n in (0.3, 0.25, 0.2)]      # (same centres as the gallery)
    gd = _t(gal)
    prep = ops.match_prepare(gd)
    buf = _t(probes[0]).clone()
    cap = 16384
    for packed in (True, False):
        kw = dict(prepared=prep) if packed else {}
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                ops.match_radius(buf, 0.5, gd, capacity=cap, return_rescored=True, **kw)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            pairs, dists, counts, total, resc = ops.match_radius(buf, 0.5, gd, capacity=cap, return_rescored=True, **kw)
        for x in (probes[1], probes[2], probes[0]):
            buf.copy_(_t(x))
            g.replay()
            torch.cuda.synchronize()
            wp, wd, knife = ref_radius(x, gal, 0.5, want_knife=True)
            n = int(total.item())
            assert knife == 0 and 0 < n == len(wp) <= cap
            assert (resc.item() >= n) == packed and (packed or resc.item() == 0)
            gp, gdist = pairs[:n].cpu().numpy().astype(np.int64), dists[:n].cpu().numpy()
            order = np.lexsort((gp[:, 1], gp[:, 0]))
            _same((gp[order], gdist[order], counts.cpu().numpy().astype(np.int64)), (wp, wd), 300, ("replay", packed))


def test_bad_arguments_raise_and_launch_nothing():
    x, lab = rc.clustered(2, 50, 32, 5)
    ad, ld = _t(x), _t(lab)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), 1e39):
        with pytest.raises(ValueError):
            ops.match_radius(ad, bad)
    with pytest.raises(ValueError):
        ops.match_radius(ad, 0.5, ad[:, :16].contiguous())                      # mismatched D
    with pytest.raises(ValueError):
        ops.match_radius(ad, 0.5, labels_a=ld[:10], which="same")               # label lengths
    with pytest.raises(ValueError):
        ops.match_radius(ad, 0.5, ad, labels_a=ld, labels_b=ld[:49], which="different")
    with pytest.raises(ValueError):
        ops.match_radius(ad, 0.5, ad, a_row0=1)                                 # a_row0 + P > Q
    with pytest.raises(ValueError):
        ops.match_radius(ad, 0.5, ad, a_row0=-2)
    with pytest.raises(ValueError):
        ops.match_radius(ad, 0.5, which="other")
    with pytest.raises(ValueError):
        ops.match_radius(ad, 0.5, capacity=-1)
    # the C entry points reject the same before any launch: the outputs keep their sentinel
    lib = _lib.load()
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    cnt = torch.full((50,), -7, dtype=torch.int32, device=DEV)
    tot = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    pr = torch.full((8, 2), -7, dtype=torch.int32, device=DEV)
    ds = torch.full((8,), -7.0, device=DEV)

    def call(P=50, Q=50, D=32, row0=-1, t=0.5, filt=0, la=0, lb=0, cap=8, pairs=None):
        return lib.frmap_match_radius(ad.data_ptr(), la, P, ad.data_ptr(), lb, Q, D, row0, t, filt, cnt.data_ptr(), tot.data_ptr(),
                                      pr.data_ptr() if pairs is None else pairs, ds.data_ptr(), cap, 0, ws.data_ptr(), 0)

    for kw in (dict(t=-1.0), dict(t=float("nan")), dict(t=float("inf")), dict(filt=3), dict(filt=1), dict(filt=2, la=ld.data_ptr()),
               dict(row0=1), dict(row0=-2), dict(Q=40, row0=0), dict(D=30), dict(cap=-1), dict(pairs=0)):
        assert call(**kw) == -1, kw
    assert b"a_row0" in (call(row0=1), lib.frmap_last_error())[1]
    torch.cuda.synchronize()
    assert (cnt == -7).all() and (tot == -7).all() and (pr == -7).all() and (ds == -7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert tot.item() == len(ref_radius(x, x, 0.5)[0]) and (cnt >= 0).all()


def test_large_packed_equals_scan():
    x, _ = rc.clustered(31, 16384, 512, 2048, noise=0.5)
    t = 0.7            # on the 3000-row set of the same recipe (375 identities, 8 rows each) 0.7 accepts 4 611 of 4 498 500 pairs = 0.1 %
    scan = _run(x, t)
    packed = _run(x, t, packed=True, return_rescored=True)
    n, pairs = len(scan[0]), 16384 * 16383 // 2
    print("large: accepted", n, "of", pairs, "re-scored", int(packed[3][0]))
    assert 0 < n < pairs // 100
    assert (scan[0] == packed[0]).all() and (scan[1].view(np.int32) == packed[1].view(np.int32)).all() and (scan[2] == packed[2]).all()
    assert len(set(map(tuple, scan[0].tolist()))) == n and scan[2].sum() == n
    assert n <= int(packed[3][0]) < pairs
