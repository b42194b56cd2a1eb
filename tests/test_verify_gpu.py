"""GPU: exact verification counts (`ops.verify_counts`, both paths) equal the numpy reference `ref_verify_counts` exactly, with
no tolerance; the MFMA path really bins and re-scores; shards, graph capture, bad arguments, agreement with `search_batch`, and the
metrics / `threshold_for_far` end to end."""
import numpy as np
import pytest
import torch

from frmap_amd import evaluate, matching, ops, synth

import match_cases as mc
from test_match_topk_cpu import exact_d2
from test_verify_cpu import pair_dists, ref_verify_counts

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _clustered(seed, n, d, ids, noise=0.35):
    rng = np.random.default_rng(seed)
    centres = synth.unit_rows(seed, ids, d, "verify").numpy()
    lab = rng.integers(0, ids, n).astype(np.int32)
    x = centres[lab] + noise / np.sqrt(d) * rng.standard_normal((n, d)).astype(np.float32)
    return x.astype(np.float32), lab


def _grid(x, T=64, b=None):
    return evaluate.default_thresholds(torch.from_numpy(x if b is None else np.concatenate((x, b))), n=T)


def _run(a, la, t, b=None, lb=None, a_row0=None, packed=False, rescored=False):
    ad = torch.from_numpy(a).to(DEV)
    bd = torch.from_numpy(b).to(DEV) if b is not None else None
    la_d = torch.from_numpy(np.asarray(la, np.int32)).to(DEV)
    lb_d = torch.from_numpy(np.asarray(lb, np.int32)).to(DEV) if lb is not None else None
    prep = None
    if packed:
        prep = ops.match_prepare(ad if bd is None else bd)
    out = ops.verify_counts(ad, la_d, t, bd, lb_d, a_row0=a_row0, prepared=prep, return_rescored=rescored)
    torch.cuda.synchronize()
    if rescored:
        return out[0].cpu().numpy(), int(out[1].item())
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 500, 3000])
def test_scan_self_sizes(n):
    x, lab = _clustered(n, n, 128, max(1, n // 6))
    t = _grid(x)
    assert (_run(x, lab, t) == ref_verify_counts(x, lab, t)).all()


@pytest.mark.parametrize("D", [32, 128, 512, 1000])
def test_scan_cross_dims(D):
    a, la = _clustered(D, 70, D, 9)
    b, lb = _clustered(D + 1, 130, D, 9)
    t = _grid(a, 33, b)
    assert (_run(a, la, t, b, lb) == ref_verify_counts(a, la, t, b, lb)).all()


@pytest.mark.parametrize("D", [32, 128, 512])
@pytest.mark.parametrize("mode", ["self", "cross"])
def test_packed_equals_reference(monkeypatch, D, mode):
    monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
    x, lab = _clustered(7 + D, 600, D, 40)
    if mode == "self":
        t = _grid(x, 256)
        got, resc = _run(x, lab, t, packed=True, rescored=True)
        want = ref_verify_counts(x, lab, t)
    else:
        b, lb = _clustered(9 + D, 300, D, 40)
        t = _grid(x, 256, b)
        got, resc = _run(x, lab, t, b, lb, packed=True, rescored=True)
        want = ref_verify_counts(x, lab, t, b, lb)
    assert (got == want).all()
    assert resc > 0            # a fine grid always straddles some bands: the re-score ran


def test_near_duplicates_and_thresholds_on_a_distance(monkeypatch):
    monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
    probes, gal, _ = mc.build_case(700, 512, "unit", 99)
    x = torch.cat((gal, probes)).numpy()
    lab = (np.arange(x.shape[0]) % 37).astype(np.int32)
    dist, _ = pair_dists(x, lab)
    d = np.sort(dist[np.isfinite(dist)])
    picks = d[:: max(1, len(d) // 150)][:150]
    t = np.unique(np.concatenate([picks, np.nextafter(picks, np.float32(0)), np.nextafter(picks, np.float32(np.inf)),
                                  d[:40]]).astype(np.float32))
    t = t[t >= 0][: ops.VERIFY_MAX_THRESHOLDS]
    want = ref_verify_counts(x, lab, t)
    assert (_run(x, lab, t) == want).all()
    got, resc = _run(x, lab, t, packed=True, rescored=True)
    assert (got == want).all() and resc > 0


def test_nan_inf_and_huge_rows(monkeypatch):
    monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
    x, lab = _clustered(5, 520, 64, 30)
    x[3] = np.nan
    x[100, 7] = np.inf
    x[200] *= 3e19          # fp32 norm^2 overflows, the float64 d2 of two such rows does not
    x[201] = x[200] * 1.0000001
    lab[201] = lab[200]
    t = np.concatenate([_grid(x[:150], 100), np.float32([1e3, 1e10, 3e19])]).astype(np.float32)
    t = np.unique(t)
    want = ref_verify_counts(x, lab, t)
    assert (_run(x, lab, t) == want).all()
    assert (_run(x, lab, t, packed=True) == want).all()


def test_t1_tmax_and_empty(monkeypatch):
    x, lab = _clustered(8, 300, 64, 20)
    t1 = np.float32([1.0])
    assert (_run(x, lab, t1) == ref_verify_counts(x, lab, t1)).all()
    tm = np.linspace(0, 2.5, ops.VERIFY_MAX_THRESHOLDS).astype(np.float32)
    want = ref_verify_counts(x, lab, tm)
    assert (_run(x, lab, tm) == want).all()
    monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
    assert (_run(x, lab, tm, packed=True) == want).all()
    e = np.zeros((0, 64), np.float32)
    assert (_run(e, np.zeros(0, np.int32), tm[:5]) == 0).all()
    assert (_run(e, np.zeros(0, np.int32), tm[:5], x, lab) == 0).all()
    assert (_run(x, lab, tm[:5], e, np.zeros(0, np.int32)) == 0).all()
    assert (_run(x[:0], lab[:0], tm[:5], x, lab, a_row0=300) == 0).all()


def test_shards_sum_to_the_whole(monkeypatch):
    x, lab = _clustered(21, 900, 128, 50)
    t = _grid(x, 128)
    whole = _run(x, lab, t)
    assert (whole == ref_verify_counts(x, lab, t)).all()
    for packed in (False, True):
        monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
        parts = sum(_run(x[r0:r0 + 300], lab[r0:r0 + 300], t, x, lab, a_row0=r0, packed=packed) for r0 in (0, 300, 600))
        assert (parts == whole).all(), packed


def test_large_packed_equals_scan():
    x, lab = _clustered(31, 16384, 512, 2048, noise=0.5)
    t = _grid(x, 256)
    scan = _run(x, lab, t)
    packed, resc = _run(x, lab, t, packed=True, rescored=True)
    assert (packed == scan).all()
    assert scan[:, -1].sum() == 16384 * 16383 // 2 and 0 < resc < 16384 * 16383 // 2


def test_graph_capture_replays(monkeypatch):
    monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
    x, lab = _clustered(41, 700, 128, 40)
    ad, ld = torch.from_numpy(x).to(DEV), torch.from_numpy(lab).to(DEV)
    t = torch.from_numpy(_grid(x, 64)).to(DEV)
    prep = ops.match_prepare(ad)
    want = ref_verify_counts(x, lab, t.cpu().numpy())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ops.verify_counts(ad, ld, t, prepared=prep)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.verify_counts(ad, ld, t, prepared=prep)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == want).all()


def test_bad_arguments_raise():
    x, lab = _clustered(2, 50, 32, 5)
    ad, ld = torch.from_numpy(x).to(DEV), torch.from_numpy(lab).to(DEV)
    for bad in ([0.5, 0.4], [float("nan")], [float("inf")], [-0.1], [], np.zeros(ops.VERIFY_MAX_THRESHOLDS + 1)):
        with pytest.raises(ValueError):
            ops.verify_counts(ad, ld, bad)
    with pytest.raises(ValueError):
        ops.verify_counts(ad, ld, [1.0], ad, ld, a_row0=1)          # a_row0 + P > Q
    with pytest.raises(ValueError):
        ops.verify_counts(ad, ld[:10], [1.0])
    with pytest.raises(ValueError):
        ops.verify_counts(ad, ld, [1.0], ad[:, :16].contiguous(), ld)
    from frmap_amd import _lib
    lib = _lib.load()
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    out = torch.empty(4, dtype=torch.int64, device=DEV)
    t = torch.ones(2, device=DEV)
    assert lib.frmap_verify_counts(ad.data_ptr(), ld.data_ptr(), 50, ad.data_ptr(), ld.data_ptr(), 50, 32, -1, t.data_ptr(), 0,
                                   out.data_ptr(), 0, ws.data_ptr(), 0) == -1
    assert lib.frmap_verify_counts(ad.data_ptr(), ld.data_ptr(), 50, ad.data_ptr(), ld.data_ptr(), 40, 32, 0, t.data_ptr(), 2,
                                   out.data_ptr(), 0, ws.data_ptr(), 0) == -1
    assert b"a_row0" in lib.frmap_last_error()
    # thresholds that break the contract on the device (not checked by a host copy): every output all-ones
    tb = torch.tensor([1.0, 0.5], device=DEV)
    assert lib.frmap_verify_counts(ad.data_ptr(), ld.data_ptr(), 50, ad.data_ptr(), ld.data_ptr(), 50, 32, -1, tb.data_ptr(), 2,
                                   out.data_ptr(), 0, ws.data_ptr(), 0) == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [-1, -1, -1, -1]


def test_agrees_with_search_batch(monkeypatch):
    monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
    x, lab = _clustered(51, 600, 512, 30)
    g = matching.Gallery([f"id{v}" for v in lab], torch.from_numpy(x), DEV)
    _, dist, _ = matching.search_batch(g.matrix[:3], g, 5)
    ad = g.matrix
    for p in range(3):
        for k in range(1, 5):
            d = dist[p, k].item()
            j = None
            for t, expect_self in ((np.float32(d), True), (np.nextafter(np.float32(d), np.float32(0)), False)):
                single = ops.verify_counts(ad[p:p + 1], g.labels[p:p + 1], [float(t)], ad, g.labels, prepared=g.prepared)
                scan = ops.verify_counts(ad[p:p + 1], g.labels[p:p + 1], [float(t)], ad, g.labels)
                c = single.cpu().numpy()
                assert (c == scan.cpu().numpy()).all()
                want = ref_verify_counts(x[p:p + 1], lab[p:p + 1], [t], x, lab)
                assert (c == want).all()
                if j is None:
                    j = int(c.sum())
                else:
                    assert int(c.sum()) < j          # the pair at distance d is accepted at d, rejected just below


def test_metrics_and_threshold_for_far_end_to_end():
    x, lab = _clustered(61, 800, 128, 60)
    m = evaluate.verification_metrics(torch.from_numpy(x).to(DEV), lab)
    t = m["thresholds"].astype(np.float32)
    G, I = evaluate.pair_totals(lab)
    want = evaluate.metrics_from_counts(t, ref_verify_counts(x, lab, t), G, I)
    for key in ("genuine_pairs", "impostor_pairs", "roc_auc", "eer", "eer_threshold", "best_accuracy", "best_threshold"):
        assert want[key] == m[key] or (np.isnan(want[key]) and np.isnan(m[key])), key
    assert m["tar_at_far"] == want["tar_at_far"]
    assert 0.5 < m["roc_auc"] <= 1.0
    g = matching.Gallery([f"p{v}" for v in lab], torch.from_numpy(x), DEV)
    thr, tar = matching.threshold_for_far(g, 1e-2)
    assert (thr, tar) == want["tar_at_far"][1e-2]
    k = int(np.nonzero(t == np.float32(thr))[0][0])
    assert want["far"][k] <= 1e-2 and (k + 1 == len(t) or want["far"][k + 1] > 1e-2)   # the largest grid threshold within the FAR
    # the threshold carries over to compare_faces: held-out probes (new captures of enrolled people, and strangers) are accepted
    # exactly when their nearest enrolment is within it
    p_same, _ = _clustered(61, 800, 128, 60)          # same centres and labels, fresh noise below
    rng = np.random.default_rng(62)
    held = np.concatenate([p_same[:30] + 0.35 / np.sqrt(128) * rng.standard_normal((30, 128)).astype(np.float32),
                           3.0 * synth.unit_rows(63, 30, 128, "stranger").numpy()]).astype(np.float32)   # >= ~2 from any enrolment
    nearest = np.sqrt(exact_d2(held, x).min(axis=1)).astype(np.float32)
    decided = []
    for probe, d in zip(held, nearest):
        name, dist, idx = matching.compare_faces(torch.from_numpy(probe).to(DEV), g, thr)
        assert dist == d
        assert (idx is not None) == bool(d <= np.float32(thr))
        decided.append(idx is not None)
    assert any(decided) and not all(decided)
    # at the boundary itself: a probe is accepted at its own distance and rejected one fp32 step below
    for probe, d in zip(held[:3], nearest[:3]):
        pd = torch.from_numpy(probe).to(DEV)
        assert matching.compare_faces(pd, g, float(d))[2] is not None
        assert matching.compare_faces(pd, g, float(np.nextafter(d, np.float32(0))))[2] is None
