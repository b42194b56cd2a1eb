"""GPU: the matcher over the whole fp32 magnitude range (`range_cases.py`: unit rows scaled by 2^-149 .. 2^100, alone and mixed in
one call, the zero row among them) - top-1, top-k, verification counts and threshold search, unpacked and packed, against the
suite's float64-sum references, plus the pack itself, enrolment row by row and one captured replay.

Bars (the suite's own, no extra allowance): indices, labels, counts and pair lists equal; |dist - ref| <= 2e-6 + 1e-6 * ref; a
distance is +inf exactly where the reference lists nothing; packed and unpacked bit-equal wherever `test_match_topk_gpu._check`
demands it; k = 1 in entry mode bit-identical to `ops.match_top1`.

What these cases see that no narrower one does: a row below 2^-113, whose power-of-two scale 2^(14 - e) is 2^127 (subnormal inverse)
or +inf unless its exponent is clamped (csrc/match_scale_rule.h), and a row above about 2^64, whose fp32 squared norm is +inf so
that the expanded distance has no finite bound and the pair must be kept for the exact re-score (match_device.h: match_unbounded)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from frmap_amd import matching, ops  # noqa: E402

import match_cases as mc  # noqa: E402
import range_cases as rc  # noqa: E402
from test_match_radius_cpu import ref_radius  # noqa: E402
from test_match_topk_cpu import ref_topk  # noqa: E402
from test_match_topk_gpu import _check as check_topk  # noqa: E402
from test_verify_cpu import ref_verify_counts  # noqa: E402

DEV = "cuda"
ALL = [(cid, G, D) for cid in rc.CASE_IDS for (G, D) in rc.SHAPES]


@functools.lru_cache(maxsize=None)
def _case(cid, G, D):
    return rc.build(cid, G, D)


def _close(dist, ref, what):
    """|dist - ref| <= 2e-6 + 1e-6 * ref where the reference is finite, +inf exactly where it is not."""
    dd, rd = np.asarray(dist, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(rd)
    assert np.all(np.isinf(dd[~fin]) & (dd[~fin] > 0)), what
    assert np.isfinite(dd[fin]).all(), (what, int((~np.isfinite(dd[fin])).sum()))
    err = np.abs(dd[fin] - rd[fin]) - 1e-6 * rd[fin]
    assert err.size == 0 or float(err.max()) <= 2e-6, (what, float(err.max()))


def _prepared(gd, monkeypatch):
    monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)          # the split-fp16 GEMM at every gallery size
    return ops.match_prepare(gd)


@pytest.mark.parametrize("cid,G,D", ALL)
def test_top1_is_the_first_exact_minimum(cid, G, D, monkeypatch):
    c = _case(cid, G, D)
    first, dmin, _ = mc.float64_first_min(c.probes, c.gal)
    pd, gd = c.probes.to(DEV), c.gal.to(DEV)
    for packed in (False, True):
        prep = _prepared(gd, monkeypatch) if packed else None
        idx, dist, ids = ops.match_top1(pd, gd, thresh=float(np.float32(2.0 ** 65)), prepared=prep)
        monkeypatch.undo()
        bad = torch.nonzero(idx.cpu().long() != first).flatten().tolist()
        assert not bad, (cid, G, D, packed, [(p, int(idx[p]), int(first[p]), c.probe_exp[p]) for p in bad[:8]])
        _close(dist.cpu().numpy(), dmin.numpy(), (cid, G, D, packed))
        want_ids = torch.where(dist.cpu() <= float(np.float32(2.0 ** 65)), idx.cpu(), torch.full_like(idx.cpu(), -1))
        assert torch.equal(ids.cpu(), want_ids)


@pytest.mark.parametrize("cid,G,D", ALL)
def test_topk_entry_mode(cid, G, D, monkeypatch):
    c = _case(cid, G, D)
    check_topk(c.probes, c.gal, ks=(1, 5, 64), what=cid, monkeypatch=monkeypatch)


@pytest.mark.parametrize("cid,G,D", ALL)
def test_topk_identity_mode(cid, G, D, monkeypatch):
    c = _case(cid, G, D)
    check_topk(c.probes, c.gal, ks=(1, 5, 64), labels=c.labels_g, what=cid, monkeypatch=monkeypatch)


@pytest.mark.parametrize("cid,G,D", ALL)
def test_verify_counts_self_and_cross(cid, G, D, monkeypatch):
    c = _case(cid, G, D)
    p, g, lp, lg = c.probes.numpy(), c.gal.numpy(), c.labels_p.numpy(), c.labels_g.numpy()
    want_self = ref_verify_counts(g, lg, rc.THRESHOLDS)
    want_cross = ref_verify_counts(p, lp, rc.THRESHOLDS, g, lg)
    pd, gd = c.probes.to(DEV), c.gal.to(DEV)
    lpd, lgd = c.labels_p.to(DEV).to(torch.int32), c.labels_g.to(DEV).to(torch.int32)
    for packed in (False, True):
        prep = _prepared(gd, monkeypatch) if packed else None
        got_self = ops.verify_counts(gd, lgd, rc.THRESHOLDS, prepared=prep).cpu().numpy()
        got_cross = ops.verify_counts(pd, lpd, rc.THRESHOLDS, gd, lgd, prepared=prep).cpu().numpy()
        monkeypatch.undo()
        assert np.array_equal(got_self, want_self), (cid, G, D, packed, got_self.tolist(), want_self.tolist())
        assert np.array_equal(got_cross, want_cross), (cid, G, D, packed, got_cross.tolist(), want_cross.tolist())


@pytest.mark.parametrize("cid,G,D", ALL)
def test_match_radius_all_and_same(cid, G, D, monkeypatch):
    c = _case(cid, G, D)
    p, g, lp, lg = c.probes.numpy(), c.gal.numpy(), c.labels_p.numpy(), c.labels_g.numpy()
    P = p.shape[0]
    pd, gd = c.probes.to(DEV), c.gal.to(DEV)
    lpd, lgd = c.labels_p.to(DEV).to(torch.int32), c.labels_g.to(DEV).to(torch.int32)
    for thresh in rc.RADIUS_THRESHOLDS:
        thresh = float(np.float32(thresh))
        for which in ("all", "same"):
            wp, wd = ref_radius(p, g, thresh, None, (lp, lg), which)
            counts = np.bincount(wp[:, 0], minlength=P)
            want = {tuple(pr): d for pr, d in zip(wp.tolist(), wd.tolist())}
            for packed in (False, True):
                what = (cid, G, D, thresh, which, packed)
                prep = _prepared(gd, monkeypatch) if packed else None
                kw = dict(labels_a=lpd, labels_b=lgd, which=which, prepared=prep)
                pairs, dists, cnt = ops.match_radius(pd, thresh, gd, **kw)                      # count, then fill; sorted by (i, j)
                cap = len(wp) + 3
                cp, cd, ccnt, total = ops.match_radius(pd, thresh, gd, capacity=cap, **kw)      # one call into `cap` slots
                monkeypatch.undo()
                assert pairs.shape == (len(wp), 2) and np.array_equal(pairs.cpu().numpy().astype(np.int64), wp), what
                _close(dists.cpu().numpy(), wd, what)
                assert np.array_equal(cnt.cpu().numpy(), counts) and np.array_equal(ccnt.cpu().numpy(), counts), what
                assert total.tolist() == [len(wp)], what
                got = {tuple(pr): d for pr, d in zip(cp[:len(wp)].cpu().tolist(), cd[:len(wp)].cpu().tolist())}
                assert got.keys() == want.keys(), what
                _close([got[k] for k in want], [want[k] for k in want], what)


def _pack_is_finite(prep, rows, what):
    """The header's 'nothing overflows': every fp16 element of the pack finite; 1 / S of every row finite, nonzero, a normal power
    of two (mantissa field 0, biased exponent 1 .. 254); sum x, and band wherever sum x^2 is finite, not NaN."""
    half = prep.packed.view(torch.float16)
    assert bool(torch.isfinite(half).all()), (what, int((~torch.isfinite(half)).sum()))
    stat = prep.stat_w[:rows].cpu()
    inv = stat[:, 2]
    assert bool(torch.isfinite(inv).all()) and bool((inv != 0).all()), (what, inv[~torch.isfinite(inv) | (inv == 0)][:8])
    bits = inv.view(torch.int32)
    be = (bits >> 23) & 0xFF
    assert bool(((bits & 0x7FFFFF) == 0).all()) and bool((be >= 1).all()) and bool((be <= 254).all()) and bool((bits > 0).all()), what
    assert not bool(torch.isnan(stat).any()), what
    return half, stat


@pytest.mark.parametrize("cid,G,D", ALL)
def test_the_pack_holds_no_inf_nan_or_subnormal_scale(cid, G, D, monkeypatch):
    c = _case(cid, G, D)
    for name, rows in (("gallery", c.gal), ("probes", c.probes)):                # (probe rows take the same row-prep kernel)
        xd = rows.to(DEV)
        half, stat = _pack_is_finite(_prepared(xd, monkeypatch), rows.shape[0], (cid, G, D, name))
        monkeypatch.undo()
        amax = rows.abs().max(dim=1).values.double()
        scaled = amax / stat[:, 2].double()                                       # amax S, exact in float64
        assert bool((scaled < 2.0 ** 14).all()), (cid, G, D, name)
        live = amax >= 2.0 ** -113                                                # at or above the cut: the design range of the split
        assert bool((scaled[live] >= 2.0 ** 13).all()), (cid, G, D, name)
        assert bool((stat[amax == 0, 2] == 1.0).all())                            # a zero row keeps S = 1
        assert float(half.float().abs().max()) < 2.0 ** 14


def test_rows_at_the_scale_cut(monkeypatch):
    """Row maxima placed ON the binades around the cut 2^-113 (a unit row's largest element is about 2^-1.7, so the ladder's classes
    -115 / -114 / -113 all lie below it): 2^-115, 2^-114 (where an unclamped 2^(14 - e) is 2^127 with a subnormal inverse), 2^-113 and
    2^-112, each at the bottom, the middle and the top of its binade, next to unit rows."""
    D = 64
    unit = rc.synth.unit_rows(88, 12, D, "range_cut").double().numpy()
    unit /= np.abs(unit).max(axis=1, keepdims=True)                                   # largest |element| = 1
    maxima = [m * 2.0 ** e for e in (-115, -114, -113, -112) for m in (1.0, 1.5, 2.0 - 2.0 ** -23)]
    small = rc.f32(unit * np.asarray(maxima)[:, None])
    assert [float(r.abs().max()) for r in small] == [float(np.float32(m)) for m in maxima]
    gal = torch.cat([small, rc.synth.unit_rows(89, 58, D, "range_cut_unit")]).contiguous()      # 70 rows: one slot and a ragged one
    probes = torch.cat([small, rc.f32(unit * np.asarray(maxima)[::-1, None].copy()), gal[12:16], torch.zeros(1, D)]).contiguous()
    gd = gal.to(DEV)
    prep = _prepared(gd, monkeypatch)
    _, stat = _pack_is_finite(prep, gal.shape[0], "cut")
    scaled = gal.abs().max(dim=1).values.double() / stat[:, 2].double()
    assert bool((scaled[:6] < 2.0 ** 13).all()) and bool((scaled[6:] >= 2.0 ** 13).all()) and bool((scaled < 2.0 ** 14).all())
    assert bool((stat[:9, 2] == 2.0 ** -126).all()) and float(stat[9, 2]) == 2.0 ** -125
    monkeypatch.undo()
    check_topk(probes, gal, ks=(1, 5, 64), what="cut", monkeypatch=monkeypatch)
    first, dmin, _ = mc.float64_first_min(probes, gal)
    assert (first[:12] == 0).all()                                                    # exact ties across the twelve small rows: the first wins


def test_enrolment_row_by_row_equals_one_pack(monkeypatch):
    """A gallery prepared at capacity, then a row at 2^-140, one at 2^-114, one at 2^66 and a zero row appended through
    `Gallery.append` (frmap_match_pack_gallery_rows, across the slot boundary at row 64): pack and statistics bit-equal to the same
    gallery prepared in one go, answers equal to the reference."""
    G0, D = 60, 128
    c = _case("mixed", 65, D)
    monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
    g = matching.Gallery([f"id{i % 7}" for i in range(G0)], c.gal[:G0], DEV)
    unit = rc.synth.unit_rows(77, 4, D, "range_enrol").double().numpy()
    g.append("id4", torch.from_numpy(unit[0].astype(np.float32)))                # (out of room: the buffer grows, a fresh pack at capacity)
    pack = g._pack
    assert pack is not None and pack.capacity >= G0 + 5
    new = [rc.f32(unit[1] * 2.0 ** -140), rc.f32(unit[2] * 2.0 ** -114), rc.f32(unit[3] * 2.0 ** 66), torch.zeros(D)]
    for j, row in enumerate(new):
        assert g.append(f"id{(G0 + 1 + j) % 7}", row) == G0 + 1 + j
        assert g._pack is pack                                                   # re-packed in place, row by row
    G = G0 + 5
    whole = g.matrix.clone()
    once = ops.match_prepare(whole)
    torch.cuda.synchronize()
    assert torch.equal(pack.stat_w[:G].view(torch.int32), once.stat_w[:G].view(torch.int32))
    n = min(pack.packed.numel(), once.packed.numel())
    assert n == once.packed.numel() and torch.equal(pack.packed[:n], once.packed)
    _pack_is_finite(pack, G, "enrolled")
    gal = whole.cpu()
    assert torch.equal(gal[G0 + 1:], torch.stack(new))
    probes = torch.cat([c.probes, torch.stack(new), rc.f32(unit[1:] * 2.0 ** 66 * (1 + 2.0 ** -12))])
    ref_i, ref_d, _ = ref_topk(probes.numpy(), gal.numpy(), 5)
    idx, dist, _ = ops.match_topk(probes.to(DEV), g.matrix, 5, prepared=pack)
    assert np.array_equal(idx.cpu().long().numpy(), ref_i)
    _close(dist.cpu().numpy(), ref_d, "enrolled top-5")
    i1, d1 = ops.match_top1(probes.to(DEV), g.matrix, prepared=pack)
    assert np.array_equal(i1.cpu().long().numpy(), ref_i[:, 0])
    _close(d1.cpu().numpy(), ref_d[:, 0], "enrolled top-1")
    want = ref_verify_counts(gal.numpy(), np.arange(G) % 7, rc.THRESHOLDS)
    got = ops.verify_counts(g.matrix, (torch.arange(G) % 7).to(DEV).to(torch.int32), rc.THRESHOLDS, prepared=pack)
    assert np.array_equal(got.cpu().numpy(), want)


def test_captured_packed_topk_replays_on_other_magnitudes(monkeypatch):
    """Captured on `mixed`, replayed on `split` data of the same shape written into the same buffers (and re-packed there): per-row
    scales are data, nothing about them may be baked in at capture time."""
    G, D, k = 200, 64, 5
    a, b = _case("mixed", G, D), _case("split", G, D)
    P = min(a.probes.shape[0], b.probes.shape[0])
    monkeypatch.setattr(ops, "MATCH_MFMA_MIN_G", 1)
    pd, gd = a.probes[:P].to(DEV).contiguous(), a.gal.to(DEV).contiguous()
    prep = ops.match_prepare(gd)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ops.match_topk(pd, gd, k, prepared=prep)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.match_topk(pd, gd, k, prepared=prep)
    graph.replay()
    torch.cuda.synchronize()
    ref_i, ref_d, _ = ref_topk(a.probes[:P].numpy(), a.gal.numpy(), k)
    assert np.array_equal(out[0].cpu().long().numpy(), ref_i)
    pd.copy_(b.probes[:P])
    gd.copy_(b.gal)
    prep.update_rows(gd, 0, G)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    gi, gdist = out[0].clone(), out[1].clone()
    ei, edist, _ = ops.match_topk(pd, gd, k, prepared=prep)
    assert torch.equal(gi, ei) and torch.equal(gdist, edist)
    ref_i, ref_d, _ = ref_topk(b.probes[:P].numpy(), b.gal.numpy(), k)
    assert np.array_equal(gi.cpu().long().numpy(), ref_i)
    _close(gdist.cpu().numpy(), ref_d, "replay")
