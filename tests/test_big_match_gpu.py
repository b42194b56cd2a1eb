"""GPU: the gallery matcher on a gallery past the 2 GiB and 4 GiB offset marks, in its fp32 form and in its packed split-fp16 form.

The gallery is a block of 4,099 unit rows (512-d, `synth.unit_rows`) tiled on the device to G = 2^22 + 2 x 4,099 + 5 rows: 8 GiB
of fp32 (past 2^31 bytes at row 2^20, 2^32 bytes at row 2^21 and 2^31 elements at row 2^22) and 12 GiB packed (3 x 512 fp16 a row:
past 2^31 bytes at row 699,050 and past 2^32 bytes = 2^31 elements at row 1,398,101).  4,099 is an odd prime: no mark is a
multiple of the period (`big_cases.assert_period`).  Planted rows are near-copies (1e-3 away) of their own probes: the first row;
the last row before and the first after every mark of both forms, by rows and by the packed form's 64-row tiles; the last row.

* A probe with a plant returns the plant's row and its exact distance (the existing test's bar: 2e-6 + 1e-6 d).
* A probe without one returns the FIRST occurrence of the block's best row - an index below the period, with 1,025 exact
  copies of it further on: first-minimum tie-breaking across the whole gallery.
* The margins are asserted on the CPU in float64 against the block, never a fixed number: a plant is closer than every block
  row and every other plant by more than the distance tolerance plus the block's own runner-up gap for that probe; the
  block's best row is unique within the block by more than the tolerance.
* `match_topk` by row: the plant, then the copies of the best block row in ascending row order; by identity (label = row modulo
  the period, plants their own): the k nearest identities, each at its first row.
* The packed gallery built in one call equals the one built by appending rows across its 4 GiB mark, byte for byte.

* `match_radius` over the whole gallery: a threshold that admits exactly the plants, and one whose per-probe counts follow in
  closed form from the block's float64 distances and the number of copies of each row.
* `verify_counts` on 65,536 x 65,537 tiled labelled rows (past 2^32 pairs): genuine / impostor counts in closed form.

Both run on the split-fp16 GEMM path (a prepared B); the exact scans of the same entry points visit every pair in float64 and
have no case of a few seconds at these sizes: their address arithmetic is the pair feed of `match_device.h` ("Large
tensors"), which the GEMM path's exact re-score shares."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import big_cases as bc  # noqa: E402
import guard  # noqa: E402
from frmap_amd import ops, synth  # noqa: E402

DEV = "cuda"
D = 512
PERIOD = 4099
G = 2 ** 22 + 2 * PERIOD + 5
TILE = 64                                      # rows per tile of the packed form
ROW_F32, ROW_PACKED = D * 4, 3 * D * 2
TOL = lambda d: 2e-6 + 1e-6 * d                # the distance bar of test_match_exact_gpu.py


def _mark_rows():
    """Rows next to every mark: (last row wholly before | holding the mark, first after), by rows and by 64-row tiles."""
    rows = {0, G - 1}
    for row_bytes, elem in ((ROW_F32, 4), (ROW_PACKED, 2)):
        for mark in bc.marks_in_bytes(elem):
            r = mark // row_bytes
            rows |= {r - 1, r, r + 1}
            t = r // TILE * TILE
            rows |= {t - 1, t, t + TILE - 1, t + TILE}
    assert all(0 <= r < G for r in rows)
    return sorted(rows)


@pytest.fixture(scope="module")
def case():
    """The block, the probes and plants, the float64 expectations (CPU), and the gallery on the device with its pack."""
    bc.assert_period(ROW_F32, 4, PERIOD, what="gallery fp32")
    bc.assert_period(ROW_PACKED, 2, PERIOD, what="gallery packed")
    assert G * ROW_F32 > 2 ** 33 + 2 * PERIOD * ROW_F32 and G * ROW_PACKED > 2 ** 32 + 2 * PERIOD * ROW_PACKED
    bc.need_memory(bc.estimate_bytes([G * ROW_F32, (G + 255) // 256 * 256 * ROW_PACKED, G * 16, G * 4, 2 * 2 ** 30]), "match gallery")
    block = synth.unit_rows(5151, PERIOD, D, "gal")
    rows = _mark_rows()
    n_free = 4
    probes = synth.unit_rows(5152, len(rows) + n_free, D, "probe")
    noise = synth.unit_rows(5153, len(rows), D, "noise")
    plants = (probes[:len(rows)].double() + 1e-3 * noise.double()).float()

    # candidates of the full gallery, by their FIRST row: block row b at b (or its next copy where a plant sits on it), the plants
    planted = set(rows)
    first = []
    for b in range(PERIOD):
        r = b
        while r in planted:
            r += PERIOD
        first.append(r)
    cand_idx = torch.tensor(first + rows, dtype=torch.int64)
    cand = torch.cat([block, plants])
    diff = (probes[:, None, :] - cand[None, :, :]) + torch.tensor(1e-6, dtype=torch.float32)      # fp32 elements, as the kernel
    d = diff.double().pow(2).sum(-1).sqrt()                                                         # [P, PERIOD + plants]
    order = torch.from_numpy(np.lexsort((cand_idx.numpy()[None, :].repeat(len(probes), 0), d.numpy()), axis=1))
    best = order[:, 0]
    want_idx, want_dist = cand_idx[best], d.gather(1, best[:, None])[:, 0]
    # margins
    db = d[:, :PERIOD].sort(dim=1).values
    gap_block = db[:, 1] - db[:, 0]                                                                 # the block's runner-up gap
    for i in range(len(probes)):
        tol = TOL(float(db[i, 0]))
        if i < len(rows):
            assert int(want_idx[i]) == rows[i], (i, "the plant is not the nearest row")
            others = torch.cat([d[i, :PERIOD], d[i, PERIOD:PERIOD + i], d[i, PERIOD + i + 1:]])
            assert float(others.min() - want_dist[i]) > tol + float(gap_block[i]), (i, "plant margin")
        else:
            assert int(want_idx[i]) < PERIOD and int(best[i]) < PERIOD and float(gap_block[i]) > 2 * tol, (i, "best block row not unique")
            assert float(d[i, PERIOD:].min() - want_dist[i]) > 2 * tol, (i, "a plant of another probe is as near")

    gal = bc.tile_on_device(block.to(DEV), G)
    gal[torch.tensor(rows, device=DEV)] = plants.to(DEV)
    prep = ops.match_prepare(gal)
    torch.cuda.synchronize()
    yield {"block": block, "rows": rows, "probes": probes, "plants": plants, "d": d, "order": order, "cand_idx": cand_idx,
           "want_idx": want_idx, "want_dist": want_dist, "gal": gal, "prep": prep, "n_free": n_free}
    del gal, prep
    torch.cuda.empty_cache()


def _check_top1(c, idx, dist, what):
    idx, dist = idx.cpu().long(), dist.cpu().double()
    bad = (idx != c["want_idx"]).nonzero().flatten().tolist()
    assert not bad, (what, [(b, int(idx[b]), int(c["want_idx"][b]), int(idx[b]) % PERIOD) for b in bad])
    err = (dist - c["want_dist"]).abs() - 1e-6 * c["want_dist"]
    assert float(err.max()) <= 2e-6, (what, float(err.max()))
    assert bool((idx[-c["n_free"]:] < PERIOD).all()), "first occurrence"


def _gallery_intact(c):
    """The first and the last whole period still hold the block, the planted rows their plants."""
    blk = c["block"].to(DEV)
    planted = torch.zeros(G, dtype=torch.bool, device=DEV)
    planted[torch.tensor(c["rows"], device=DEV)] = True
    for start in (0, (G // PERIOD - 1) * PERIOD):
        keep = ~planted[start:start + PERIOD]
        assert torch.equal(c["gal"][start:start + PERIOD][keep].view(torch.int32), blk[keep].view(torch.int32)), ("gallery modified", start)
    assert torch.equal(c["gal"][torch.tensor(c["rows"], device=DEV)].cpu(), c["plants"])


def test_marks_have_a_plant_on_each_side(case):
    rows = set(case["rows"])
    assert {0, G - 1, 2 ** 20 - 1, 2 ** 20, 2 ** 21 - 1, 2 ** 21, 2 ** 22 - 1, 2 ** 22, 699050, 699051, 1398101, 1398102} <= rows
    assert {699008 - 1, 699008, 699071, 699072} <= rows                  # the packed tile that holds byte 2^31
    assert G // PERIOD - 1 > 500                                          # exact copies of every block row further on


@pytest.mark.parametrize("form", ["fp32", "packed"])
def test_match_top1_across_the_marks(case, form):
    c = case
    g = guard.Guard(0xFF)
    with g.patch(ops):
        idx, dist = ops.match_top1(c["probes"].to(DEV), c["gal"], prepared=c["prep"] if form == "packed" else None)
    g.check()
    _check_top1(c, idx, dist, form)
    _gallery_intact(c)


@pytest.mark.parametrize("form", ["fp32", "packed"])
def test_match_topk_rows_plant_then_copies_in_row_order(case, form):
    c, k = case, 8
    g = guard.Guard(0xFF)
    with g.patch(ops):
        idx, dist, _ = ops.match_topk(c["probes"].to(DEV), c["gal"], k, prepared=c["prep"] if form == "packed" else None)
    g.check()
    idx, dist = idx.cpu().long(), dist.cpu().double()
    planted = set(c["rows"])
    for i in range(len(c["probes"])):
        want, wd = [], []
        for j in c["order"][i].tolist():                                  # candidates by (distance, first row)
            if j >= PERIOD:
                want.append(int(c["cand_idx"][j])); wd.append(float(c["d"][i, j]))
            else:                                                         # a block row: every copy of it, in row order
                copies = [r for r in range(j, G, PERIOD) if r not in planted][:k]
                want += copies; wd += [float(c["d"][i, j])] * len(copies)
            if len(want) >= k:
                break
        assert idx[i].tolist() == want[:k], (form, i, idx[i].tolist(), want[:k])
        assert all(abs(float(dist[i, t]) - wd[t]) <= TOL(wd[t]) for t in range(k)), (form, i)
    top1 = ops.match_top1(c["probes"].to(DEV), c["gal"], prepared=c["prep"] if form == "packed" else None)
    assert torch.equal(idx[:, 0], top1[0].cpu().long()) and torch.equal(dist[:, 0].float(), top1[1].cpu())


def test_match_topk_identities_at_their_first_rows(case):
    """Identity = row modulo the period for the tiled rows, one of its own for every plant: the k nearest identities are the k
    nearest candidates, each reported at its first row (the copies of an identity 4,099 rows further on all tie with it)."""
    c, k = case, 5
    labels = (torch.arange(G, dtype=torch.int32, device=DEV) % PERIOD)
    labels[torch.tensor(c["rows"], device=DEV)] = PERIOD + torch.arange(len(c["rows"]), dtype=torch.int32, device=DEV)
    idx, dist, lab = ops.match_topk(c["probes"].to(DEV), c["gal"], k, labels=labels, prepared=c["prep"])
    idx, dist, lab = idx.cpu().long(), dist.cpu().double(), lab.cpu().long()
    for i in range(len(c["probes"])):
        top = c["order"][i, :k]
        assert float((c["d"][i, c["order"][i, 1:k + 1]] - c["d"][i, top]).min()) > 0, "a tie between identities"
        assert idx[i].tolist() == c["cand_idx"][top].tolist(), (i, idx[i].tolist(), c["cand_idx"][top].tolist())
        assert lab[i].tolist() == [int(j) for j in top], (i, "labels")
        assert float(((dist[i] - c["d"][i, top]).abs() - 1e-6 * c["d"][i, top]).max()) <= 2e-6


def test_packed_gallery_appended_across_its_4gib_mark_equals_the_rebuilt_one(case):
    """`MatchPack.update_rows` (incremental enrolment) from 1,398,000 to 1,398,300 rows: the rows on both sides of byte 2^32 of
    the packed form, whose 64-row tiles are re-packed in place.  Every byte equals the pack built from all rows at once."""
    c = case
    lo, hi = 1398000, 1398300
    assert lo * ROW_PACKED < 2 ** 32 < hi * ROW_PACKED
    full = c["gal"][:hi]
    whole = ops.MatchPack(full)
    grown = ops.MatchPack(c["gal"][:lo], capacity=hi)
    grown.update_rows(full, lo, hi)
    torch.cuda.synchronize()
    assert whole.packed.numel() == grown.packed.numel() > 2 ** 32
    for a0 in range(0, whole.packed.numel(), bc.CHUNK_BYTES):
        assert torch.equal(whole.packed[a0:a0 + bc.CHUNK_BYTES], grown.packed[a0:a0 + bc.CHUNK_BYTES]), ("packed bytes differ from offset", a0)
    assert torch.equal(whole.stat_w.view(torch.int32), grown.stat_w.view(torch.int32))
    probes = c["probes"].to(DEV)
    a, b = ops.match_top1(probes, full, prepared=whole), ops.match_top1(probes, full, prepared=grown)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    del whole, grown
    torch.cuda.empty_cache()


def _copies(c):
    """Rows of the full gallery that hold candidate j (a block row: its unplanted copies; a plant: its row), as counts."""
    planted = np.zeros(G, dtype=bool)
    planted[c["rows"]] = True
    n = np.array([(G - 1 - b) // PERIOD + 1 - int(planted[b::PERIOD].sum()) for b in range(PERIOD)] + [1] * len(c["rows"]), dtype=np.int64)
    assert int(n.sum()) == G
    return n


def test_match_radius_counts_follow_from_the_tiling(case):
    """Two thresholds.  0.01 admits exactly the plants (each 1e-3 from its probe; every other row is beyond 1.2): the list is
    (probe, its plant's row) with the exact distance.  The midpoint between the best and the second-best block distance of an
    unplanted probe admits, for every probe, whole families of copies: per-probe counts and the total are the block's float64
    counts times the copies of each row - a closed form, past 4 GiB of gallery on both sides of every mark."""
    c = case
    probes, n_rows = c["probes"].to(DEV), len(c["rows"])
    pairs, dists, counts = ops.match_radius(probes, 0.01, b=c["gal"], prepared=c["prep"])
    assert pairs.cpu().tolist() == [[i, r] for i, r in enumerate(c["rows"])]
    assert counts.cpu().tolist() == [1] * n_rows + [0] * c["n_free"]
    wd = c["want_dist"][:n_rows]
    assert float(((dists.cpu().double() - wd).abs() - 1e-6 * wd).max()) <= 2e-6
    j = n_rows                                                            # the first probe without a plant
    db = c["d"][j, :PERIOD].sort().values
    t = float((db[0] + db[1]) / 2)
    assert float((c["d"] - t).abs().min()) > 2 * TOL(t), "a candidate distance sits on the threshold"
    want = ((c["d"] <= t).numpy() * _copies(c)[None, :]).sum(axis=1)
    assert int(want[j]) == int(_copies(c)[int(c["order"][j, 0])]) > 500
    g = guard.Guard(0xFF)
    with g.patch(ops):
        _, _, cnt, total = ops.match_radius(probes, t, b=c["gal"], prepared=c["prep"], capacity=0)
    g.check()
    assert cnt.cpu().tolist() == want.tolist() and int(total) == int(want.sum())


def test_verify_counts_past_2_to_the_32_pairs():
    """65,536 x 65,537 labelled rows (cross mode, packed B): 4,295,032,832 pairs, past 2^32.  A and B are blocks of 7 and 11 unit
    rows tiled; the accepted genuine / impostor counts at thresholds between the block's 77 distances are the block's float64
    counts times the multiplicities of each row pair: what only 64-bit counters hold (the impostor total alone passes 2^31)."""
    P, Q, Ka, Kb = 65536, 65537, 7, 11
    assert P * Q > 2 ** 32
    ba, bb = synth.unit_rows(6161, Ka, D, "a"), synth.unit_rows(6162, Kb, D, "b")
    bb[3] = (ba[2].double() + 1e-2 * synth.unit_rows(6163, 1, D, "n")[0].double()).float()       # one close pair, genuine
    la, lb = torch.arange(Ka, dtype=torch.int32) % 3, (torch.arange(Kb, dtype=torch.int32) + 2) % 3
    diff = (ba[:, None, :] - bb[None, :, :]) + torch.tensor(1e-6, dtype=torch.float32)
    d = diff.double().pow(2).sum(-1).sqrt()                                                      # [Ka, Kb]
    ds = d.flatten().sort().values
    cuts = [0, 1, 20, 50, 76]
    thr = [float((ds[i] + ds[i + 1]) / 2) if i + 1 < ds.numel() else float(ds[i] + 0.1) for i in cuts]
    for t in thr:
        assert float((d - t).abs().min()) > 2 * TOL(t), "a block distance sits on a threshold"
    ma = np.array([(P - 1 - u) // Ka + 1 for u in range(Ka)], dtype=np.int64)
    mb = np.array([(Q - 1 - v) // Kb + 1 for v in range(Kb)], dtype=np.int64)
    mult = ma[:, None] * mb[None, :]
    same = (la[:, None] == lb[None, :]).numpy()
    want = np.array([[int((mult * ((d.numpy() <= t) & s)).sum()) for t in thr] for s in (same, ~same)])
    assert int(mult.sum()) == P * Q and want[1, -1] > 2 ** 31 and want[:, -1].sum() == P * Q
    a, b = bc.tile_on_device(ba.to(DEV), P), bc.tile_on_device(bb.to(DEV), Q)
    lad, lbd = la.to(DEV).repeat(P // Ka + 1)[:P].contiguous(), lb.to(DEV).repeat(Q // Kb + 1)[:Q].contiguous()
    prep = ops.match_prepare(b)
    g = guard.Guard(0xFF)
    with g.patch(ops):
        got = ops.verify_counts(a, lad, thr, b, lbd, prepared=prep)
    g.check()
    assert got.cpu().tolist() == want.tolist(), (got.cpu().tolist(), want.tolist())
