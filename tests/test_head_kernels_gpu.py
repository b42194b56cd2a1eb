"""GPU: the fp32 head kernels (`csrc/head_match.hip`) and the grid-stride loops of `csrc/layout_pool.hip` at the shapes where
they switch paths, against float64 references; tolerances are the ones the older tests use for the same op.

* `gap_norm_match`: the sixteen-loads-in-flight pooling loop (HW > 15 row subsets), one and two scan passes (G <= 40 < G), G = 1,
  64 and 0, C >= 2048 (one subset, a loop over channel groups), C / 8 that does not divide 256, ties across waves and passes
  (its last step, `match_write_top1`, is the one `match_small_kernel` and `match_finalize_rec_kernel` end in);
* `gemm_nt_f32_kernel` through `linear_f32`, `cosine_logits` and `arcmargin_eval`: the K tail (K % 32 != 0), several row blocks,
  fewer than 128 columns, first-index-wins of the arg-max inside a wave, across waves and across workgroups;
* `gap_linear_norm` at K / 8 = 24 (idle lanes) and K = 8; `softmax_argmax`, `pairwise_distance`, `l2_normalize` at widths below,
  at and above one wave; `cast_*` and `maxpool` with more items than threads in the grid.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from frmap_amd import ops, synth  # noqa: E402
from oracle import face_oracle as fo  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]


# --------------------------------------------------------------------------------------------------------------------------------
# gap_norm_match
# --------------------------------------------------------------------------------------------------------------------------------
def _gnm_map(seed, B, HW, C, dtype):
    """A non-negative map (as after a ReLU) with a per-face channel gain, so the pooled embeddings of two faces point apart."""
    return (torch.relu(synth.randn(seed, (B, HW, C), "map") + 0.3) * synth.randn(seed, (B, 1, C), "gain").abs() * 0.5).to(dtype)


def _gnm_ref(fmap, gal, normalize, eps=1e-12):
    e = fmap.double().mean(dim=1)
    if normalize:
        e = e / e.norm(dim=1, keepdim=True).clamp_min(eps)
    if gal is None:
        return e, None
    return e, torch.sqrt(((e[:, None, :] - gal.double()[None] + 1e-6) ** 2).sum(-1))


# C = 512: 4 row subsets, the 16-deep loop needs HW > 60: 49 tail only; 64 one trip for subsets 0..3; 200 three trips + tail
# C = 256 / 192 / 8: 8 / 10 / 256 subsets (192: C / 8 = 24 does not divide 256, 16 idle threads; HW = 121, 130 < 15 subsets + 1:
# tail only, HW = 16 < 256 subsets: most subsets empty); C = 2048: C / 8 = 256, the one-subset branch, HW = 20 > 15: one trip
# G = 36, 7, 5, 3: one scan pass; 40: exactly one; 41: a second pass of one row; 64: two passes; 1; 0: no gallery
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,HW,C,G", [(5, 49, 512, 36), (3, 64, 512, 41), (3, 200, 512, 64), (2, 121, 256, 1), (2, 130, 192, 40),
                                      (2, 20, 2048, 7), (3, 1, 512, 5), (2, 16, 8, 3), (2, 49, 512, 0)])
def test_gap_norm_match_paths(B, HW, C, G, dtype):
    """One launch against float64 and against avgpool_global -> l2_normalize -> match_top1, `normalize` on and off, packed and
    unpacked, a threshold that splits the batch (face 0 has a planted near hit at a third of the typical distance)."""
    fmap = _gnm_map(900 + HW + G, B, HW, C, dtype)
    fd = fmap.view(B, 1, HW, C).to(DEV)
    for normalize in (True, False):
        e64, _ = _gnm_ref(fmap, None, normalize)
        pooled = ops.avgpool_global(fd)
        emb_u = ops.l2_normalize(pooled, 1e-12) if normalize else pooled
        if G == 0:
            idx, dist, ids, pk, emb = ops.gap_norm_match(fd, None, 1.0, normalize=normalize, want_emb=True, packed=True)
            assert torch.allclose(emb.cpu().double(), e64, atol=1e-6) and torch.allclose(emb, emb_u, atol=1e-6)
            assert bool((idx == -1).all()) and bool(torch.isinf(dist).all()) and bool((ids == -1).all())
            assert bool((pk[:, 0] == -1).all()) and bool(torch.isinf(pk.view(torch.float32)[:, 1]).all())
            continue
        scale = 1.0 if normalize else float(e64.norm(dim=1).mean())
        gal = synth.unit_rows(910 + G, G, C).double() * scale
        near = e64[0] + 0.3 * scale * synth.unit_rows(911, 1, C, "near")[0].double()
        gal[G // 2] = near
        gal = gal.float()
        _, d64 = _gnm_ref(fmap, gal, normalize)
        want_d, want_i = d64.min(dim=1)
        if G > 1:                                     # the float64 winner must be clear of fp32 rounding for `idx ==` to be fair
            top2 = d64.topk(2, dim=1, largest=False).values
            assert float((top2[:, 1] - top2[:, 0]).min()) > 1e-4 * scale
        srt = want_d.sort().values
        thr = float(srt[0] + srt[1]) / 2              # face 0 (the near hit) inside, every other face outside
        assert int(want_i[0]) == G // 2 and float(srt[1] - srt[0]) > 0.1 * scale
        want_ids = torch.where(want_d <= thr, want_i, torch.full_like(want_i, -1)).int()
        for packed in (False, True):
            idx, dist, ids, pk, emb = ops.gap_norm_match(fd, gal.to(DEV), thr, normalize=normalize, want_emb=True, packed=packed)
            assert torch.allclose(emb.cpu().double(), e64, atol=1e-6), (normalize, float((emb.cpu().double() - e64).abs().max()))
            assert torch.equal(idx.cpu(), want_i.int()), (normalize, idx.cpu(), want_i)
            assert torch.allclose(dist.cpu().double(), want_d, rtol=1e-5, atol=0), (normalize, dist.cpu(), want_d)
            assert torch.equal(ids.cpu(), want_ids)
            if packed:
                assert torch.equal(pk[:, 0], ids) and torch.equal(pk.view(torch.float32)[:, 1], dist)
            else:
                assert pk is None
        idx_u, dist_u, ids_u = ops.match_top1(emb_u, gal.to(DEV), thr)
        assert torch.equal(idx, idx_u) and torch.equal(ids, ids_u)
        assert torch.allclose(dist, dist_u, atol=1e-5) and torch.allclose(emb, emb_u, atol=1e-6)
        idx0, dist0, ids0, _, emb0 = ops.gap_norm_match(fd, gal.to(DEV), None, normalize=normalize, want_emb=False)
        assert ids0 is None and emb0 is None and torch.equal(idx0, idx) and torch.equal(dist0, dist)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gap_norm_match_ties_across_waves_and_passes(dtype):
    """Gallery rows 3, 6, 45, 63 are identical and equal to face 0's embedding: row 3 is scored by wave 3 in pass 0, row 6 by
    wave 2 in pass 0, rows 45 and 63 by waves 1 and 3 in pass 1.  The first index wins, as in `compare_faces`."""
    B, HW, C, G = 3, 200, 512, 64
    fmap = _gnm_map(950, B, HW, C, dtype)
    fd = fmap.view(B, 1, HW, C).to(DEV)
    e64, _ = _gnm_ref(fmap, None, True)
    gal = synth.unit_rows(951, G, C)
    for r in (3, 6, 45, 63):
        gal[r] = e64[0].float()
    idx, dist, _, _, emb = ops.gap_norm_match(fd, gal.to(DEV), None, normalize=True, want_emb=True)
    assert int(idx[0]) == 3 and float(dist[0]) < 1e-4
    assert idx.cpu().tolist()[1:] == _gnm_ref(fmap, gal, True)[1].argmin(dim=1).tolist()[1:]
    idx_u, _ = ops.match_top1(emb, gal.to(DEV))
    assert torch.equal(idx, idx_u)
    gal2 = gal.clone()
    gal2[3] = gal[0]                                  # without row 3 the first copy is row 6: another wave, same pass
    assert int(ops.gap_norm_match(fd, gal2.to(DEV), None, normalize=True)[0][0]) == 6
    gal2[6] = gal[1]                                  # ... then row 45, in the second pass
    assert int(ops.gap_norm_match(fd, gal2.to(DEV), None, normalize=True)[0][0]) == 45


# --------------------------------------------------------------------------------------------------------------------------------
# gap_linear_norm
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,K,N", [(9, 5, 5, 192, 256), (17, 2, 2, 8, 512)])
def test_gap_linear_norm_idle_lanes_and_tiny_k(B, H, W, K, N, dtype):
    """K = 192: K / 8 = 24 channel groups do not divide the 64 lanes, lanes 48..63 of the pooling stage hold no row subset and
    must stay idle; K = 8: a single channel group.  The checks are those of `test_fused_arcface_head`."""
    fmap = torch.relu(synth.randn(9840 + K, (B, H, W, K), "m")).to(dtype)
    w = synth.randn(9841 + K, (N, K), "w") * (1.0 / math.sqrt(K))
    scale = 1.0 + 0.1 * synth.randn(9842, (N,), "s")
    shift = 0.1 * synth.randn(9843, (N,), "b")
    pooled = fmap.float().mean(dim=(1, 2))
    pre_ref = (pooled.double() @ w.double().t()).float() * scale + shift
    emb_ref = F.normalize(pre_ref, p=2, dim=1, eps=1e-12)
    emb, pre = ops.gap_linear_norm(fmap.to(DEV), w.t().contiguous().to(DEV), scale.to(DEV), shift.to(DEV), 1e-12, want_pre=True)
    assert torch.allclose(pre.cpu(), pre_ref, atol=2e-5, rtol=2e-5), float((pre.cpu() - pre_ref).abs().max())
    assert torch.allclose(emb.cpu(), emb_ref, atol=2e-6, rtol=2e-5), float((emb.cpu() - emb_ref).abs().max())
    assert torch.allclose(emb.norm(dim=1).cpu(), torch.ones(B), atol=1e-5)
    three = ops.l2_normalize(ops.linear_f32(ops.avgpool_global(fmap.to(DEV)), w.to(DEV), scale.to(DEV), shift.to(DEV)), 1e-12)
    assert torch.allclose(emb, three, atol=2e-6, rtol=2e-5), "fused and three-launch heads differ"
    emb_r, pre_r = ops.gap_linear_norm(fmap.to(DEV), w.t().contiguous().to(DEV), None, shift.to(DEV), 1e-12, want_pre=True, relu=True)
    pre_rr = F.relu((pooled.double() @ w.double().t()).float() + shift)
    assert torch.allclose(pre_r.cpu(), pre_rr, atol=2e-5, rtol=2e-5), "relu head"
    assert torch.allclose(emb_r.cpu(), F.normalize(pre_rr, p=2, dim=1, eps=1e-12), atol=2e-6, rtol=2e-5), "relu head, normalised"


# --------------------------------------------------------------------------------------------------------------------------------
# gemm_nt_f32_kernel: linear_f32, cosine_logits, arcmargin_eval
# --------------------------------------------------------------------------------------------------------------------------------
# K = 4, 36, 100, 8: the last 32-wide K step is partial (`k0 + skq < K`); B = 65, 130: 2 and 3 row blocks with a ragged last
# one; N = 5, 1: one partial column block; N = 129: a second column block of one column
@pytest.mark.parametrize("B,K,N", [(3, 4, 5), (65, 36, 129), (64, 100, 128), (130, 8, 1)])
def test_linear_f32_k_tail_and_ragged_blocks(B, K, N):
    x = synth.randn(1041, (B, K), "x")
    w = synth.randn(1042, (N, K), "w") / math.sqrt(K)
    sc = synth.randn(1043, (N,), "s").abs() + 0.5
    sh = synth.randn(1044, (N,), "h")
    ref = (x.double() @ w.double().t()) * sc.double() + sh.double()
    for relu in (False, True):
        y = ops.linear_f32(x.to(DEV), w.to(DEV), sc.to(DEV), sh.to(DEV), relu).cpu()
        r = ref.clamp_min(0) if relu else ref
        assert torch.allclose(y.double(), r, atol=2e-5, rtol=2e-5), (relu, float((y.double() - r).abs().max()))
    y2 = ops.linear_f32(x.to(DEV), w.to(DEV)).cpu()
    assert torch.allclose(y2.double(), x.double() @ w.double().t(), atol=2e-5, rtol=2e-5)


def test_linear_f32_refuses_k_not_multiple_of_4():
    with pytest.raises(ValueError, match="linear_f32"):
        ops.linear_f32(torch.zeros(3, 6, device=DEV), torch.zeros(5, 6, device=DEV))


def _cos64(x, w):
    return F.normalize(x.double(), dim=1, eps=1e-12) @ F.normalize(w.double(), dim=1, eps=1e-12).t()


# B = 130: three row blocks; C = 300, 1000: 3 and 8 workgroups per row meeting in one atomicMax; C = 1, 129: one column, and a
# second workgroup of one column; D = 36, 4, 100: a partial last K step
@pytest.mark.parametrize("B,C,D", [(130, 300, 36), (64, 1, 512), (65, 129, 4), (7, 1000, 100)])
def test_cosine_logits_blocks_tail_and_first_index_argmax(B, C, D):
    x = synth.randn(1100 + D, (B, D), "x")
    w = synth.randn(1101 + D, (C, D), "w")
    cos = _cos64(x, w)
    if C > 1:                                         # the float64 winner must be clear of fp32 rounding on every row
        top2 = cos.topk(2, dim=1).values
        assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-5
    logits, arg = ops.cosine_logits(x.to(DEV), w.to(DEV), s=32.0)
    assert torch.allclose(logits.cpu().double(), cos * 32.0, atol=1e-4), float((logits.cpu().double() - cos * 32.0).abs().max())
    assert arg.cpu().tolist() == cos.argmax(1).tolist()
    none, arg2 = ops.cosine_logits(x.to(DEV), w.to(DEV), s=1.0, want_logits=False)
    assert none is None and arg2.cpu().tolist() == cos.argmax(1).tolist()
    # planted ties: weight row j is a copy of row 5 and probe 2 is aligned with both - column 20 sits in the same wave as
    # column 5, column 70 in another wave of the workgroup, column 700 in another workgroup: the lowest index is returned
    for j in (20, 70, 700):
        if j >= C:
            continue
        w2, x2 = w.clone(), x.clone()
        w2[j] = w2[5]
        x2[2] = 3.0 * w2[5]
        for want_logits in (True, False):
            lg, a = ops.cosine_logits(x2.to(DEV), w2.to(DEV), s=32.0, want_logits=want_logits)
            assert int(a[2]) == 5, (j, want_logits, int(a[2]))
            if want_logits:
                assert float(lg[2, 5]) == float(lg[2, j]) and abs(float(lg[2, 5]) - 32.0) < 1e-4
        keep = [b for b in range(B) if b != 2]
        assert a.cpu()[keep].tolist() == _cos64(x2, w2).argmax(1)[keep].tolist()


@pytest.mark.parametrize("s,m,easy", [(16.0, 0.3, True), (30.0, 0.5, False), (24.0, 0.5, False)])
@pytest.mark.parametrize("B,C,D", [(70, 130, 36), (5, 129, 512)])
def test_arcmargin_eval_blocks_tail_and_clamped_labels(B, C, D, s, m, easy):
    """Against `oracle.face_oracle.arcmargin_eval` in float32 at 2e-4 (the golden test's tolerance), two row blocks / a second
    column block of 1-2 columns / a partial K step, labels 0 and C - 1.  Row 1 is its label's weight row (cos = 1), row 2 its
    negative (cos = -1): there the float32 clamp constant 1 - 1e-7 rounds to 1 - 1.19e-7, which moves acos by at most 4.2e-5,
    times s <= 24 = 1e-3, so those two label entries are held to 2e-3."""
    x = synth.randn(1200 + D, (B, D), "x")
    w = synth.randn(1201 + D, (C, D), "w")
    lab = torch.from_numpy(np.random.default_rng(1202).integers(0, C, B)).long()
    lab[0], lab[1], lab[2], lab[B - 1] = 0, C // 2, 7, C - 1
    x[1], x[2] = w[lab[1]], -w[lab[2]]
    out, mm = ops.arcmargin_eval(x.to(DEV), w.to(DEV), lab.to(DEV), s, m, easy, want_minmax=True)
    out = out.cpu()
    ref = fo.arcmargin_eval(w, x, lab, s, m, easy)
    atol = torch.full_like(ref, 2e-4)
    atol[1, lab[1]] = atol[2, lab[2]] = 2e-3
    err = (out - ref).abs()
    assert bool((err <= atol).all()), (float(err.max()), float(err[1, lab[1]]), float(err[2, lab[2]]))
    cos = _cos64(x, w)
    assert abs(float(mm[0]) - float(cos.max())) < 1e-5 and abs(float(mm[1]) - float(cos.min())) < 1e-5
    out2, none = ops.arcmargin_eval(x.to(DEV), w.to(DEV), lab.to(DEV), s, m, easy)
    assert none is None and torch.equal(out2.cpu(), out)


# --------------------------------------------------------------------------------------------------------------------------------
# one-wave-per-row kernels
# --------------------------------------------------------------------------------------------------------------------------------
# C below, at and above one wave (63, 64, 65), 1, 2 and 1000 (16 columns per lane); B = 1, 5 (two rows of a workgroup idle),
# 260 (65 workgroups)
@pytest.mark.parametrize("B", [1, 5, 260])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 1000])
def test_softmax_argmax_widths(C, B):
    logits = synth.randn(1300 + C, (B, C), "l") * 3
    want = {}
    if B >= 5:
        logits[1] = torch.where(torch.arange(C) % 2 == 0, 80.0, -80.0)      # exp(-160) underflows, exp(0) does not overflow
        want[1] = 0
        if C > 64:                                    # a tie inside one lane (columns 0 and 64): the first index wins
            logits[2, 0] = logits[2, 64] = logits[2].max() + 1.0
            want[2] = 0
        if C > 65:                                    # a tie across lanes 63 and 1 (columns 63 and 65)
            logits[3, 63] = logits[3, 65] = logits[3].max() + 1.0
            want[3] = 63
    probs, pred = ops.softmax_argmax(logits.to(DEV))
    ref = F.softmax(logits.double(), dim=1)
    assert torch.allclose(probs.cpu().double(), ref, atol=1e-6), float((probs.cpu().double() - ref).abs().max())
    pred = pred.cpu()
    for b in range(B):
        row = logits[b]
        assert int(pred[b]) == int((row == row.max()).nonzero()[0]), b
    for b, c in want.items():
        assert int(pred[b]) == c
    none, pred2 = ops.softmax_argmax(logits.to(DEV), want_probs=False)
    assert none is None and torch.equal(pred2.cpu(), pred)


@pytest.mark.parametrize("B", [1, 259])
@pytest.mark.parametrize("D", [1, 4, 63, 64, 65, 1000])
def test_pairwise_distance_and_l2_normalize_widths(D, B):
    a, b = synth.randn(1400 + D, (B, D), "a"), synth.randn(1401 + D, (B, D), "b")
    b[0] = a[0]                                       # identical rows: sqrt(D) * 1e-6, the eps of F.pairwise_distance
    if B > 1:
        a[1] = 0.0                                    # a zero row
    dref = torch.sqrt(((a.double() - b.double() + 1e-6) ** 2).sum(1))
    thr = float(dref.median())
    d, same = ops.pairwise_distance(a.to(DEV), b.to(DEV), thr)
    d, same = d.cpu(), same.cpu()
    assert torch.allclose(d[1:].double(), dref[1:], rtol=1e-6)
    assert abs(float(d[0]) - math.sqrt(D) * 1e-6) <= 1e-5 * math.sqrt(D) * 1e-6
    assert same.tolist() == (d < thr).int().tolist()
    clear = (dref - thr).abs() > 1e-5 * thr
    assert same[clear].tolist() == (dref < thr).int()[clear].tolist()
    d2, none = ops.pairwise_distance(a.to(DEV), b.to(DEV))
    assert none is None and torch.equal(d2.cpu(), d)
    n = ops.l2_normalize(a.to(DEV), 1e-12).cpu()
    assert torch.allclose(n.double(), F.normalize(a.double(), p=2, dim=1, eps=1e-12), atol=1e-6)
    if B > 1:
        assert torch.equal(n[1], torch.zeros(D))      # x / max(0, eps) = 0, no NaN


# --------------------------------------------------------------------------------------------------------------------------------
# grid-stride loops
# --------------------------------------------------------------------------------------------------------------------------------
def test_cast_grid_stride_loop():
    """n = 8192 * 256 + 1000: more elements than the casts' grid has threads, so their loops iterate, with a ragged last trip."""
    n = 8192 * 256 + 1000
    t = synth.randn(1500, (n,), "c")
    h = ops.cast_from_f32(t.to(DEV), torch.float16).cpu()
    assert torch.equal(h, t.to(torch.float16))
    assert torch.equal(ops.cast_to_f32(h.to(DEV)).cpu(), h.float())


def test_maxpool_grid_stride_loop():
    """10 x 242 x 242 x 64, k = 2, s = 1, p = 0: 4.65 M 8-channel output items against a grid capped at 16 384 workgroups
    (4.19 M threads).  Exact: a maximum of representable values."""
    x = synth.randn(1501, (10, 242, 242, 64), "x").to(torch.bfloat16)
    y = ops.maxpool(x.to(DEV), 2, 1, 0).cpu()
    ref = torch.maximum(torch.maximum(x[:, :-1, :-1], x[:, 1:, :-1]), torch.maximum(x[:, :-1, 1:], x[:, 1:, 1:]))
    assert y.shape == ref.shape and torch.equal(y, ref)
