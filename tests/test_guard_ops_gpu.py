"""GPU: the layout / pool / cast kernels, the heads, the matching entry points, the transformer kernels and the trackers between
guard bands (`guard.py`).  Every case follows the two-fill rule: unguarded, then with every operand, output and workspace the
wrapper allocates between bands of 0xFF.. and of 0x5A..; `check()` passes and all returned tensors hold the same bits three
times.  The layout / pool / cast cases are also compared with a float64 CPU reference (`test_kernels_gpu.py::test_pools`'
tolerances); what the other kernels compute is tested in their own files.  One positive control at the end.

Workspace fields (first write / first read, read from `head_match.hip`, `match_device.h`, `conv_pp.hip`; each operation's fields
are laid out by one function of `head_match.hip` - `top1_ws`, `topk_ws`, `verify_ws`, `radius_ws` - that its `*_workspace_bytes` shares):
  cosine_logits   keys u64 [B]           `fill_u64_kernel` (0) before the GEMM / atomicMax in the GEMM, then `argkey_finalize_kernel`
                  inv_a [B], inv_w [C]   `row_stats_kernel` x 2 / the GEMM's epilogue
  arcmargin_eval  mm u32 [2]             `minmax_init_kernel` / atomicMax, atomicMin in the GEMM (integers), `minmax_finalize_kernel`
                  inv_a [B], inv_w [C]   `row_stats_kernel` x 2 / the GEMM's epilogue
  match_top1      recs [4 ceil(G/128)][B]   the MODE_DIST epilogue, one record per (workgroup column, wave, b < B): every slot, rows
                                            past G as never-candidates (idx -1) / `match_finalize_rec_kernel`
                  stat_a [B][2], stat_w [G][2]   `row_stats_kernel` x 2 / the GEMM's epilogue
  match_top1_packed  recs [Gpad/64][B]   `match_epilogue_records` (every 64-row slot of every N tile, b < M) / the finalize kernel
                  stat_a [B][4], split [B][3D]   `match_row_prep_kernel` / the GEMM (loads of row min(b, M - 1))
  match_topk      (scan: no workspace field is used; k = 1 without labels is match_top1's)
  match_topk_packed  recs MatchRecK [Gpad/64][B], stat_a, split   as match_top1_packed (`match_epilogue_topr`, pad[] zeroed)
  verify_counts   hist u64 [2][T+1], misc u64 [2], tab f32 [3T]   `verify_prep_kernel`, first launch / scan or GEMM, finalize
                  stat_a [P][4], split [P][3D]   `match_row_prep_kernel` / the GEMM (packed path only)
  match_radius    misc u64 [1] (rescored, when the caller passes none)   `radius_prep_kernel` / atomicAdd in the GEMM epilogue
                  stat_a, split          as verify_counts
  The record index fields (`MatchRec.idx`, `MatchRecK.idx[]`) are what a finalize kernel turns into a gallery address: each is
  written by the epilogue for every record the finalize kernel reads.  No field is read before it is written.
Run-to-run bits: the only atomics are on integers (arg-max keys, min / max keys, histogram bins, pair counts and slots), so no
kernel here needs the reference-bound fallback; `match_radius` pairs are compared after the wrapper's own (i, j) sort.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import attention_cases as ac  # noqa: E402
import conv_cases as cc  # noqa: E402
import fuse_cases as fc  # noqa: E402
import guard  # noqa: E402
import track_cases as tc  # noqa: E402
from frmap_amd import _lib, ops, synth  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _tol(dtype):      # test_kernels_gpu.py's: one rounding of the output to the storage dtype + fp32 accumulation noise
    return (2e-3, 2e-3) if dtype == torch.float16 else (1.6e-2, 1.6e-2)


def _rule(run, what):
    return guard.two_fills(run, [ops], what=what)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# --------------------------------------------------------------------------------------------------------------------------------
# layout, pool, cast
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,H,W", [(2, 6, 5), (2, 7, 5)], ids=["even-HW-float2", "odd-HW-scalar"])
def test_pack_input(B, H, W, dtype):
    x = synth.randn(11, (B, 3, H, W), "g.x")
    y, = _rule(lambda place: ops.pack_input(place(x), dtype), "pack_input")
    assert torch.equal(y[..., :3], _nhwc(x).to(dtype)) and float(y[..., 3].float().abs().max()) == 0.0


@pytest.mark.parametrize("nchw,nhwc4", [(True, None), (False, torch.float16), (True, torch.bfloat16)], ids=["nchw", "nhwc4", "both"])
def test_normalize_u8(nchw, nhwc4):
    g = torch.Generator().manual_seed(12)
    img = torch.randint(0, 256, (2, 7, 5, 3), generator=g).to(torch.uint8)
    o1, o2 = _rule(lambda place: ops.normalize_u8(place(img), MEAN, STD, want_nchw=nchw, nhwc4_dtype=nhwc4), "normalize_u8")
    ref = (img.permute(0, 3, 1, 2).double() / 255 - torch.tensor(MEAN).double().view(1, 3, 1, 1)) / torch.tensor(STD).double().view(1, 3, 1, 1)
    assert (o1 is None) == (not nchw) and (o2 is None) == (nhwc4 is None)
    if nchw:
        assert torch.allclose(o1.double(), ref, atol=1e-6, rtol=1e-6)
    if nhwc4 is not None:      # the fp32 value rounded once: u |ref| plus the fp32 tolerance above
        r = _nhwc(ref)
        assert bool(((o2[..., :3].double() - r).abs() <= cc.UNIT[nhwc4] * r.abs() + 2e-6).all())
        assert float(o2[..., 3].float().abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (2, 2, 0)], ids=["3-2-1", "2-2-0-drops-last-row-col"])
def test_maxpool(k, s, p, dtype):
    x = synth.randn(13, (3, 8, 7, 5), "g.x").to(dtype)
    y, = _rule(lambda place: ops.maxpool(place(_nhwc(x)), k, s, p), "maxpool")
    assert torch.equal(y.permute(0, 3, 1, 2).double(), cc.window_max(x.double(), k, s, p))       # exact: a max of representable values


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("H,W", [(1, 1), (7, 7), (5, 13)], ids=["HW1", "HW49", "HW65"])
def test_avgpool_global(H, W, dtype):
    x = synth.randn(14, (3, 72, H, W), "g.x").to(dtype)
    y, = _rule(lambda place: ops.avgpool_global(place(_nhwc(x))), "avgpool_global")
    assert torch.allclose(y.double(), x.double().mean(dim=(2, 3)), atol=1e-5)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("H,W", [(14, 14), (5, 3)], ids=["14-to-6", "5x3-to-6x6-windows-repeat"])
def test_avgpool_adaptive(H, W, dtype):
    x = synth.randn(15, (2, 24, H, W), "g.x").to(dtype)
    y, = _rule(lambda place: ops.avgpool_adaptive(place(_nhwc(x)), 6, 6), "avgpool_adaptive")
    atol, rtol = _tol(dtype)
    assert torch.allclose(y.permute(0, 3, 1, 2).double(), F.adaptive_avg_pool2d(x.double(), (6, 6)), atol=atol, rtol=rtol)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [1, 255, 257])
def test_casts(n, dtype):
    t = synth.randn(16, (n,), "g.c")
    lo, = _rule(lambda place: ops.cast_from_f32(place(t), dtype), "cast_from_f32")
    assert torch.equal(lo, t.to(dtype))
    hi, = _rule(lambda place: ops.cast_to_f32(place(t.to(dtype))), "cast_to_f32")
    assert torch.equal(hi, t.to(dtype).float())


# --------------------------------------------------------------------------------------------------------------------------------
# heads
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,N", [(1, 4, 1), (65, 128, 36), (3, 512, 129)])
def test_linear_f32_and_l2_normalize(B, K, N):
    x, w = synth.randn(21, (B, K), "g.x"), synth.randn(22, (N, K), "g.w") / K ** 0.5
    sc, sh = synth.randn(23, (N,), "g.s").abs() + 0.5, synth.randn(24, (N,), "g.h")
    _rule(lambda place: ops.linear_f32(place(x), place(w), place(sc), place(sh), True), "linear_f32")
    _rule(lambda place: ops.linear_f32(place(x), place(w)), "linear_f32 plain")
    _rule(lambda place: ops.l2_normalize(place(x)), "l2_normalize")


@pytest.mark.parametrize("B,C", [(1, 1), (5, 36), (65, 63), (3, 65)])
def test_softmax_argmax_and_pairwise_distance(B, C):
    logits = synth.randn(25, (B, C), "g.l") * 3
    _rule(lambda place: ops.softmax_argmax(place(logits)), "softmax_argmax")
    _rule(lambda place: ops.softmax_argmax(place(logits), want_probs=False), "softmax_argmax pred only")
    a, b = synth.randn(26, (B, C), "g.a"), synth.randn(27, (B, C), "g.b")
    _rule(lambda place: ops.pairwise_distance(place(a), place(b), 1.0 * C ** 0.5), "pairwise_distance")
    _rule(lambda place: ops.pairwise_distance(place(a), place(b)), "pairwise_distance no thresh")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,HW,K,N", [(1, 1, 8, 256), (3, 49, 512, 512), (65, 4, 128, 256)])     # (the kernel takes N = 256 or 512)
def test_gap_linear_norm(B, HW, K, N, dtype):
    fmap = synth.randn(28, (B, HW, 1, K), "g.m").to(dtype)
    wt = synth.randn(29, (K, N), "g.w") / K ** 0.5
    sc, sh = synth.randn(30, (N,), "g.s").abs() + 0.5, synth.randn(31, (N,), "g.h")
    _rule(lambda place: ops.gap_linear_norm(place(fmap), place(wt), place(sc), place(sh), want_pre=True), "gap_linear_norm")
    _rule(lambda place: ops.gap_linear_norm(place(fmap), place(wt), None, place(sh), relu=True), "gap_linear_norm no scale")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,HW,C,G", [(1, 1, 8, 1), (3, 49, 512, 36), (65, 4, 64, 64)])
def test_gap_norm_match(B, HW, C, G, dtype):
    fmap = synth.randn(32, (B, HW, 1, C), "g.m").to(dtype)
    gal = synth.unit_rows(33, G, C, "g.gal")
    _rule(lambda place: ops.gap_norm_match(place(fmap), place(gal), 1.2, normalize=True, want_emb=True, packed=True), "gap_norm_match")
    _rule(lambda place: ops.gap_norm_match(place(fmap), place(gal)), "gap_norm_match plain")


@pytest.mark.parametrize("B,C,D", [(1, 1, 4), (5, 36, 64), (65, 129, 128)])
def test_cosine_logits_and_arcmargin(B, C, D):
    x, w = synth.randn(34, (B, D), "g.x"), synth.randn(35, (C, D), "g.w")
    lab = torch.arange(B, dtype=torch.int64) % C
    _rule(lambda place: ops.cosine_logits(place(x), place(w), s=32.0), "cosine_logits")
    _rule(lambda place: ops.cosine_logits(place(x), place(w), want_logits=False), "cosine_logits argmax only")
    _rule(lambda place: ops.arcmargin_eval(place(x), place(w), place(lab), 30.0, 0.5, want_minmax=True), "arcmargin_eval")
    _rule(lambda place: ops.arcmargin_eval(place(x), place(w), place(lab), 16.0, 0.3, easy_margin=True), "arcmargin_eval easy")


# --------------------------------------------------------------------------------------------------------------------------------
# matching: the 64-row scan (G = 7), the fp32 GEMM (G = 65) and the packed MFMA path (G = 600, D % 32 == 0, pack buffers guarded)
# --------------------------------------------------------------------------------------------------------------------------------
MATCH_D = 64
MATCH_SHAPES = [(1, 7, False), (1, 65, False), (65, 65, False), (1, 600, True), (65, 600, True)]
MATCH_IDS = ["B1-G7", "B1-G65", "B65-G65", "B1-G600-packed", "B65-G600-packed"]


def _gallery_and_probes(B, G, seed):
    gal = synth.unit_rows(seed, G, MATCH_D, "g.gal")
    pr = synth.unit_rows(seed + 1, B, MATCH_D, "g.pr")
    pr[0] = gal[G // 2]                      # an exact hit
    if G > 3:
        gal[G - 1] = gal[1]                  # duplicate rows: ties inside the records
    return gal, pr


def _prepared(gallery_dev, packed):
    """`match_prepare` under the patched `ops`: its pack and statistics buffers come from the guard at exactly the bytes it asks for."""
    if not packed:
        return None
    assert ops.wants_pack(int(gallery_dev.shape[0]), int(gallery_dev.shape[1]))
    return ops.match_prepare(gallery_dev)


@pytest.mark.parametrize("B,G,packed", MATCH_SHAPES, ids=MATCH_IDS)
def test_match_top1(B, G, packed):
    gal, pr = _gallery_and_probes(B, G, 41)

    def run(place):
        g = place(gal)
        return ops.match_top1(place(pr), g, 0.9, packed=True, prepared=_prepared(g, packed))
    idx = _rule(run, "match_top1")[0]
    assert int(idx[0]) == G // 2


def test_match_top1_empty_gallery():
    pr = synth.unit_rows(42, 3, MATCH_D, "g.pr")
    idx, dist = _rule(lambda place: ops.match_top1(place(pr), None), "match_top1 G = 0")
    assert idx.tolist() == [-1] * 3 and bool(torch.isinf(dist).all())


@pytest.mark.parametrize("k,by_label", [(1, False), (5, False), (5, True), (64, True)])
@pytest.mark.parametrize("B,G,packed", MATCH_SHAPES, ids=MATCH_IDS)
def test_match_topk(B, G, packed, k, by_label):
    gal, pr = _gallery_and_probes(B, G, 43)
    labels = (torch.arange(G, dtype=torch.int32) * 7) % max(G // 3, 1)

    def run(place):
        g = place(gal)
        return ops.match_topk(place(pr), g, k, place(labels) if by_label else None, prepared=_prepared(g, packed))
    idx = _rule(run, "match_topk")[0]
    assert int(idx[0, 0]) == G // 2


@pytest.mark.parametrize("mode", ["self", "block", "cross"])
@pytest.mark.parametrize("P,Q,packed", MATCH_SHAPES, ids=MATCH_IDS)
def test_verify_counts(P, Q, packed, mode):
    b, a = _gallery_and_probes(P, Q, 45)
    lb = (torch.arange(Q, dtype=torch.int32) * 5) % 9
    la = (torch.arange(P, dtype=torch.int32) * 3) % 9
    thr = torch.tensor([1e-4, 0.5, 1.0, 1.3, 1.5, 2.5], dtype=torch.float32)
    row0 = min(2, Q - P)                     # (every shape of the table has P <= Q)

    def run(place):
        t = place(thr)
        bd = place(b)
        if mode == "self":       # over B itself
            return ops.verify_counts(bd, place(lb), t, prepared=_prepared(bd, packed), return_rescored=True)
        if mode == "block":
            ad, lad = place(b[row0:row0 + P].clone()), place(lb[row0:row0 + P].clone())
            return ops.verify_counts(ad, lad, t, bd, place(lb), a_row0=row0, prepared=_prepared(bd, packed), return_rescored=True)
        return ops.verify_counts(place(a), place(la), t, bd, place(lb), prepared=_prepared(bd, packed), return_rescored=True)
    counts = _rule(run, "verify_counts " + mode)[0]
    assert counts.shape == (2, 6) and bool((counts[:, 1:] >= counts[:, :-1]).all())


@pytest.mark.parametrize("which", ["all", "same"])
@pytest.mark.parametrize("P,Q,packed", MATCH_SHAPES, ids=MATCH_IDS)
def test_match_radius(P, Q, packed, which):
    b, a = _gallery_and_probes(P, Q, 47)
    lb = (torch.arange(Q, dtype=torch.int32) * 5) % 9
    la = lb[(torch.arange(P) * 3) % Q].clone()

    def run(place):
        bd = place(b)
        return ops.match_radius(place(a), 1.35, bd, labels_a=place(la), labels_b=place(lb), which=which, prepared=_prepared(bd, packed))
    pairs, dists, counts = _rule(run, "match_radius")                      # (sorted by (i, j) in the wrapper: the canonical order)
    assert pairs.shape[0] == dists.shape[0] == int(counts.sum()) and (which != "all" or pairs.shape[0] > 0)


# --------------------------------------------------------------------------------------------------------------------------------
# transformer kernels (the existing guard tests of `mha_tokens` and `cnn_attention` stay in test_attention_gpu.py)
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,L,D", [(2, 5, 64), (5, 49, 512), (1, 65, 192)])
def test_layernorm_kernels(B, L, D, dtype):
    x = synth.randn(51, (B, L, D), "g.x").to(dtype)
    pos = synth.randn(52, (L, D), "g.p") * 0.1
    g1, b1 = synth.randn(53, (D,), "g.g").abs() + 0.5, synth.randn(54, (D,), "g.b") * 0.1
    _rule(lambda place: ops.add_pos_layernorm(place(x), place(pos), place(g1), place(b1), want_sum=True), "add_pos_layernorm sum")
    _rule(lambda place: ops.add_pos_layernorm(place(x), None, place(g1), place(b1)), "add_pos_layernorm")
    _rule(lambda place: ops.mean_layernorm(place(x), place(g1), place(b1)), "mean_layernorm")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,L,H", [(1, 1, 1), (3, 49, 2), (2, 63, 4), (2, 64, 4)])
def test_mha_tokens(B, L, H, dtype):
    qkv = ac.mha_inputs("peaked", 55 + L, B, L, H, dtype)
    _rule(lambda place: ops.mha_tokens(place(qkv), H), "mha_tokens")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("H,W,C,Cq,KS,want_map,want_pool", [(1, 1, 256, 8, 1, True, True), (7, 7, 512, 64, 7, True, True),
                                                            (5, 11, 512, 8, 3, True, False), (7, 9, 256, 128, 5, False, True)])
def test_cnn_attention(H, W, C, Cq, KS, want_map, want_pool, dtype):
    ops_in = ac.cnn_attention_inputs(56 + H * W, 3, H, W, C, Cq, KS, dtype)
    _rule(lambda place: ops.cnn_attention(*[place(t) for t in ops_in], Cq, want_map=want_map, want_pool=want_pool), "cnn_attention")


# --------------------------------------------------------------------------------------------------------------------------------
# trackers: the state comes from `ops.track_state` / `ops.track_fuse_state` (a `torch.zeros` of the patched module: guarded at
# exactly `*_state_bytes`) and is returned with the outputs
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,M", [tc.GRID[0], (2, 65)])
def test_track_step(S, M):
    scene = tc.moving_scene(S, M, 3, 100 * S + M)
    hw = torch.tensor([[240, 320]] * S, dtype=torch.int32)
    steps = [tc.pad_step(frame, M) for frame in scene]

    def run(place):
        state = ops.track_state(S, M, DEV)
        out = []
        for boxes, probs, counts in steps:
            out += list(ops.track_step(state, place(torch.from_numpy(boxes)), place(torch.from_numpy(probs)),
                                       place(torch.from_numpy(counts)), place(hw)))
        return out + [state]
    _rule(run, "track_step")


@pytest.mark.parametrize("S,M,D", [fc.GRID[0] + (fc.D_GRID[0],), (5, 65, 65)])
def test_track_fuse(S, M, D):
    steps = fc.random_steps(S, M, D, 3, 1000 * S + 10 * M + D)

    def run(place):
        state = ops.track_fuse_state(S, M, D, DEV)
        out = []
        for ids, counts, emb, rows in steps:
            t = lambda a, dt: place(torch.from_numpy(np.ascontiguousarray(a, dtype=dt)))
            out += list(ops.track_fuse(state, t(ids, np.int32), t(counts, np.int32), t(emb, np.float32), t(rows, np.int32).view(-1, 2), 0.9))
        return out + [state]
    _rule(run, "track_fuse")


# --------------------------------------------------------------------------------------------------------------------------------
# the one positive control: a deliberately wrong call whose every access stays inside two guarded allocations
# --------------------------------------------------------------------------------------------------------------------------------
def test_positive_control_one_element_too_many():
    """`frmap_cast_from_f32` told n + 1 on a guarded input and output of n elements: it reads the first float of the input's rear
    band (0x5A5A5A5A = 1.5e16, +inf in fp16) and stores 0x7C00 over the first two bytes of the output's rear band.  `check()`
    must name the output and offset 0 of its rear band.  (fp16 under fill 0x5A: a bf16 result, 0x5A5A, or a NaN result under 0xFF
    could equal the fill.)"""
    n = 255
    g = guard.Guard(0x5A)
    x = g.place(synth.randn(61, (n,), "g.c"))
    out = g.empty((n,), torch.float16)
    g.check()
    assert _lib.load().frmap_cast_from_f32(x.data_ptr(), out.data_ptr(), n + 1, ops.dt_code(torch.float16),
                                           torch.cuda.current_stream().cuda_stream) == 0
    with pytest.raises(guard.GuardError) as e:
        g.check()
    assert (e.value.order, e.value.region, e.value.offset) == (1, "rear", 0), str(e.value)
    assert "allocation #1" in str(e.value) and "[255] float16" in str(e.value) and "offset 0" in str(e.value)
    assert torch.equal(out.cpu(), x.cpu().to(torch.float16))
