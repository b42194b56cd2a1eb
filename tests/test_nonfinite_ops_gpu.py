"""GPU: one non-finite element into every pooling, cast, head, token and attention kernel between the input and the embedding;
the rules of `poison.py` on what comes out ("Non-finite values").

An op is a table row: its per-image operand(s), how it is launched, its float64 reference (the ones the older tests of the same
op use) and the rule those tests hold a finite element to.  The driver runs it clean, then once per position of
`poison.positions` in every per-image operand, the kind (NaN, +inf, -inf) rotating with position and operand, and hands every
floating output to `poison.compare`: class of every element as in the float64 reference on the poisoned operands, bit identity
wherever that reference is unchanged, every other row / image bit for bit.  The footprint is where the reference turns NaN under
a NaN at the same place.  Integer outputs (an arg-max, a match index) have no class: they are held to rule 3 (no other row
changes) and, where the op documents a sentinel for a probe it declines, to that sentinel.  `arcmargin_eval` is left out: it keeps
the reference's own NaN / Inf -> 0 rule.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import attention_cases as ac  # noqa: E402
import conv_cases as cc  # noqa: E402
import poison  # noqa: E402
from frmap_amd import ops, synth  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]


def _close(atol, rtol=0.0, zero_exact=True):
    """The older tests' `allclose(atol, rtol)` as a `finite_ok`; a reference that is exactly 0 (relu(-inf), x / inf) must be 0."""
    def ok(got, want, mask):
        good = (got.double() - want).abs() <= atol + rtol * want.abs()
        if zero_exact:
            good = torch.where(want == 0, got.double() == 0, good)
        return ~mask | good
    return ok


def _drive(name, operands, poisonable, run, ref, rules, int_outputs=(), kinds=poison.KINDS, rot=0, every_kind=False, extra=None):
    """operands: dict of CPU tensors; poisonable: the keys whose axis 0 is the image; run(operands) -> tuple of CPU outputs;
    ref(operands) -> tuple of float64 references of the floating outputs (the first len(rules) outputs); rules: a `finite_ok` or
    None (exact) per floating output, or a function of the poisoned operands that returns that list; int_outputs: positions in
    run()'s tuple of integer outputs held to rule 3 alone.  every_kind: all of `kinds` at every position (default: the kind
    rotates with the position).  extra: {operand: [(name, index)]} positions beyond `poison.positions`.
    Returns [(operand, index, kind, outputs)] for checks of the caller's own."""
    got_c, ref_c = run(operands), ref(operands)
    for r in ref_c:
        assert bool(torch.isfinite(r).all()), name
    seen, ri = [], rot
    for key in poisonable:
        where = poison.positions(operands[key].shape) + list((extra or {}).get(key, []))
        todo = [(p, k) for p in where for k in kinds] if every_kind else [(p, kinds[(ri + i) % len(kinds)]) for i, p in enumerate(where)]
        ri += len(where)
        for (pname, idx), kind in todo:
            what = "%s: %s at %s %s of %s" % (name, kind, pname, list(idx), key)
            op_ = dict(operands)
            op_[key] = poison.poisoned(operands[key], idx, poison.poison_value(kind))
            op_n = dict(operands)
            op_n[key] = poison.poisoned(operands[key], idx, math.nan)
            got_p, ref_p, ref_n = run(op_), ref(op_), ref(op_n)
            for k, rule in enumerate(rules(op_) if callable(rules) else rules):
                poison.compare(got_c[k], got_p[k], ref_c[k], ref_p[k], poison.nan_footprint(ref_n[k]), image=idx[0], finite_ok=rule,
                               what="%s, output %d" % (what, k))
            for k in int_outputs:
                keep = [b for b in range(got_c[k].shape[0]) if b != idx[0]]
                assert torch.equal(got_c[k][keep], got_p[k][keep]), "%s: integer output %d of another row changed" % (what, k)
            seen.append((key, idx, kind, got_p))
    return seen


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# --------------------------------------------------------------------------------------------------------------------------------
# layout_pool.hip
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (2, 2, 0)])
def test_maxpool(k, s, p, dtype):
    """2 x 16 x 7 x 5.  Exact: a maximum of representable values; a window that drops a -inf returns its other members' maximum."""
    o = {"x": synth.randn(2100 + k, (2, 16, 7, 5), "x").to(dtype)}
    _drive("maxpool(%d,%d,%d)" % (k, s, p), o, ["x"], lambda q: (_nchw(ops.maxpool(_nhwc(q["x"]).to(DEV), k, s, p).cpu()),),
           lambda q: (cc.window_max(q["x"].double(), k, s, p),), [None], rot=k)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_avgpools(dtype):
    """avgpool_global (fp32 out) and avgpool_adaptive 7x5 -> 3x3 (storage out) on 3 x 16 x 7 x 5."""
    o = {"x": synth.randn(2110, (3, 16, 7, 5), "x").to(dtype)}
    _drive("avgpool_global", o, ["x"], lambda q: (ops.avgpool_global(_nhwc(q["x"]).to(DEV)).cpu(),),
           lambda q: (q["x"].double().mean(dim=(2, 3)),), [_close(1e-6, 1e-6)])
    _drive("avgpool_adaptive", o, ["x"], lambda q: (_nchw(ops.avgpool_adaptive(_nhwc(q["x"]).to(DEV), 3, 3).cpu()),),
           lambda q: (F.adaptive_avg_pool2d(q["x"].double(), (3, 3)),), [_close(0.0, 2 * cc.UNIT[dtype])], rot=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_pack_input_and_casts(dtype):
    """`pack_input` and the casts keep NaN and the infinities and round an fp32 value past the storage maximum to inf."""
    o = {"x": synth.randn(2120, (3, 3, 6, 5), "x")}

    def ref_pack(q):
        r = torch.zeros((q["x"].shape[0], 4) + tuple(q["x"].shape[2:]), dtype=torch.float64)
        r[:, :3] = q["x"].to(dtype).double()
        return (r,)
    _drive("pack_input", o, ["x"], lambda q: (_nchw(ops.pack_input(q["x"].to(DEV), dtype).cpu()),), ref_pack, [None])
    _drive("cast_from_f32", o, ["x"], lambda q: (ops.cast_from_f32(q["x"].to(DEV), dtype).cpu(),), lambda q: (q["x"].to(dtype).double(),), [None], rot=1)
    h = {"x": o["x"].to(dtype)}
    _drive("cast_to_f32", h, ["x"], lambda q: (ops.cast_to_f32(q["x"].to(DEV)).cpu(),), lambda q: (q["x"].double(),), [None], rot=2)
    if dtype == torch.float16:             # overflow: 2e5 and -2e5 are more than 2 x 65504 away from zero: +-inf in fp16 whatever the rounding
        for v, cls in ((2.0e5, poison.PINF), (-2.0e5, poison.NINF)):
            x = poison.poisoned(o["x"], (1, 2, 3, 4), v)
            poison.overflow_ok(x.double(), "cast")
            for y in (ops.cast_from_f32(x.to(DEV), dtype).cpu(), _nchw(ops.pack_input(x.to(DEV), dtype).cpu())[:, :3]):
                assert int(poison.classify(y)[1, 2, 3, 4]) == cls
                y[1, 2, 3, 4] = o["x"][1, 2, 3, 4].to(dtype)
                assert torch.equal(y, o["x"].to(dtype))


# --------------------------------------------------------------------------------------------------------------------------------
# head_match.hip
# --------------------------------------------------------------------------------------------------------------------------------
def test_linear_f32_relu():
    """B = 5, K = 36 (a partial K step), N = 129; relu((x w^T) scale + shift).  No weight and no scale is zero."""
    B, K, N = 5, 36, 129
    o = {"x": synth.randn(2130, (B, K), "x"), "w": synth.randn(2131, (N, K), "w") / math.sqrt(K),
         "sc": synth.randn(2132, (N,), "s").abs() + 0.5, "sh": synth.randn(2133, (N,), "h")}
    poison.assert_no_zero(o["w"])
    _drive("linear_f32+relu", o, ["x"], lambda q: (ops.linear_f32(q["x"].to(DEV), q["w"].to(DEV), q["sc"].to(DEV), q["sh"].to(DEV), True).cpu(),),
           lambda q: (((q["x"].double() @ q["w"].double().t()) * q["sc"].double() + q["sh"].double()).clamp_min(0),), [_close(2e-5, 2e-5)])


@pytest.mark.parametrize("D", [4, 65, 1000])
def test_l2_normalize(D):
    """A row with one NaN is all NaN, as in `F.normalize`; a row with one infinity is 0 except for NaN at the infinity."""
    o = {"x": synth.randn(2140 + D, (5, D), "x")}
    seen = _drive("l2_normalize", o, ["x"], lambda q: (ops.l2_normalize(q["x"].to(DEV), 1e-12).cpu(),),
                  lambda q: (F.normalize(q["x"].double(), p=2, dim=1, eps=1e-12),), [_close(1e-6)])
    for key, idx, kind, (y,) in seen:
        if kind == "nan":
            assert bool(torch.isnan(y[idx[0]]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("relu", [False, True], ids=["bn", "relu"])
def test_gap_linear_norm(relu, dtype):
    """9 x 5 x 5 x 192 -> 256 (`test_gap_linear_norm_idle_lanes_and_tiny_k`'s shape): pre and emb."""
    B, H, W, K, N = 9, 5, 5, 192, 256
    o = {"m": torch.relu(synth.randn(2150, (B, K, H, W), "m")).to(dtype), "w": synth.randn(2151, (N, K), "w") * (1.0 / math.sqrt(K)),
         "sc": 1.0 + 0.1 * synth.randn(2152, (N,), "s"), "sh": 0.1 * synth.randn(2153, (N,), "b")}
    poison.assert_no_zero(o["w"])

    def run(q):
        emb, pre = ops.gap_linear_norm(_nhwc(q["m"]).to(DEV), q["w"].t().contiguous().to(DEV), None if relu else q["sc"].to(DEV), q["sh"].to(DEV),
                                       1e-12, want_pre=True, relu=relu)
        return pre.cpu(), emb.cpu()

    def ref(q):
        pre = q["m"].double().mean(dim=(2, 3)) @ q["w"].double().t()
        pre = (pre + q["sh"].double()).clamp_min(0) if relu else pre * q["sc"].double() + q["sh"].double()
        return pre, F.normalize(pre, p=2, dim=1, eps=1e-12)
    _drive("gap_linear_norm", o, ["m"], run, ref, [_close(2e-5, 2e-5), _close(2e-6, 2e-5)], rot=int(relu))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
def test_gap_norm_match_declines_a_poisoned_probe(normalize, dtype):
    """5 x 49 x 512 against 36 rows.  The embedding follows the rules; a probe whose embedding is not finite is declined with the
    matcher's sentinel (index -1, distance +inf, id -1: `test_nan_and_empty_rows_never_win`), every other face keeps its answer."""
    B, HW, C, G = 5, 49, 512, 36
    o = {"m": (torch.relu(synth.randn(2160, (B, C, 7, 7), "map") + 0.3) * 0.5).to(dtype), "g": synth.unit_rows(2161, G, C)}

    def run(q):
        idx, dist, ids, _, emb = ops.gap_norm_match(_nhwc(q["m"]).to(DEV), q["g"].to(DEV), 1e9, normalize=normalize, want_emb=True)
        return emb.cpu(), dist.cpu(), idx.cpu(), ids.cpu()

    def ref(q):
        e = q["m"].double().mean(dim=(2, 3))
        return ((e / e.norm(dim=1, keepdim=True).clamp_min(1e-12)) if normalize else e,)
    clean = run(o)
    seen = _drive("gap_norm_match", o, ["m"], run, ref, [_close(1e-6)], int_outputs=(2, 3), rot=int(normalize))
    for key, idx, kind, (emb, dist, mi, ids) in seen:
        b = idx[0]
        keep = [i for i in range(B) if i != b]
        assert not bool(torch.isfinite(emb[b]).all())
        assert int(mi[b]) == -1 and float(dist[b]) == math.inf and int(ids[b]) == -1, (kind, idx, int(mi[b]), float(dist[b]), int(ids[b]))
        assert torch.equal(dist[keep], clean[1][keep])


@pytest.mark.parametrize("C", [2, 65, 1000])
def test_softmax_argmax(C):
    o = {"l": synth.randn(2170 + C, (5, C), "l") * 3}
    _drive("softmax_argmax", o, ["l"], lambda q: tuple(t.cpu() for t in ops.softmax_argmax(q["l"].to(DEV))),
           lambda q: (F.softmax(q["l"].double(), dim=1),), [_close(1e-6)], int_outputs=(1,), rot=C)


@pytest.mark.parametrize("D", [4, 65, 1000])
def test_pairwise_distance(D):
    o = {"a": synth.randn(2180 + D, (5, D), "a"), "b": synth.randn(2181 + D, (5, D), "b")}
    _drive("pairwise_distance", o, ["a", "b"], lambda q: (ops.pairwise_distance(q["a"].to(DEV), q["b"].to(DEV))[0].cpu(),),
           lambda q: (torch.sqrt(((q["a"].double() - q["b"].double() + 1e-6) ** 2).sum(1)),), [_close(0.0, 1e-6)], rot=D)


def test_cosine_logits():
    """65 x 4 against 129 classes (a partial K step, a second column block)."""
    o = {"x": synth.randn(2190, (65, 4), "x"), "w": synth.randn(2191, (129, 4), "w")}
    poison.assert_no_zero(o["w"])
    _drive("cosine_logits", o, ["x"], lambda q: tuple(t.cpu() for t in ops.cosine_logits(q["x"].to(DEV), q["w"].to(DEV), s=32.0)),
           lambda q: (32.0 * (F.normalize(q["x"].double(), dim=1, eps=1e-12) @ F.normalize(q["w"].double(), dim=1, eps=1e-12).t()),),
           [_close(1e-4)], int_outputs=(1,))


# --------------------------------------------------------------------------------------------------------------------------------
# transformer.hip
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_add_pos_layernorm_and_mean_layernorm(dtype):
    B, L, D = 3, 5, 256
    o = {"x": synth.randn(2200, (B, L, D), "x").to(dtype), "pos": synth.randn(2201, (L, D), "p") * 0.5,
         "g": 1.0 + 0.1 * synth.randn(2202, (D,), "g"), "b": 0.1 * synth.randn(2203, (D,), "b")}
    atol, rtol = (2e-3, 2e-3) if dtype == torch.float16 else (1.6e-2, 1.6e-2)          # `test_attention_gpu._tol`

    def run(q):
        t, y = ops.add_pos_layernorm(q["x"].to(DEV), q["pos"].to(DEV), q["g"].to(DEV), q["b"].to(DEV), want_sum=True)
        return t.cpu(), y.cpu()

    def ref(q):
        t, y = ac.add_pos_layernorm_ref(q["x"], q["pos"], q["g"], q["b"], True)
        return t.double(), y
    _drive("add_pos_layernorm", o, ["x"], run, ref, [None, _close(2 * atol, rtol, zero_exact=False)])
    _drive("mean_layernorm", o, ["x"], lambda q: (ops.mean_layernorm(q["x"].to(DEV), q["g"].to(DEV), q["b"].to(DEV)).cpu(),),
           lambda q: (ac.mean_layernorm_ref(q["x"], q["g"], q["b"]),), [_close(2e-4, 1e-4, zero_exact=False)], rot=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("H", [1, 2])
def test_mha_tokens(H, dtype):
    """B = 3, L = 21 (not a multiple of 16: padded keys are live), the `flat` family (an almost uniform softmax: no probability
    rounds to zero in the storage type, so P * inf is inf in the kernel as in float64).  Every kind (NaN, +inf, -inf) at every
    position: two in Q rows, one in a K row, two in V rows.  A poison in a Q row reaches that output row alone, one in a K or V row
    what the float64 reference says; finite changed elements meet `attention_cases.mha_ratio`'s rule."""
    B, L = 3, 21
    o = {"qkv": ac.mha_inputs("flat", 2210 + H, B, L, H, dtype)}
    u = cc.UNIT[dtype]

    def rules(q):                           # the rule's magnitude terms belong to the poisoned operands of this run
        terms = ac.mha_ref(q["qkv"], H)[2]
        terms = torch.where(torch.isfinite(terms), terms, torch.zeros_like(terms))
        return [lambda got, want, mask: ~mask | ((got.double() - want).abs() <= 2 * u * terms + 1e-6)]
    D = H * ac.DH
    parts = {("Q" if idx[2] < D else "K" if idx[2] < 2 * D else "V") for _, idx in poison.positions(o["qkv"].shape)}
    assert parts == {"Q", "K", "V"}, parts
    seen = _drive("mha_tokens", o, ["qkv"], lambda q: (ops.mha_tokens(q["qkv"].to(DEV), H).cpu(),), lambda q: (ac.mha_ref(q["qkv"], H)[0],),
                  rules, every_kind=True)
    assert {(k, "Q" if i[2] < D else "K" if i[2] < 2 * D else "V") for _, i, k, _ in seen} >= {("nan", "Q"), ("nan", "K"), ("nan", "V")}
    clean = ops.mha_tokens(o["qkv"].to(DEV), H).cpu()
    for key, idx, kind, (y,) in seen:
        if idx[2] < D:                     # a Q element: only row idx[1] of image idx[0] (and only its head) may differ
            same = (y == clean) | (torch.isnan(y) & torch.isnan(clean))
            same[idx[0], idx[1]] = True
            assert bool(same.all()), (kind, idx)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_cnn_attention(dtype):
    """3 x 4 x 9 x 256, Cq = 32, KS = 3 (`test_attention_gpu.py`'s non-square case): map (storage) and pooled (fp32) outputs, poison
    in qkv (its q part: channel 0; k part: channel 40, an extra position; v part: channels 160 and 319) and in x."""
    B, H, W, C, Cq, KS = 3, 4, 9, 256, 32, 3
    qkv, x, gamma, sw, sb = ac.cnn_attention_inputs(2220, B, H, W, C, Cq, KS, dtype)
    poison.assert_no_zero(sw)
    o = {"qkv": qkv, "x": x}
    ref64 = ac.cnn_attention_ref(qkv, x, Cq, gamma, sw, sb)
    A = ac.cnn_attention_margin(qkv, x, Cq, gamma, sw, sb, ref64)
    u = cc.UNIT[dtype]

    def run(q):
        m, p = ops.cnn_attention(q["qkv"].to(DEV), q["x"].to(DEV), gamma.to(DEV), sw.to(DEV), sb.to(DEV), Cq, want_map=True, want_pool=True)
        return m.cpu(), p.cpu()
    _drive("cnn_attention", o, ["qkv", "x"], run, lambda q: ac.cnn_attention_ref(q["qkv"], q["x"], Cq, gamma, sw, sb),
           [_close(A, 2 * u, zero_exact=False), _close(A, 0.0, zero_exact=False)], extra={"qkv": [("k-part", (1, 2, 4, Cq + 8))]})
