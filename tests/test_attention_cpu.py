"""CPU: the float64 references of `attention_cases.py` against torch / the oracle, and the TEETH of the acceptance rules the
GPU tests apply: an fp32 emulation of each attention kernel passes them, and the same emulation with one deliberate mistake
(key mask off by one or absent, attention matrix transposed, scale 1/sqrt(D) for 1/sqrt(128), gate convolution with H and W
swapped) is rejected by a wide factor."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import face_oracle as fo

import attention_cases as ac

DTYPES = [torch.float16, torch.bfloat16]


@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("L", [1, 17, 49, 64])
def test_mha_ref_equals_torch_multi_head_attention(L, H):
    """`mha_ref` against F.multi_head_attention_forward in float64 with identity projections and no biases."""
    B, D = 2, H * ac.DH
    qkv = ac.mha_inputs("peaked", 100 + L, B, L, H, torch.float16)
    O, P, terms = ac.mha_ref(qkv, H)
    q, k, v = (z.transpose(0, 1).contiguous() for z in qkv.double().split(D, dim=-1))          # torch wants [L, B, D]
    eye = torch.eye(D, dtype=torch.float64)
    o, w = F.multi_head_attention_forward(q, k, v, D, H, None, None, None, None, False, 0.0, eye, None, training=False,
                                          need_weights=True, use_separate_proj_weight=True, q_proj_weight=eye,
                                          k_proj_weight=eye, v_proj_weight=eye, average_attn_weights=False)
    assert torch.allclose(O, o.transpose(0, 1), atol=1e-12, rtol=1e-12)
    assert torch.allclose(P, w, atol=1e-13, rtol=1e-12)
    assert torch.allclose(P.sum(-1), torch.ones(B, H, L, dtype=torch.float64), atol=1e-13)
    assert bool((terms >= O.abs()).all())


@pytest.mark.parametrize("KS", [1, 3, 7])
def test_cnn_attention_ref_equals_oracle_attention_module(KS):
    """`cnn_attention_ref` (NHWC, packed q|k|v) against `oracle.face_oracle.attention_module` (NCHW, 1x1 convolutions) in
    float64 on a non-square map, plus the position mean."""
    B, H, W, C, Cq = 2, 4, 9, 64, 8
    x = ac.synth.randn(200 + KS, (B, C, H, W), "x").double()
    sd = {"a.gamma": torch.tensor([0.7], dtype=torch.float64),
          "a.spatial_attention.conv.weight": ac.synth.randn(201, (1, 2, KS, KS), "sw").double() / KS,
          "a.spatial_attention.conv.bias": torch.tensor([-0.3], dtype=torch.float64)}
    for name, n in (("query", Cq), ("key", Cq), ("value", C)):
        sd[f"a.{name}.weight"] = ac.synth.randn(202, (n, C, 1, 1), name).double() * (0.7 / math.sqrt(C) if n == Cq else 0.1)
        sd[f"a.{name}.bias"] = ac.synth.randn(203, (n,), name + ".b").double() * 0.1
    want = fo.attention_module(sd, "a.", x)
    qkv = torch.cat([F.conv2d(x, sd[f"a.{n}.weight"], sd[f"a.{n}.bias"]) for n in ("query", "key", "value")], dim=1)
    m, pool = ac.cnn_attention_ref(qkv.permute(0, 2, 3, 1), x.permute(0, 2, 3, 1), Cq, sd["a.gamma"],
                                   sd["a.spatial_attention.conv.weight"], sd["a.spatial_attention.conv.bias"])
    assert torch.allclose(m.permute(0, 3, 1, 2), want, atol=1e-12, rtol=1e-12)
    assert torch.allclose(pool, want.mean(dim=(2, 3)), atol=1e-12, rtol=1e-12)


def test_input_families_are_what_they_claim():
    """Peaked logits have a standard deviation near 4 and a large top probability; flat ones an almost uniform softmax; the
    mask-sensitive ones sit near -19, far below the 0 of a padded key."""
    H, L = 4, 49
    for fam, lo, hi in (("peaked", 0.4, 1.0), ("flat", 0.0, 0.06)):
        qkv = ac.mha_inputs(fam, 7, 3, L, H, torch.float16)
        _, P, _ = ac.mha_ref(qkv, H)
        top = float(P.max(-1).values.mean())
        assert lo < top < hi, (fam, top)
    qkv = ac.mha_inputs("mask_sensitive", 7, 3, L, H, torch.float16).double()
    q, k = (ac._heads(z, 3, L, H) for z in qkv.split(H * ac.DH, dim=-1)[:2])
    logits = q @ k.transpose(-1, -2) / math.sqrt(ac.DH)
    assert -23 < float(logits.mean()) < -16 and float(logits.max()) < -10


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [1, 15, 16, 17, 33, 49, 63])
def test_mha_acceptance_rule_has_teeth(L, dtype):
    """The correct emulation is inside `|out - O| <= 2 u (P @ |V| + |O|) + 1e-6` on every input family; each wrong one is
    outside it by at least 10 x.  With one key the softmax is the constant 1, so at L = 1 a transposed matrix and another scale
    ARE the correct kernel: there they must pass, and only the key mask can be (and is) caught."""
    B, H = 2, 4
    for fam in ("peaked", "flat", "mask_sensitive"):
        qkv = ac.mha_inputs(fam, 300 + L, B, L, H, dtype)
        ref = ac.mha_ref(qkv, H)
        raw, rule = ac.mha_ratio(ac.emulate_mha(qkv, H, dtype), ref)
        print(f"mha teeth {fam} L={L} {dtype}: correct {raw:.3f} u")
        assert rule <= 1.0, (fam, rule)
        if fam == "mask_sensitive":
            for upto in (L + 1, ac.LP):                               # the mask one key late, and no mask at all
                bad = ac.mha_ratio(ac.emulate_mha(qkv, H, dtype, mask_upto=upto), ref)[1]
                assert bad >= 10.0, (fam, upto, bad)
        if fam == "peaked":
            wrong = (ac.mha_ratio(ac.emulate_mha(qkv, H, dtype, transpose=True), ref)[1],
                     ac.mha_ratio(ac.emulate_mha(qkv, H, dtype, scale=1.0 / math.sqrt(H * ac.DH)), ref)[1])
            if L == 1:
                assert max(wrong) <= 1.0
            else:
                assert min(wrong) >= 10.0, wrong


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W", [(4, 9), (8, 8)])
def test_cnn_attention_acceptance_rule_has_teeth(H, W, dtype):
    """The correct emulation passes `|map - want| <= 2 u |want| + A`, `|pool - want| <= A`; a transposed attention matrix fails
    more than half of the map on both shapes; a gate convolution that swaps H and W fails more than half of it on the 4 x 9
    map and is, by construction, invisible on the square one (which is why the GPU cases are not square)."""
    B, C, Cq, KS = 2, 256, 32, 3
    qkv, x, gamma, sw, sb = ac.cnn_attention_inputs(400 + H, B, H, W, C, Cq, KS, dtype)
    ref = ac.cnn_attention_ref(qkv, x, Cq, gamma, sw, sb)
    A = ac.cnn_attention_margin(qkv, x, Cq, gamma, sw, sb, ref)
    fm, fp, worst = ac.cnn_attention_fail(*ac.emulate_cnn_attention(qkv, x, Cq, gamma, sw, sb, dtype), ref, A)
    print(f"cnn_attention teeth {H}x{W} {dtype}: A = {A:.3g}, correct err/A = {worst:.3f}")
    assert not bool(fm.any()) and not bool(fp.any())
    fm, fp, _ = ac.cnn_attention_fail(*ac.emulate_cnn_attention(qkv, x, Cq, gamma, sw, sb, dtype, transpose=True), ref, A)
    assert float(fm.float().mean()) > 0.5 and float(fp.float().mean()) > 0.5
    m, p = ac.emulate_cnn_attention(qkv, x, Cq, gamma, sw, sb, dtype, swap_hw=True)
    fm, fp, _ = ac.cnn_attention_fail(m, p, ref, A)
    if H == W:
        assert not bool(fm.any()) and not bool(fp.any())
    else:
        assert float(fm.float().mean()) > 0.5
