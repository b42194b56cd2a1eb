"""No GPU: the instruments of the conv-family GPU tests (`conv_cases.py`) checked on the CPU.

* the float64 references against `F.conv2d`, `F.max_pool2d`, `F.gelu` and `F.linear` in float64;
* the exact-integer builder's two conditions (S <= 256, every (tap, cin) position in at least two output channels) on every entry
  of the GPU case tables, and that fp32 arithmetic rounded to either storage dtype reproduces float64 on them;
* where C_ACC comes from: the worst `|y32 - ref| / (2^-24 S)` of two fp32 restatements (the chunk-by-chunk order of the kernels,
  and torch's own fp32 conv), re-measured here;
* that the one-rounding bound accepts the correct emulation and misses each broken form by at least 2 x, and that the exact-integer
  equality rejects a dropped term and replicate padding;
* that every bound case of the GPU tables keeps the rule sharp (the accumulation allowance stays under a quarter of the rounding
  term).
"""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc

DTYPES = [torch.float16, torch.bfloat16]

# B, H, W, Cin, Cout, k, stride: many chunks, a ragged map, one chunk, stride 2, 1x1
EMU_SHAPES = [(2, 7, 7, 512, 64, 3, 1), (2, 9, 9, 128, 64, 3, 1), (2, 10, 6, 32, 64, 3, 1), (2, 8, 6, 64, 64, 3, 2), (3, 7, 7, 128, 64, 1, 1)]


def _emu_operands(i, family, dtype):
    B, H, W, Cin, Cout, k, s = EMU_SHAPES[i]
    return cc.float_operands(family, 100 + i, B, H, W, Cin, Cout, k, dtype, s, res=True), s


# ------------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,Cout,k,s,pad", [(2, 9, 7, 32, 8, 3, 1, 1), (2, 9, 7, 32, 8, 3, 2, 1), (3, 8, 6, 16, 8, 1, 1, 0),
                                                  (3, 9, 6, 16, 8, 1, 2, 0), (2, 21, 13, 3, 8, 7, 2, 3), (2, 6, 5, 3, 8, 3, 1, 1)])
def test_conv_reference_is_conv2d_in_float64(B, H, W, Cin, Cout, k, s, pad):
    g = torch.Generator().manual_seed(B * H + k)
    x, w = torch.randn((B, Cin, H, W), generator=g), torch.randn((Cout, Cin, k, k), generator=g)
    shift = torch.randn((Cout,), generator=g)
    want = F.conv2d(x.double(), w.double(), None, stride=s, padding=pad) + shift.double().view(1, -1, 1, 1)
    r = torch.randn(tuple(want.shape), generator=g)
    ref, S = cc.conv_ref(x, w, shift, s, pad, r)
    assert torch.allclose(ref, want + r.double(), rtol=1e-13, atol=1e-13)
    wantS = F.conv2d(x.double().abs(), w.double().abs(), None, stride=s, padding=pad) + shift.double().abs().view(1, -1, 1, 1) + r.double().abs()
    assert torch.allclose(S, wantS, rtol=1e-13, atol=1e-13) and bool((S >= ref.abs() - 1e-12).all())
    if k == 3 and s == 1:      # + projection shortcut (stride 2 over a map of size 2 H x 2 W)
        xd, wd = torch.randn((B, 16, 2 * H, 2 * W), generator=g), torch.randn((Cout, 16, 1, 1), generator=g)
        ref2, S2 = cc.conv_shortcut_ref(x, w, shift, xd, wd, 2)
        assert torch.allclose(ref2, want + F.conv2d(xd.double(), wd.double(), None, stride=2), rtol=1e-13, atol=1e-13)
        assert torch.allclose(S2, wantS - r.double().abs() + F.conv2d(xd.double().abs(), wd.double().abs(), None, stride=2), rtol=1e-13, atol=1e-13)


def test_pool_gelu_and_linear_references():
    g = torch.Generator().manual_seed(5)
    t = torch.randn((2, 5, 31, 19), generator=g, dtype=torch.float64)
    for k, s, p in ((3, 2, 1), (2, 2, 0)):
        assert torch.equal(cc.window_max(t, k, s, p), F.max_pool2d(t, k, s, p))
        assert torch.equal(cc.window_max(t[:, :, :30, :18], k, s, p), F.max_pool2d(t[:, :, :30, :18], k, s, p))
    pr, pS = cc.pooled(t, t.abs() + 1, cc.ACT_RELU, 3, 2, 1)
    assert torch.equal(pr, F.max_pool2d(F.relu(t), 3, 2, 1)) and torch.equal(pS, F.max_pool2d(t.abs() + 1, 3, 2, 1))
    v = torch.linspace(-6, 6, 24001, dtype=torch.float64)
    assert torch.allclose(cc.act64(v, cc.ACT_GELU), F.gelu(v), rtol=0, atol=1e-15)
    assert torch.equal(cc.act64(v, cc.ACT_RELU), F.relu(v)) and torch.equal(cc.act64(v, cc.ACT_NONE), v)
    vv = v.clone().requires_grad_(True)
    F.gelu(vv).sum().backward()
    assert 1.128 < float(vv.grad.abs().max()) <= cc.GELU_LIP
    x, w, b = torch.randn((5, 96), generator=g), torch.randn((64, 96), generator=g), torch.randn((64,), generator=g)
    r = torch.randn((5, 64), generator=g)
    ref, S = cc.linear_ref(x, w, b, r)
    assert torch.allclose(ref, F.linear(x.double(), w.double(), b.double()) + r.double(), rtol=1e-13, atol=1e-13)
    assert torch.allclose(S, F.linear(x.double().abs(), w.double().abs(), b.double().abs()) + r.double().abs(), rtol=1e-13, atol=1e-13)


# ------------------------------------------------------------------------------------------------------------------------------
# exact-integer builder
# ------------------------------------------------------------------------------------------------------------------------------
def test_exact_weights_are_spread_and_cover():
    """The construction the issue measured: n_nz = 200 at (Cin 512, Cout 128, 3x3) covers every position at least 5 times, and one
    channel's nonzeros reach every tap and every 32-channel chunk."""
    w = cc.exact_weights(1, 128, 512, 3, 200)
    assert cc.coverage_min(w) >= 5 and int((w != 0).sum(dim=(1, 2, 3)).min()) == 200 == int((w != 0).sum(dim=(1, 2, 3)).max())
    nz0 = (w[0] != 0)                                                       # [Cin, 3, 3]
    assert bool(nz0.any(dim=0).all()), "channel 0 misses a tap"
    assert bool(nz0.view(16, 32, 3, 3).any(dim=1).any(dim=-1).any(dim=-1).all()), "channel 0 misses a 32-channel chunk"


@pytest.mark.parametrize("name", [c.name for c in cc.CONV_CASES])
def test_exact_case_conditions(name):
    """(a) and (b) on the case's operands; the outputs take many distinct values; fp32 arithmetic (torch's own order) rounded to fp16
    and to bf16 IS the float64 result."""
    case = cc.case_by_name(name)
    o = cc.exact_case_operands(case)
    want, S, act = cc.case_reference(case, o)
    preS = cc.conv_shortcut_ref(o["x"], o["w"], o["shift"], o["xd"], o["wd"], case.ds[1])[1] if case.op == "ds" else \
        cc.conv_ref(o["x"], o["w"], o["shift"], case.stride, cc.case_pad(case), o.get("r"))[1]
    cc.assert_exact_conditions(o, preS, name)
    assert act != cc.ACT_GELU and case.act != cc.ACT_GELU
    assert want.unique().numel() >= 16 or want.numel() < 200, (name, want.unique().numel())   # (27-term sums behind ReLU + max: 22)
    y32 = F.conv2d(o["x"].float(), o["w"].float(), None, stride=case.stride, padding=cc.case_pad(case)) + o["shift"].view(1, -1, 1, 1)
    if o.get("r") is not None:
        y32 = y32 + o["r"].float()
    if case.op == "ds":
        y32 = y32 + F.conv2d(o["xd"].float(), o["wd"].float(), None, stride=case.ds[1])
    pool = {"pool2": (2, 2, 0), "c3pool2": (2, 2, 0), "stem3": (3, 2, 1), "stem2": (2, 2, 0)}.get(case.op.replace("u8", ""))
    relu = case.act == cc.ACT_RELU or case.op.startswith("stem")
    y32 = F.relu(y32) if relu else y32
    y32 = F.max_pool2d(y32, *pool) if pool else y32
    for dtype in DTYPES:
        cc.assert_exact(y32.to(dtype), want, act, name)


@pytest.mark.parametrize("name", [c.name for c in cc.LINEAR_CASES if c.act != cc.ACT_GELU])
def test_exact_linear_case_conditions(name):
    lc = next(c for c in cc.LINEAR_CASES if c.name == name)
    o = cc.linear_operands(lc, "exact", None)
    ref, S = cc.linear_ref(o["x"], o["w"], o["shift"], o["r"])
    cc.assert_exact_conditions({"w": o["w"].view(lc.N, lc.K, 1, 1), "x": o["x"], "shift": o["shift"], "r": o["r"]}, S, name)
    y32 = o["x"].float() @ o["w"].float().t() + o["shift"] + (o["r"].float() if lc.res else 0)
    for dtype in DTYPES:
        cc.assert_exact(y32.to(dtype), ref, cc.ACT_NONE, name)


def test_exact_equality_rejects_dropped_term_and_replicate_padding():
    for (B, H, W, Cin, Cout) in ((2, 7, 7, 512, 128), (3, 5, 3, 32, 128)):
        o = cc.exact_operands(31, B, H, W, Cin, Cout, 3, res=True)
        ref, S = cc.conv_ref(o["x"], o["w"], o["shift"], residual=o["r"])
        cc.assert_exact_conditions(o, S)
        oc, c, ky, kx = (int(v) for v in torch.nonzero(o["w"])[Cin + 3])          # some product that exists
        for dtype in DTYPES:
            cc.assert_exact(cc.emulate_conv(o, dtype, act=cc.ACT_RELU), ref, cc.ACT_RELU)
            cc.assert_exact(cc.emulate_conv(o, dtype, act=cc.ACT_RELU, chunk_round=True, splitk_storage=True), ref, cc.ACT_RELU)   # integers: exact in any order
            with pytest.raises(AssertionError, match="differ from the exact integers"):
                cc.assert_exact(cc.emulate_conv(o, dtype, drop_term=(oc, c, ky, kx)), ref)
            with pytest.raises(AssertionError, match="differ from the exact integers"):
                cc.assert_exact(cc.emulate_conv(o, dtype, replicate_pad=True), ref)


# ------------------------------------------------------------------------------------------------------------------------------
# the one-rounding bound
# ------------------------------------------------------------------------------------------------------------------------------
def test_c_acc_is_four_times_the_fp32_restatements():
    """C_ACC = 8 is 4 x the worst `|y32 - ref| / (2^-24 S)` of the chunk-by-chunk fp32 restatement (the kernels' order), as a power
    of two; torch's own fp32 conv, another order, stays under it too.  Printed, then asserted."""
    worst_seq = worst_torch = 0.0
    for i, (B, H, W, Cin, Cout, k, s) in enumerate(EMU_SHAPES):
        for family in ("gauss", "relu"):
            for dtype in DTYPES:
                o, _ = _emu_operands(i, family, dtype)
                ref, S = cc.conv_ref(o["x"], o["w"], o["shift"], s, None, o["r"])
                y_seq = cc.emulate_conv(o, dtype, s, want_fp32=True)
                y_t = F.conv2d(o["x"].float(), o["w"].float(), None, stride=s, padding=k // 2) + o["shift"].view(1, -1, 1, 1) + o["r"].float()
                a = float(((y_seq.double() - ref).abs() / (cc.EPS32 * S)).max())
                b = float(((y_t.double() - ref).abs() / (cc.EPS32 * S)).max())
                print(f"c: {EMU_SHAPES[i]} {family} {str(dtype)[6:]}: chunk-sequential {a:.2f}, torch fp32 conv {b:.2f}  (x 2^-24 S)")
                worst_seq, worst_torch = max(worst_seq, a), max(worst_torch, b)
    print(f"c: worst chunk-sequential {worst_seq:.2f}, worst torch {worst_torch:.2f}, C_ACC = {cc.C_ACC:g}")
    assert 4 * worst_seq <= cc.C_ACC <= 16 * worst_seq, worst_seq
    assert 2 * worst_torch <= cc.C_ACC, worst_torch


@pytest.mark.parametrize("dtype", DTYPES)
def test_bound_accepts_the_correct_emulation_and_rejects_each_rounding_defect(dtype):
    worst_ok = 0.0
    least = {"chunk_round": math.inf, "splitk_storage": math.inf, "round_before_residual": math.inf}
    for i, (B, H, W, Cin, Cout, k, s) in enumerate(EMU_SHAPES):
        for family in ("gauss", "relu") + (("subnormal",) if dtype == torch.float16 else ()):
            o, _ = _emu_operands(i, family, dtype)
            ref, S = cc.conv_ref(o["x"], o["w"], o["shift"], s, None, o["r"])
            what = f"{EMU_SHAPES[i]} {family} {str(dtype)[6:]}"
            worst_ok = max(worst_ok, cc.assert_one_rounding(cc.emulate_conv(o, dtype, s, act=cc.ACT_RELU), ref, S, dtype, cc.ACT_RELU, what))
            want = cc.act64(ref, cc.ACT_RELU)
            for flaw in least:
                if flaw != "round_before_residual" and Cin == 32:
                    continue                        # one chunk: nothing to round between chunks, nothing to split
                ratio = cc.one_rounding_ratio(cc.emulate_conv(o, dtype, s, act=cc.ACT_RELU, **{flaw: True}), want, S, dtype)
                least[flaw] = min(least[flaw], ratio)
                assert ratio >= 2.0, (what, flaw, ratio)
                with pytest.raises(AssertionError):
                    cc.assert_one_rounding(cc.emulate_conv(o, dtype, s, act=cc.ACT_RELU, **{flaw: True}), ref, S, dtype, cc.ACT_RELU, what)
            if family == "gauss" and Cin == 512:    # NOT caught: a shift rounded to the storage dtype
                print(f"bound: {what}: shift rounded to storage reaches {cc.one_rounding_ratio(cc.emulate_conv(o, dtype, s, act=cc.ACT_RELU, shift_storage=True), want, S, dtype):.2f} x the bound")
    print(f"bound {str(dtype)[6:]}: correct emulation reaches {worst_ok:.3f} x the bound; smallest miss of each defect:",
          {k_: round(v, 1) for k_, v in least.items()})
    assert worst_ok <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_bound_rejects_tanh_gelu(dtype):
    """1x1 conv + erf-GELU (HybridNet's MLP): the tanh form differs by up to 4.7e-4, most visibly where GELU is small (v ~ -2.3)."""
    o = cc.float_operands("gauss", 140, 3, 7, 7, 128, 256, 1, dtype, w_gain=2.0)
    ref, S = cc.conv_ref(o["x"], o["w"], o["shift"])
    ok = cc.assert_one_rounding(cc.emulate_conv(o, dtype, act=cc.ACT_GELU), ref, S, dtype, cc.ACT_GELU, "erf-GELU")
    bad = cc.one_rounding_ratio(cc.emulate_conv(o, dtype, act=cc.ACT_GELU, tanh_gelu=True), cc.act64(ref, cc.ACT_GELU), S, dtype, cc.GELU_LIP)
    print(f"gelu {str(dtype)[6:]}: erf form reaches {ok:.3f} x the bound, tanh form {bad:.1f} x")
    assert bad >= 2.0, bad


@pytest.mark.parametrize("name", [c.name for c in cc.CONV_CASES + cc.GELU_CASES if not c.op.endswith("u8")] + [c.name for c in cc.LINEAR_CASES])
def test_bound_cases_keep_the_rule_sharp(name):
    """`c 2^-24 max S <= u mean|ref| / 4` on the float operands of every GPU case, at fp16 (bf16's u is 8 x larger), for the
    Gaussian and the post-ReLU builder: checked here so that a case that would drown the rounding term never reaches a GPU."""
    lin = next((c for c in cc.LINEAR_CASES if c.name == name), None)
    for family in ("gauss", "relu"):
        if lin is not None:
            o = cc.linear_operands(lin, family, torch.float16)
            want, S, act = cc.linear_ref(o["x"], o["w"], o["shift"], o["r"]) + (lin.act,)
        else:
            case = cc.case_by_name(name)
            want, S, act = cc.case_reference(case, cc.float_case_operands(case, family, torch.float16))
        slack = cc.C_ACC * cc.EPS32 * float(S.max()) / (cc.UNIT[torch.float16] * float(cc.act64(want, act).abs().mean()) / 4)
        assert slack <= 1.0, (name, family, slack)
