"""GPU: every conv-family kernel between guard bands (`guard.py`): it writes all of its output and nothing else, and its result
does not depend on a byte outside its operands.

Every entry of `conv_cases.CONV_CASES` and `CENSUS_CASES` (exact-integer operands), `GELU_CASES` (their float operands) and `LINEAR_CASES`, in fp16
and bf16, runs through `conv_cases.run_case` / `run_linear` three times: unguarded, and with every operand, output and
workspace between bands of 0xFF.. (NaN) and of 0x5A.. (203.25 in fp16).  `Guard.check()` must pass and the three outputs must
hold the same bits.  What the values ARE is the business of `test_conv_exact_gpu.py` / `test_conv_bound_gpu.py`.  The weight
packers are guarded too: the packed buffer is exactly `numel` elements, a permutation of the weights (1x1 / 3x3) or the rows
[Cout][kh KR + kw 4 + c] with zeros in the pitch padding (Cin = 3).

Workspace fields of this family (`conv_igemm.hip`, `frmap_linear_mfma`; first write / first read, read from the code):
  slab [ksplit][M][N] fp32   written in full by `conv_epilogue_partial` of the K-slice workgroups (every m < M, every channel of
                             the workgroup's 64-channel tile; the grid covers ceil(M / BM) x N / 64 x ksplit) / read by
                             `splitk_finalize_kernel` after that launch, slabs 0 .. ksplit - 1 only.  `ksplit` there is
                             `plan_1x1`'s, clamped to at most the `linear_ksplit` that sizes the workspace.  No field is read first.
Run-to-run bits: no conv kernel accumulates floats with atomics (split-K sums its slabs in a fixed order), so every case here
follows the bit-identity rule; none uses a reference bound.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_cases as cc  # noqa: E402
import guard  # noqa: E402
from frmap_amd import _lib, ops  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", cc.CONV_CASES + cc.CENSUS_CASES, ids=[c.name for c in cc.CONV_CASES + cc.CENSUS_CASES])
def test_conv_case_is_guarded(case, dtype):
    o = cc.gpu_operands(case, "exact", dtype)
    fused_pool = case.op in ("pool2", "c3pool2")        # (their two-launch twin runs between the same bands)
    guard.two_fills(lambda place: cc.run_case(case, o, dtype, also_unfused=fused_pool, place=place), [ops], what=case.name)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", cc.GELU_CASES, ids=[c.name for c in cc.GELU_CASES])
def test_gelu_case_is_guarded(case, dtype):
    o = cc.gpu_operands(case, "gauss", dtype)
    guard.two_fills(lambda place: cc.run_case(case, o, dtype, place=place), [ops], what=case.name)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("lc", cc.LINEAR_CASES, ids=[c.name for c in cc.LINEAR_CASES])
def test_linear_case_is_guarded(lc, dtype):
    """The split-K cases get a workspace of exactly `frmap_linear_mfma_workspace_bytes` between bands."""
    o = cc.linear_operands(lc, "gauss" if lc.act == cc.ACT_GELU else "exact", dtype)
    seen = []

    def run(place):
        g = getattr(place, "__self__", None)
        y = cc.run_linear(lc, o, dtype, place=place)
        if g is not None:
            seen.append(sorted(a.nbytes for a in g.allocs if a.who == "ops.linear_mfma"))
        return y
    guard.two_fills(run, [ops], what=lc.name)
    ws = _lib.load().frmap_linear_mfma_workspace_bytes(lc.M, lc.K, lc.N)
    want = sorted([lc.M * lc.N * 2] + ([ws] if ws else []))
    assert seen == [want, want], (lc.name, seen, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("Cout,Cin,k", [(64, 32, 1), (128, 160, 1), (64, 32, 3), (128, 64, 3)])
def test_pack_conv_weight_is_guarded(Cout, Cin, k, dtype):
    w = cc.exact_operands(31 + k, 1, 4, 4, Cin, Cout, k, n_nz=Cin * k * k)["w"].float()
    w = w * torch.arange(1, Cout + 1, dtype=torch.float32).view(-1, 1, 1, 1).remainder(7).add(1)      # (small integers: exact in both types)
    packed, = guard.two_fills(lambda place: ops.pack_conv_weight(place(w), dtype), [ops], what="pack_conv_weight")
    assert packed.numel() == w.numel() and packed.dtype == dtype
    assert torch.equal(packed.float().sort().values, w.reshape(-1).sort().values)                        # a permutation of the weights


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("Cout,k", [(64, 7), (32, 3)])
def test_pack_conv_weight_c3_is_guarded(Cout, k, dtype):
    g = torch.Generator().manual_seed(5 + k)
    w = torch.randint(1, 9, (Cout, 3, k, k), generator=g).float()                                        # no zero weight: padding stands out
    packed, = guard.two_fills(lambda place: ops.pack_conv_weight_c3(place(w), dtype), [ops], what="pack_conv_weight_c3")
    pitch = _lib.load().frmap_small_cin_kpad(k, k)
    KR = 32 if k * 4 > 16 else 16
    want = torch.zeros((Cout, pitch))
    for kh in range(k):
        for kw in range(k):
            want[:, kh * KR + kw * 4:kh * KR + kw * 4 + 3] = w[:, :, kh, kw]
    assert packed.numel() == Cout * pitch and int((want == 0).sum()) == Cout * (pitch - 3 * k * k)
    assert torch.equal(packed.float().view(Cout, pitch), want)
