"""GPU: every conv-family address scheme on tensors past the 2 GiB and 4 GiB offset marks (`big_cases.py`: periodic operands).

One case per address scheme of conv_igemm.hip (wave kernel's per-image / per-patch descriptors, the register-prefetch kernel's
re-based descriptors with one image per tile and with several, its residual descriptor at m0 * Cout, the generic kernel's 64-bit
gather, both stride-2 kernels, the 1x1 gather and stage kernels, the fused shortcut with its second large operand, the pooled
generic and wave forms), conv_pp.hip (3x3 with 128 / 256-channel tiles and split-K, stride 2, the shortcut form, 1x1 layouts
1 / 2 / 3, the pooled form), conv_small_cin.hip, stem_pool.hip (fp32 with both pools, uint8), stem_s2d.hip (fp32, uint8) and
linear_mfma with large M.  Exact-integer operands of period 7 (`conv_cases.exact_operands`), one dtype per case, alternating.

Per case: the batch is `big_cases.smallest_batch` of its large operands (input, shortcut input, residual, output: each past 2^32
bytes = 2^31 elements by two periods; the stems' fp32 input past 8 GiB, the uint8 input past 4 GiB); the path is asserted by the
layout / form query at that batch; the first period equals the float64 reference bit for bit (`conv_cases.assert_exact`); every
other output item holds the bits of its index modulo 7; the output comes from `guard.Guard.patch` under the fill 0xFF with its
bands checked; the operands' first and last period are unchanged.  All kernels here compute an output pixel from its own image in
a position-independent order (fixed chunk order, split-K merged in a fixed order), so bit-identity is the rule for all of them.
Each case prints its batch, operand sizes and path (`pytest -s`)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import big_cases as bc  # noqa: E402
import conv_cases as cc  # noqa: E402
import guard  # noqa: E402
from frmap_amd import _lib, ops  # noqa: E402

K = bc.K
LARGE_KEYS = ("x", "r", "xd", "x4", "u8")


def _dt(dtype):
    return str(dtype)[6:]


@pytest.mark.parametrize("case,dtype,kernel", bc.BIG_CONV, ids=[c.name for c, _, _ in bc.BIG_CONV])
def test_conv_past_the_offset_marks(case, dtype, kernel):
    operands, B = bc.conv_operands(case), bc.conv_batch(case)
    for op in operands:
        bc.assert_period(op.item_bytes, op.elem_bytes, what=f"{case.name}.{op.name}")
        assert bc.crosses(B, op), (case.name, op)
    assert bc.conv_pixels(case, B) < bc.LIMIT_M
    bc.need_memory(bc.conv_estimate(case, B), case.name)
    what = f"{case.file} {case.name} {_dt(dtype)} B={B}"

    o = cc.gpu_operands(case, "exact", dtype)                    # the block: K images
    want, S, act = cc.case_reference(case, o)
    assert float(S.max()) <= cc.S_MAX_EXACT
    block = cc.device_operands(case, o, dtype)
    big = {k: bc.tile_on_device(block[k], B) for k in LARGE_KEYS if k in block}
    g = guard.Guard(0xFF)
    y = None
    try:
        with g.patch(ops):
            y = cc.launch_case(case._replace(B=B), dict(block, **big), dtype)
        g.check()
        sizes = {op.name: "%.2f GiB" % (B * op.item_bytes / 2 ** 30) for op in operands}
        print(f"\n{what}: M={bc.conv_pixels(case, B)} {sizes} query={case.query} kernel={kernel} estimate={bc.conv_estimate(case, B) / 2 ** 30:.1f} GiB "
              f"peak={torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
        assert y.dtype == dtype and y.shape[0] == B and y.numel() * 2 == B * operands[0].item_bytes
        cc.assert_exact(y[:K].cpu().permute(0, 3, 1, 2), want, act, what + " (first period)")
        bc.assert_periodic(y, K, what=what)
        for k, t in big.items():
            bc.assert_operand_intact(t, block[k], what=f"{what} operand {k}")
    finally:
        del y, big, g
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()


@pytest.mark.parametrize("lc", bc.BIG_LINEAR, ids=[c.name for c in bc.BIG_LINEAR])
def test_linear_mfma_past_the_offset_marks(lc):
    """`linear_mfma` with M past 2^25 rows (x, residual and out past 4 GiB).  At that M `linear_ksplit` is 1 (asserted): the
    split-K form cannot be reached with large operands (`big_cases.BIG_CONV_NOT_RUN`)."""
    dtype = torch.float16
    operands = bc.linear_operands(lc)
    B = bc.smallest_batch(operands)
    for op in operands:
        bc.assert_period(op.item_bytes, op.elem_bytes, what=f"{lc.name}.{op.name}")
        assert bc.crosses(B, op)
    assert B < bc.LIMIT_M
    bc.need_memory(bc.estimate_bytes([B * op.item_bytes for op in operands], bands=2 ** 20), lc.name)
    assert _lib.load().frmap_linear_mfma_workspace_bytes(B, lc.K, lc.N) == 0, "split-K at a large M"
    o = cc.exact_operands(8101, K, 1, 1, lc.K, lc.N, 1, res=lc.res, n_nz=lc.K)
    x, w, r = o["x"].reshape(K, lc.K), o["w"].reshape(lc.N, lc.K), o["r"].reshape(K, lc.N)
    ref, S = cc.linear_ref(x, w, o["shift"], r)
    assert float(S.max()) <= cc.S_MAX_EXACT
    wpk = ops.pack_conv_weight(w.float().view(lc.N, lc.K, 1, 1).to(cc.DEV), dtype)
    xb, rb = x.to(dtype).to(cc.DEV), r.to(dtype).to(cc.DEV)
    xbig, rbig = bc.tile_on_device(xb, B), bc.tile_on_device(rb, B)
    g = guard.Guard(0xFF)
    y = None
    try:
        with g.patch(ops):
            y = ops.linear_mfma(xbig, wpk, o["shift"].float().to(cc.DEV), lc.N, lc.act, rbig)
        g.check()
        print(f"\n{lc.name} fp16 M={B} K={lc.K} N={lc.N}: x {B * lc.K * 2 / 2 ** 30:.2f} GiB, out and residual {B * lc.N * 2 / 2 ** 30:.2f} GiB")
        cc.assert_exact(y[:K].cpu(), ref, lc.act, lc.name + " (first period)")
        bc.assert_periodic(y, K, what=lc.name)
        bc.assert_operand_intact(xbig, xb, what=lc.name + " x")
        bc.assert_operand_intact(rbig, rb, what=lc.name + " residual")
    finally:
        del y, xbig, rbig, g
        torch.cuda.empty_cache()
