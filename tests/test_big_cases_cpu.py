"""CPU: the instrument of the large-tensor tests (`big_cases.py`), proven with the marks scaled down to 2^15 and 2^16 bytes.

A toy "kernel" in torch reads a large operand byte by byte through an offset computation and stores `byte + 1` at the same
offset of a guarded output.  The correct variant passes the three checks of a case (first period, periodic output, nothing else
written).  Each broken variant - the byte offset truncated to log2(MARK) bits, on the load and on the store side; the record count
clamped at MARK, so reads beyond it return 0; the offset computed in a signed type of that width - must fail them.  Then: a
period that divides a mark is refused, `smallest_batch` equals hand-computed values, and every case of the GPU tables keeps its
period condition, crosses every mark, stays under the memory cap and under its launcher's limit, on the path it names.
"""
import pytest
import torch

import big_cases as bc
import conv_cases as cc

MARK = 2 ** 16                                                  # stands for 2^32 bytes; MARK / 2 for 2^31
SMALL = {"bytes": (MARK // 2, MARK), "elems": MARK // 2}        # 2-byte elements: 2^15 elements = 2^16 bytes
ITEM = 96                                                       # bytes per item: 48 two-byte elements
K = 7
FILL = 0xFF
BAND = 4096
CHUNK = 4096


def _block():
    g = torch.Generator().manual_seed(11)
    return torch.randint(0, 250, (K, ITEM), generator=g).to(torch.uint8)


def toy_kernel(x, B, variant):
    """out[o] = x[src(o)] + 1 for every byte offset o < B * ITEM, between bands of FILL.  Returns (output [B, ITEM], its raw buffer)."""
    n = B * ITEM
    o = torch.arange(n, dtype=torch.int64)
    front = MARK                                                # room in front of the operand for a negative offset
    xp = torch.full((front + n,), FILL, dtype=torch.uint8)
    xp[front:] = x.reshape(-1)
    src, dst, live = o, o, torch.ones(n, dtype=torch.bool)
    if variant == "load-truncated":
        src = o & (MARK - 1)
    elif variant == "store-truncated":
        dst = o & (MARK - 1)
    elif variant == "clamped":
        live = o < MARK
    elif variant == "signed":
        src = ((o + MARK // 2) % MARK) - MARK // 2              # a signed offset of log2(MARK) bits
    elif variant != "correct":
        raise ValueError(variant)
    val = torch.where(live, xp[front + src], torch.zeros((), dtype=torch.uint8)) + 1
    raw = torch.full((BAND + n + BAND,), FILL, dtype=torch.uint8)
    raw[BAND + dst] = val                                       # (a truncated store writes the same bytes twice: the last one stays)
    return raw[BAND:BAND + n].view(B, ITEM), raw


def check_case(variant, first_period=True):
    """The three checks of a GPU case, on the toy kernel (`first_period=False`: without the comparison with the reference)."""
    block = _block()
    op = bc.Operand("x", ITEM, 2)
    bc.assert_period(op.item_bytes, op.elem_bytes, K, SMALL)
    B = bc.smallest_batch([op], K, SMALL)
    assert bc.crosses(B, op, K, SMALL)
    x = bc.tile_on_device(block, B, CHUNK)
    assert torch.equal(x[K * 5 + 3], block[3]) and x.shape == (B, ITEM)
    y, raw = toy_kernel(x, B, variant)
    assert not first_period or torch.equal(y[:K], block + 1), "first period"
    bc.assert_periodic(y.contiguous(), K, CHUNK, what=variant)
    assert bool((raw[:BAND] == FILL).all()) and bool((raw[-BAND:] == FILL).all()), "band written"
    bc.assert_operand_intact(x, block, what=variant)


def test_the_correct_toy_kernel_passes():
    check_case("correct")


@pytest.mark.parametrize("variant", ["load-truncated", "store-truncated", "clamped", "signed"])
def test_each_broken_toy_kernel_fails(variant):
    with pytest.raises(AssertionError):
        check_case(variant)
    with pytest.raises(AssertionError, match="differs from item"):       # ... and the periodic check alone sees it
        check_case(variant, first_period=False)


def test_the_periodic_check_names_the_first_bad_item_and_sees_nan_bits():
    y = bc.tile_on_device(torch.arange(K * 8, dtype=torch.float32).view(K, 8), 100, 64)
    bc.assert_periodic(y, K, 64)
    z = y.clone()
    z[61, 5] = float("nan")                                     # an unwritten (0xFF..) element
    with pytest.raises(AssertionError, match="item 61 differs from item 5 .* at element 5"):
        bc.assert_periodic(z, K, 64)
    n = y.clone()
    n[:, 2] = float("nan")                                      # the same NaN bits everywhere: periodic (NaN != NaN must not matter)
    bc.assert_periodic(n, K, 64)


def test_a_period_that_could_hide_a_wrap_is_refused():
    bc.assert_period(512, 2, 7, SMALL)
    with pytest.raises(AssertionError, match="multiple of the period"):
        bc.assert_period(512, 2, 8, SMALL)                      # 8 x 512 divides 2^15
    with pytest.raises(AssertionError, match="multiple of the period"):
        bc.assert_period(4096, 2, 16)                           # ... and 16 x 4 KiB divides 2^31
    for item in (2, 96, 756, 3276, 4096, 7 * 1024, 49 * 2 ** 20):
        bc.assert_period(item, 2, 7)                            # an odd prime: no power of two is a multiple of it
    with pytest.raises(AssertionError, match="are equal"):
        bc.tile_on_device(torch.ones(K, 4), 20)                 # equal items shorten the period


def test_smallest_batch_against_hand_computed_values():
    two = 2 ** 32                                              # 2-byte elements: 2^32 bytes = 2^31 elements
    assert bc.smallest_batch([bc.Operand("x", 8192, 2)]) == two // 8192 + 1 + 14 == 524303
    assert bc.smallest_batch([bc.Operand("x", 3276, 4)]) == 2 ** 33 // 3276 + 15 == 2622095          # fp32: 2^31 elements are 8 GiB
    assert bc.smallest_batch([bc.Operand("u8", 756, 1)]) == 2 ** 32 // 756 + 15 == 5681188           # uint8: 4 GiB
    # the smallest operand decides, and every operand then crosses every mark by two periods; one item fewer does not
    ops_ = [bc.Operand("x", 4096, 2), bc.Operand("out", 1024, 2), bc.Operand("f", 2048, 4)]
    B = bc.smallest_batch(ops_)
    assert B == two // 1024 + 15 == 4194319
    assert all(bc.crosses(B, op) for op in ops_) and not bc.crosses(B - 1, ops_[1])
    assert bc.smallest_batch([bc.Operand("x", ITEM, 2)], K, SMALL) == MARK // ITEM + 15 == 697


# ------------------------------------------------------------------------------------------------------------------------------
# the GPU tables
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,dtype,kernel", bc.BIG_CONV, ids=[c.name for c, _, _ in bc.BIG_CONV])
def test_conv_case_crosses_the_marks_within_the_cap_on_its_path(case, dtype, kernel):
    operands, B = bc.conv_operands(case), bc.conv_batch(case)
    assert case.B == bc.K and {op.name for op in operands} >= {"out"}
    for op in operands:
        bc.assert_period(op.item_bytes, op.elem_bytes, what=case.name)
        assert bc.crosses(B, op) and B * op.item_bytes // op.elem_bytes > 2 ** 31
    assert any(not bc.crosses(B - 1, op) for op in operands), "not the smallest batch"
    assert bc.conv_estimate(case, B) <= bc.MEM_CAP, (case.name, bc.conv_estimate(case, B) / 2 ** 30)
    assert bc.conv_pixels(case, B) < bc.LIMIT_M, (case.name, bc.conv_pixels(case, B))
    # the block's operands are exact integers with every (tap, cin) product covered, as in the small cases
    if not case.op.endswith("u8"):
        o = cc.exact_case_operands(case)
        ref, S, _ = cc.case_reference(case, o)
        cc.assert_exact_conditions(o, S, case.name)
        assert tuple(ref.shape[1:]) == (case.Cout,) + bc.conv_out_hw(case)
    if case.query is not None:       # the path at the large batch, as `conv_cases.launch_case` will assert it on the GPU
        from frmap_amd import _lib, ops
        lib = _lib.load()
        try:
            if case.tune is not None:
                assert lib.frmap_conv_pp_tuning(*case.tune) == 0
            big = case._replace(B=B)
            assert cc.query_path(lib, ops, big) in case.query[1], (case.name, cc.query_path(lib, ops, big))
            if case.op == "ds":
                H2, W2 = 2 * case.H, 2 * case.W
                assert ops.conv_ds_supported(B, case.H, case.W, case.Cin, case.Cout, H2, W2, case.ds[0], case.ds[1])
        finally:
            lib.frmap_conv_pp_tuning(-1, -1, -1)


def test_one_dtype_per_case_alternating_and_names_unique():
    names = [c.name for c, _, _ in bc.BIG_CONV]
    assert len(set(names)) == len(names) and not set(names) & {c.name for c in cc.CONV_CASES + cc.GELU_CASES}
    dts = [d for _, d, _ in bc.BIG_CONV]
    assert all(a != b for a, b in zip(dts, dts[1:]))
    files = {c.file for c, _, _ in bc.BIG_CONV}
    assert files == {cc.IG, cc.PP, cc.SC, cc.ST, cc.S2D}


def test_linear_case_sizes():
    for lc in bc.BIG_LINEAR:
        ops_ = bc.linear_operands(lc)
        B = bc.smallest_batch(ops_)
        assert B < bc.LIMIT_M and all(bc.crosses(B, op) for op in ops_)
        assert bc.estimate_bytes([B * op.item_bytes for op in ops_]) <= bc.MEM_CAP
        from frmap_amd import _lib
        assert _lib.load().frmap_linear_mfma_workspace_bytes(B, lc.K, lc.N) == 0      # no split-K at a large M (BIG_CONV_NOT_RUN)
        assert _lib.load().frmap_linear_mfma_workspace_bytes(49152, 256, 64) > 0 and _lib.load().frmap_linear_mfma_workspace_bytes(49153, 256, 64) == 0


@pytest.mark.parametrize("op", bc.BIG_LAYOUT, ids=[o.name for o in bc.BIG_LAYOUT])
def test_layout_case_crosses_the_marks_within_the_cap_and_the_launchers_limit(op):
    large, every = bc.op_operands(op)
    B = bc.op_batch(op)
    assert 0 < B < 2 ** 31 and len(large) >= 1 and set(op.inputs) <= {o.name for o in large}
    for o in large:
        bc.assert_period(o.item_bytes, o.elem_bytes, what=op.name)
        assert bc.crosses(B, o), (op.name, o)
    assert op.B is not None or any(not bc.crosses(B - 1, o) for o in large), "not the smallest batch"
    assert bc.op_estimate(op, B) <= bc.MEM_CAP
    for what, value, bound in op.limits:
        assert value(B) < bound, (op.name, what)
    if op.name == "add_pos_layernorm-limit":        # just under: one more face would pass the limit
        assert (B + 1) * bc.APL_L >= bc.ROWS_LIMIT


def test_every_batch_sized_grid_stays_under_2_to_the_32_threads():
    """A grid of 2^32 threads or more is cut down without an error (frmap_common.h, FRMAP_GRID_FITS): the cases with one wave per row
    or one workgroup per item carry that limit in the table, and the conv cases' grids follow from M."""
    by = {o.name: o for o in bc.BIG_LAYOUT}
    for name, per_item in (("l2_normalize", 64), ("pairwise_distance", 64), ("avgpool_global", 64), ("mha_tokens", 256),
                           ("mean_layernorm", 256), ("cnn_attention", 256), ("add_pos_layernorm-limit", 64 * bc.APL_L)):
        assert by[name].limits and bc.op_batch(by[name]) * per_item < 2 ** 32, name
    for case, _, _ in bc.BIG_CONV:
        B = bc.conv_batch(case)
        assert (bc.conv_pixels(case, B) // 128 + 1) * max(case.Cout // 64, 1) * 512 < 2 ** 32, case.name      # at least 128 pixels x 64 channels a workgroup
