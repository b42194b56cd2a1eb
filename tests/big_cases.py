"""Shared code of the large-tensor tests (`test_big_cases_cpu.py`, `test_big_conv_gpu.py`, `test_big_layout_gpu.py`,
`test_big_match_gpu.py`): kernels on tensors past the 2 GiB and 4 GiB offset marks, where a 32-bit offset wraps, a signed one
turns negative and a buffer descriptor's record count is clamped.  A plain helper module like `conv_cases.py` / `guard.py`.

THE INSTRUMENT: PERIODIC OPERANDS.  A float64 reference of 2^31 elements is out of reach and not needed.

1. One period is built on the CPU: a block of K distinct items (images, token rows, gallery rows) from the existing builders,
   with the block's float64 reference from the existing reference code.  The block is uploaded once and tiled on the device to
   the batch B: `x_big[n] = block[n % K]` (`tile_on_device`).
2. The period cannot hide a wrap (`assert_period`): with `period = K x bytes per item`, no mark (2^31 bytes, 2^32 bytes, 2^31
   elements) is a multiple of the period, and a displacement by a mark lands either inside an item (mark % item bytes != 0) or on
   an item with another index modulo K; the items of a block are pairwise different (`tile_on_device` asserts it).  K = 7 does
   that for every item size that is not itself a multiple of 7 times a power of two.  A wrapped read then sees another item or
   a mid-item shift, a clamped or zeroed read sees zeros.
3. Three checks per case; the large tensors never leave the device:
   * first period: `out[:K]` against the float64 reference under the rule the kernel's existing test uses;
   * whole output: `out[n]` holds the bits of `out[n % K]` for every n (`assert_periodic`, in chunks);
   * nothing else written: the wrappers' outputs and workspaces come from `guard.Guard.patch` under the fill 0xFF (an unwritten
     element is NaN and breaks the period; a store past the end lands in a band); the large operands are allocated directly and
     their first and last period are compared with the block after the launch (`assert_operand_intact`).
4. A case is sized by bytes (`smallest_batch`): B is the smallest batch at which every large operand exceeds 2^32 bytes AND 2^31
   elements by at least two periods (2-byte tensors: one condition; fp32: 8 GiB; uint8: 4 GiB).

The case tables of the GPU files are here, so that the CPU test can check every case's period, size and memory estimate.
"""
from collections import namedtuple

import numpy as np
import torch

import conv_cases as cc

MARK_BYTES = (2 ** 31, 2 ** 32)            # byte offsets at which a signed / an unsigned 32-bit byte offset wraps
MARK_ELEMS = 2 ** 31                       # element index at which a signed 32-bit index wraps
MARKS = {"bytes": MARK_BYTES, "elems": MARK_ELEMS}
K = 7                                      # items per period
MEM_CAP = 48 * 2 ** 30                     # peak device memory of a case
CHUNK_BYTES = 256 * 2 ** 20                # comparison chunk: the temporaries of `assert_periodic` stay under 1 GiB
LIMIT_M = 2 ** 31                          # every conv launcher refuses M >= 2^31 output pixels

Operand = namedtuple("Operand", "name item_bytes elem_bytes")


def marks_in_bytes(elem_bytes, marks=MARKS):
    """Every mark as a byte offset into a tensor of `elem_bytes`-byte elements."""
    return sorted(set(marks["bytes"]) | {marks["elems"] * elem_bytes})


def assert_period(item_bytes, elem_bytes, k=K, marks=MARKS, what=""):
    """The period condition of one large operand (see the module docstring); raises AssertionError where a wrap could hide."""
    assert k >= 2 and item_bytes > 0 and item_bytes % elem_bytes == 0, (what, k, item_bytes, elem_bytes)
    period = k * item_bytes
    for mark in marks_in_bytes(elem_bytes, marks):
        assert mark % period != 0, (what, "mark %d is a multiple of the period %d x %d bytes" % (mark, k, item_bytes))
        if mark % item_bytes == 0:         # a wrap lands on an item's first byte: it must be another item of the block
            assert (mark // item_bytes) % k != 0, (what, "mark %d = %d whole items, a multiple of the period %d" % (mark, mark // item_bytes, k))


def smallest_batch(operands, k=K, marks=MARKS):
    """The smallest batch at which every large operand (`Operand`s: bytes per item, bytes per element) exceeds the largest byte
    mark and the element mark by at least two periods."""
    B = 0
    for op in operands:
        far = max(max(marks["bytes"]), marks["elems"] * op.elem_bytes)          # the farthest mark, in bytes
        B = max(B, far // op.item_bytes + 1 + 2 * k)                            # > far / item_bytes items, plus two periods
    return B


def crosses(B, op, k=K, marks=MARKS):
    """Whether a batch of B items carries `op` past every mark by two periods."""
    return all(B * op.item_bytes > m + 2 * k * op.item_bytes for m in marks_in_bytes(op.elem_bytes, marks))


def estimate_bytes(operand_bytes, chunk_bytes=CHUNK_BYTES, bands=0):
    """Peak device memory of a case: its large tensors (operands, outputs, workspaces), the tiling prototype and the comparison's
    temporaries (a prototype chunk, a chunk-sized mask: 3 chunks), the guard bands and 256 MiB for everything small."""
    return int(sum(operand_bytes)) + 3 * chunk_bytes + bands + 256 * 2 ** 20


def need_memory(nbytes, what=""):
    """The skip rule: a case skips, with the numbers, only where the device reports less free memory than its estimate."""
    import pytest
    assert nbytes <= MEM_CAP, (what, "estimate %.1f GiB over the cap of %d GiB" % (nbytes / 2 ** 30, MEM_CAP // 2 ** 30))
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip("%s needs %.1f GiB of device memory, %.1f GiB of %.1f GiB are free" % (what, nbytes / 2 ** 30, free / 2 ** 30, total / 2 ** 30))


def release(*tensors):
    """Called with the case's large tensors already deleted by the caller: returns the cached blocks to the device."""
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------------
# tiling and the periodic comparison (torch on any device: the CPU test runs them on scaled-down marks)
# ------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    """A contiguous tensor's storage as integers of its element size (NaNs compare by their bits)."""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _items_per_chunk(item_bytes, k, chunk_bytes):
    return max(1, chunk_bytes // (k * item_bytes)) * k


def tile_on_device(block, B, chunk_bytes=CHUNK_BYTES):
    """`out[n] = block[n % K]` for n < B, K = block.shape[0]; `block` is a contiguous tensor on the target device whose items are
    pairwise different (asserted: two equal items would shorten the period)."""
    k = block.shape[0]
    flat = _bits(block.contiguous()).reshape(k, -1)
    assert torch.unique(flat.cpu(), dim=0).shape[0] == k, "two items of the block are equal"
    out = torch.empty((B,) + tuple(block.shape[1:]), dtype=block.dtype, device=block.device)
    step = _items_per_chunk(flat.shape[1] * flat.element_size(), k, chunk_bytes)
    proto = block.repeat((min(step, -(-B // k) * k) // k,) + (1,) * (block.dim() - 1))
    for n0 in range(0, B, step):
        n1 = min(B, n0 + step)
        out[n0:n1] = proto[:n1 - n0]
    return out


def assert_periodic(out, k=K, chunk_bytes=CHUNK_BYTES, what=""):
    """`out[n]` holds the same bits as `out[n % k]` for every n, compared on `out`'s device chunk by chunk."""
    B = out.shape[0]
    assert out.is_contiguous() and B >= k, (what, tuple(out.shape))
    flat = _bits(out).reshape(B, -1)
    step = _items_per_chunk(flat.shape[1] * flat.element_size(), k, chunk_bytes)
    proto = flat[:k].repeat(min(step, -(-B // k) * k) // k, 1)
    for n0 in range(0, B, step):
        n1 = min(B, n0 + step)
        if torch.equal(flat[n0:n1], proto[:n1 - n0]):
            continue
        bad = (flat[n0:n1] != proto[:n1 - n0])
        rows = torch.nonzero(bad.any(dim=1)).reshape(-1)
        n = n0 + int(rows[0])
        e = int(torch.nonzero(bad[int(rows[0])]).reshape(-1)[0])
        es = out.element_size()
        raise AssertionError("%s: item %d differs from item %d (its index modulo %d) at element %d: byte offset %d = 2^31 %+d = 2^32 %+d; "
                             "%d of the %d items of this chunk differ, the last is item %d" % (
                                 what, n, n % k, k, e, (n * flat.shape[1] + e) * es, (n * flat.shape[1] + e) * es - 2 ** 31,
                                 (n * flat.shape[1] + e) * es - 2 ** 32, rows.numel(), n1 - n0, n0 + int(rows[-1])))


def assert_operand_intact(big, block, what=""):
    """The first and the last period of a large operand still hold the block (the launch wrote nothing into its input)."""
    k, B = block.shape[0], big.shape[0]
    assert torch.equal(_bits(big[:k].contiguous()), _bits(block.contiguous())), (what, "first period of the operand modified")
    last = (B // k - 1) * k
    assert torch.equal(_bits(big[last:last + k].contiguous()), _bits(block.contiguous())), (what, "last period of the operand modified")


# ------------------------------------------------------------------------------------------------------------------------------
# conv family: one case per address scheme.  Per-image shapes are the smallest the planner still gives to the same kernel at the
# large batch (asserted on the GPU by the layout / form queries of `conv_cases.launch_case`, on the CPU by the planner program of
# `test_conv_plan_cpu.py`, which plans every entry of this table at its batch and compares the kernel's name).
# ------------------------------------------------------------------------------------------------------------------------------
F16, BF16 = torch.float16, torch.bfloat16
_c, IG, PP, SC, ST, S2D, PP_OFF = cc._c, cc.IG, cc.PP, cc.SC, cc.ST, cc.S2D, cc.PP_OFF
RELU, NONE = cc.ACT_RELU, cc.ACT_NONE

# (case with B = K, dtype, the kernel the planner must name or None where no planner is involved)
BIG_CONV = [
    # ---- conv_igemm.hip, second generation off ----
    (_c("big-wave", IG, "conv", K, 8, 16, 64, 128, res=True, tune=PP_OFF, query=("conv3x3_pp", (0,))), F16, "conv3x3_c64_wave_kernel"),
    (_c("big-regprefetch-1img", IG, "conv", K, 16, 16, 32, 64, res=True, tune=PP_OFF, query=("conv3x3_pp", (0,))), BF16, "conv3x3_fast_kernel"),
    (_c("big-regprefetch-small", IG, "conv", K, 5, 3, 64, 64, res=True, act=NONE, tune=PP_OFF, query=("conv3x3_pp", (0,))), F16, "conv3x3_fast_kernel"),
    (_c("big-generic", IG, "conv", K, 8, 112, 32, 64, tune=PP_OFF, query=("conv3x3_pp", (0,))), BF16, "conv_igemm_kernel"),
    (_c("big-s2-split", IG, "conv", K, 16, 104, 32, 128, stride=2, tune=PP_OFF, query=("conv3x3s2_pp", (0,))), F16, "conv3x3s2_split_kernel"),
    (_c("big-s2-fast", IG, "conv", K, 16, 16, 32, 128, stride=2, res=True, tune=PP_OFF, query=("conv3x3s2_pp", (0,))), BF16, "conv3x3s2_fast_kernel"),
    (_c("big-1x1-gather", IG, "conv", K, 4, 4, 64, 128, k=1, stride=2, act=NONE, tune=PP_OFF, query=("conv1x1_pp", (0,))), F16, "conv_igemm_kernel"),
    (_c("big-1x1-stage", IG, "conv", K, 2, 2, 128, 128, k=1, res=True, tune=PP_OFF, query=("conv1x1_pp", (0,))), BF16, "conv1x1_kernel"),
    (_c("big-g1-shortcut", IG, "ds", K, 4, 4, 64, 128, ds=(32, 2), tune=PP_OFF, query=("conv3x3_pp_ds", (0,))), F16, "conv3x3_fast_kernel"),
    (_c("big-pool2-generic", IG, "pool2", K, 6, 6, 64, 256, query=("pool2_form", (1,))), BF16, "conv_igemm_kernel"),
    (_c("big-pool2-wave", IG, "pool2", K, 8, 8, 32, 128, query=("pool2_form", (2,))), F16, "conv3x3_c64_wave_kernel"),
    # ---- conv_pp.hip (a tile of 224 / 448 pixels spans many small images and its halo their padding rows as well: these are
    #      the smallest maps whose halo still fits the layout at a large batch) ----
    (_c("big-pp-bn128", PP, "conv", K, 10, 10, 128, 128, res=True, tune=(1, -1, 128), ri=0, query=("conv3x3_pp", (2,))), BF16, "conv3x3_pp_kernel"),
    (_c("big-pp-bn256", PP, "conv", K, 4, 4, 256, 256, res=True, tune=(1, -1, 256), ri=1, query=("conv3x3_pp", (1,))), F16, "conv3x3_pp_kernel"),
    (_c("big-pp-splitk", PP, "conv", K, 6, 6, 128, 128, tune=(1, -1, 1282), ri=0, query=("conv3x3_pp", (3,))), BF16, "conv3x3_pp_kernel"),
    (_c("big-pp-s2", PP, "conv", K, 20, 20, 32, 128, stride=2, res=True, tune=(1, -1, -1), query=("conv3x3s2_pp", (2,))), F16, "conv3x3s2_pp_kernel"),
    (_c("big-pp-shortcut", PP, "ds", K, 4, 4, 128, 256, ds=(32, 2), act=NONE, tune=(1, -1, -1), query=("conv3x3_pp_ds", (1,))), BF16, "conv3x3_pp_kernel"),
    (_c("big-pp1x1-layout1", PP, "conv", K, 2, 2, 256, 256, k=1, tune=(1, -1, 256), query=("conv1x1_pp", (1,))), F16, "conv1x1_pp_kernel"),
    (_c("big-pp1x1-layout2", PP, "conv", K, 2, 2, 128, 128, k=1, res=True, tune=(1, -1, 128), query=("conv1x1_pp", (2,))), BF16, "conv1x1_pp_kernel"),
    (_c("big-pp1x1-layout3", PP, "conv", K, 2, 2, 128, 128, k=1, act=NONE, tune=(1, -1, 1282), query=("conv1x1_pp", (3,))), F16, "conv1x1_pp_kernel"),
    (_c("big-pp-pool", PP, "pool2", K, 4, 4, 128, 512, query=("pool2_form", (3,))), BF16, "conv3x3_pp_kernel"),
    # ---- Cin = 3 and the stems (their launchers plan for themselves) ----
    (_c("big-c3-3x3", SC, "c3", K, 6, 10, 3, 32), F16, None),
    (_c("big-c3-7x7s2", SC, "c3", K, 12, 10, 3, 64, k=7, stride=2), BF16, None),
    (_c("big-c3-pool2", SC, "c3pool2", K, 6, 10, 3, 32), F16, None),
    (_c("big-stem-pool3", ST, "stem3", K, 21, 13, 3, 64, k=7, stride=2), BF16, None),          # W % 4 != 0: stem_pool_kernel
    (_c("big-stem-pool2", ST, "stem2", K, 21, 13, 3, 64, k=7, stride=2), F16, None),
    (_c("big-stem-pool2-u8", ST, "stem2u8", K, 21, 12, 3, 64, k=7, stride=2), BF16, None),
    (_c("big-stem-s2d", S2D, "stem3", K, 21, 12, 3, 64, k=7, stride=2), F16, None),          # pool3 and W % 4 == 0: stem_s2d_kernel
    (_c("big-stem-s2d-u8", S2D, "stem3u8", K, 21, 12, 3, 64, k=7, stride=2), BF16, None),
]

# Named by the issue and not run, with the reason:
BIG_CONV_NOT_RUN = {
    "linear_mfma split-K at large M": "`linear_ksplit` = min(384 / tiles, chunks / 4) with tiles = ceil(M / 256) x N / 64: it is 1 from 193 "
                                      "tiles on (M = 49,153 rows at N = 64), so no batch whose operands pass 4 GiB (M >= 2^23 at K = N = 256) splits",
}

BIG_LINEAR = [cc.LinCase("big-linear-no-split", K, 64, 64, RELU, True, False)]


def conv_out_hw(case):
    if case.op in ("pool2", "c3pool2"):
        return case.H // 2, case.W // 2
    if case.op.startswith("stem"):     # conv 7x7 s2 p3, then MaxPool2d(3, 2, 1) or MaxPool2d(2, 2)
        Hc, Wc = (case.H - 1) // 2 + 1, (case.W - 1) // 2 + 1
        return ((Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1) if case.op.startswith("stem3") else (Hc // 2, Wc // 2)
    return cc._out_hw(case.H, case.W, case.k, case.stride, cc.case_pad(case))


def conv_operands(case):
    """The large operands of a conv-family case, per item (= per image)."""
    Ho, Wo = conv_out_hw(case)
    ops_ = [Operand("out", Ho * Wo * case.Cout * 2, 2)]
    if case.op in ("conv", "ds", "pool2"):
        ops_.append(Operand("x", case.H * case.W * case.Cin * 2, 2))
        if case.res:
            ops_.append(Operand("r", Ho * Wo * case.Cout * 2, 2))
        if case.ds is not None:
            dsC, sd = case.ds
            ops_.append(Operand("xd", ((case.H - 1) * sd + 1 + (sd - 1)) * ((case.W - 1) * sd + 1 + (sd - 1)) * dsC * 2, 2))
    elif case.op in ("c3", "c3pool2"):
        ops_.append(Operand("x4", case.H * case.W * 4 * 2, 2))
    elif case.op.endswith("u8"):
        ops_.append(Operand("u8", case.H * case.W * 3, 1))
    else:
        ops_.append(Operand("x", case.H * case.W * 3 * 4, 4))
    return ops_


def conv_batch(case):
    return smallest_batch(conv_operands(case))


def conv_pixels(case, B):
    """M of the launch (output pixels of the conv itself: before the pool of the fused forms)."""
    if case.op in ("pool2", "c3pool2"):
        return B * case.H * case.W
    if case.op.startswith("stem"):
        return B * ((case.H - 1) // 2 + 1) * ((case.W - 1) // 2 + 1)
    Ho, Wo = cc._out_hw(case.H, case.W, case.k, case.stride, cc.case_pad(case))
    return B * Ho * Wo


def linear_operands(lc):
    return [Operand("x", lc.K * 2, 2), Operand("out", lc.N * 2, 2)] + ([Operand("r", lc.N * 2, 2)] if lc.res else [])


def conv_estimate(case, B):
    return estimate_bytes([B * op.item_bytes for op in conv_operands(case)], bands=4 * 2 ** 20)


# ------------------------------------------------------------------------------------------------------------------------------
# the three checks for an op given as a Python call (layout, pool, token and head kernels)
# ------------------------------------------------------------------------------------------------------------------------------
def run_periodic(name, blocks, call, check_first, modules, B=None, small_outputs=(), device="cuda", k=K):
    """`blocks`: name -> CPU tensor of k items (the large operands); `call(ops)`: the op on a dict of device tensors, returning a tuple
    of tensors with the batch as first dimension (None allowed); `check_first(outs)`: the existing acceptance rule on the CPU
    copies of a k-item result.  The op runs once on the block (B = k): that gives the outputs' item sizes and must pass the rule.
    Then B = `smallest_batch` over the operands and the outputs (indices in `small_outputs` excepted: outputs of a few bytes per
    item, which no batch an `int` holds carries past a mark) unless `B` is given (a launcher's limit), the operands are tiled, the
    op runs with its outputs and workspaces guarded (fill 0xFF), and: the first period holds the bits of the k-item run, every
    output is periodic, the bands are clean, the operands' first and last period are unchanged.  Returns (B, sizes in bytes)."""
    import guard
    dev = {n: t.contiguous().to(device) for n, t in blocks.items()}
    small = call(dev)
    torch.cuda.synchronize()
    check_first(tuple(None if t is None else t.cpu() for t in small))
    operands = [Operand(n, t[0].numel() * t.element_size(), t.element_size()) for n, t in blocks.items()]
    outs = [Operand("out%d" % i, t[0].numel() * t.element_size(), t.element_size()) for i, t in enumerate(small) if t is not None]
    large = operands + [o for o in outs if int(o.name[3:]) not in small_outputs]
    for op in large:
        assert_period(op.item_bytes, op.elem_bytes, k, what=f"{name}.{op.name}")
    if B is None:
        B = smallest_batch(large, k)
    assert all(crosses(B, op, k) for op in large), (name, B, [op for op in large if not crosses(B, op, k)])
    sizes = {op.name: B * op.item_bytes for op in operands + outs}
    est = estimate_bytes(sizes.values(), bands=len(outs) * 2 ** 20)
    need_memory(est, name)
    big = {n: tile_on_device(t, B) for n, t in dev.items()}
    g = guard.Guard(0xFF, device=device)
    res = None
    try:
        with g.patch(*modules):
            res = call(big)
        g.check()
        print("\n%s: B=%d %s estimate=%.1f GiB peak=%.1f GiB" % (name, B, {n: "%.2f GiB" % (v / 2 ** 30) for n, v in sizes.items()}, est / 2 ** 30,
                                                                torch.cuda.max_memory_allocated() / 2 ** 30))
        assert len(res) == len(small)
        for i, (r, s) in enumerate(zip(res, small)):
            if s is None:
                assert r is None
                continue
            assert r.shape[0] == B and r.dtype == s.dtype and tuple(r.shape[1:]) == tuple(s.shape[1:]), (name, i, tuple(r.shape))
            assert torch.equal(_bits(r[:k].contiguous()), _bits(s.contiguous())), (name, "output %d: the first period differs from the B = %d run" % (i, k))
            assert_periodic(r, k, what="%s output %d" % (name, i))
        for n in big:
            assert_operand_intact(big[n], dev[n], what="%s operand %s" % (name, n))
    finally:
        del res, big, g
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    return B, sizes


# ------------------------------------------------------------------------------------------------------------------------------
# layout, pool, token and head kernels (`test_big_layout_gpu.py`): name, dtype of the 2-byte tensors, the large inputs and the
# outputs as (item shape, dtype) - an output of a few bytes per item is marked small -, a fixed batch where a launcher's limit
# sets it (else `smallest_batch`), and the launcher limits as (what, value at batch B, bound it stays under)
# ------------------------------------------------------------------------------------------------------------------------------
F32, U8, I32 = torch.float32, torch.uint8, torch.int32
BigOp = namedtuple("BigOp", "name dtype inputs outputs small B limits")
ROWS_LIMIT = 2 ** 31 // 64                 # add_pos_layernorm: rows < 2^31 / 64
GEMM_ROWS_LIMIT = 65535 * 64 + 1           # the fp32 GEMM: rows on the grid's y axis
# A grid holds fewer than 2^32 threads (`FRMAP_GRID_FITS`, frmap_common.h): a larger one is cut down modulo 2^32 without an error.
WAVE_ROWS_LIMIT = 2 ** 26 - 3              # one wave per row: rows <= 2^26 - 4
WG256_LIMIT = 2 ** 24                      # one 256-thread workgroup per item: items <= 2^24 - 1
APL_L = 3


def _op(name, dtype, inputs, outputs, small=(), B=None, limits=()):
    return BigOp(name, dtype, inputs, outputs, tuple(small), B, tuple(limits))


BIG_LAYOUT = [
    _op("pack_input-pairs", F16, {"x": ((3, 4, 5), F32)}, [((4, 5, 4), F16)]),                       # H W even: two pixels per thread
    _op("pack_input-odd", BF16, {"x": ((3, 3, 5), F32)}, [((3, 5, 4), BF16)]),                       # H W odd: the one-pixel kernel
    _op("normalize_u8", F16, {"img": ((3, 5, 3), U8)}, [((3, 3, 5), F32), ((3, 5, 4), F16)]),
    _op("cast_to_f32", BF16, {"x": ((24,), BF16)}, [((24,), F32)]),
    _op("cast_from_f32", F16, {"x": ((24,), F32)}, [((24,), F16)]),
    _op("maxpool", BF16, {"x": ((3, 3, 8), BF16)}, [((3, 3, 8), BF16)]),                             # 3x3 stride 1 pad 1
    # one wave per (image, 8 channels): B C / 8 <= 2^26 - 4 waves, so the fp32 [B, C] output stays under 2 GiB: the input is the large one
    _op("avgpool_global", F16, {"x": ((1, 5, 8), F16)}, [((8,), F32)], small=(0,), limits=[("waves", lambda B: B * 1, WAVE_ROWS_LIMIT)]),
    _op("avgpool_adaptive", BF16, {"x": ((3, 3, 8), BF16)}, [((2, 2, 8), BF16)]),
    # just under the launcher's limit rows = B L < 2^31 / 64 (scalar path, D % 512 != 0); the 16-byte path at the smallest batch
    _op("add_pos_layernorm-limit", F16, {"x": ((APL_L, 128), F16)}, [((APL_L, 128), F16), ((APL_L, 128), F16)], B=(ROWS_LIMIT - 1) // APL_L,
        limits=[("rows", lambda B: B * APL_L, ROWS_LIMIT)]),
    _op("add_pos_layernorm-vec", BF16, {"x": ((1, 512), BF16)}, [((1, 512), BF16), ((1, 512), BF16)], limits=[("rows", lambda B: B, ROWS_LIMIT)]),
    _op("mha_tokens", F16, {"qkv": ((3, 384), F16)}, [((3, 128), F16)], limits=[("B H", lambda B: B, WG256_LIMIT)]),
    _op("mean_layernorm", BF16, {"t": ((2, 136), BF16)}, [((136,), F32)], limits=[("B", lambda B: B, WG256_LIMIT)]),
    _op("cnn_attention", F16, {"qkv": ((1, 1, 272), F16), "x": ((1, 1, 256), F16)}, [((1, 1, 256), F16), ((256,), F32)],
        limits=[("B", lambda B: B, WG256_LIMIT)]),
    _op("l2_normalize", BF16, {"x": ((64,), F32)}, [((64,), F32)], limits=[("rows", lambda B: B, WAVE_ROWS_LIMIT)]),
    _op("pairwise_distance", F16, {"a": ((64,), F32), "b": ((64,), F32)}, [((), F32), ((), I32)], small=(0, 1),
        limits=[("rows", lambda B: B, WAVE_ROWS_LIMIT)]),
    _op("linear_f32", BF16, {"x": ((516,), F32)}, [((516,), F32)], limits=[("rows", lambda B: B, GEMM_ROWS_LIMIT)]),
]


def _nbytes(shape, dtype):
    return int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()


def op_operands(op):
    """(the large operands, every tensor) of a `BigOp` as `Operand`s."""
    es = lambda d: torch.empty((), dtype=d).element_size()
    ins = [Operand(n, _nbytes(s, d), es(d)) for n, (s, d) in op.inputs.items()]
    outs = [Operand("out%d" % i, _nbytes(s, d), es(d)) for i, (s, d) in enumerate(op.outputs)]
    return ins + [o for i, o in enumerate(outs) if i not in op.small], ins + outs


def op_batch(op):
    return op.B if op.B is not None else smallest_batch(op_operands(op)[0])


def op_estimate(op, B):
    return estimate_bytes([B * o.item_bytes for o in op_operands(op)[1]], bands=2 * 2 ** 20)
