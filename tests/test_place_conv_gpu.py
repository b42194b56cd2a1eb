"""GPU: the conv family where its buffers start (`guard.shifted`, `place_cases.py`).

Every test of `test_guard_conv_gpu.py` - every entry of `conv_cases.CONV_CASES`, `GELU_CASES` and `LINEAR_CASES` through
`cc.run_case` / `cc.run_linear`, and the two weight packers, in fp16 and bf16 - runs again with every operand, output and workspace
"aligned to A and not to 2 A" for the A of `place_cases.requirement` (16 bytes for every tensor, `shift` vector and split-K slab of
this family, 4 for the uint8 stem image), under both fills; bands untouched, bits those of the aligned call.  No entry of the tables
is left out: they are already one case per kernel variant, layout and form, and each `Case.query` asserts the planner's answer
(`frmap_conv3x3_pp_layout`, `frmap_conv3x3s2_pp_layout`, `frmap_conv3x3_pp_ds_layout`, `frmap_conv1x1_pp_layout`,
`frmap_conv_igemm_pool2_form`) inside `launch_case`, shifted or not, so every kernel symbol and planner layout the tables name is
hit with shifted pointers.  No kernel here changes its summation order with alignment: there is no exception to the bit rule.
The same tests run once more with every placed operand - activations, residuals, shortcut inputs, fp32 weights for the packers,
`shift`, the stem images - a contiguous view one element into its allocation: the binding copies what is below its argument's
requirement (each copy kept until the launch) and the result holds the bits of the call on clones.

Then the path choices that depend on the pointer itself, each compared with the aligned call bit for bit and with fp32 torch on the
same rounded operands (`test_kernels_gpu.py::test_fused_stem_maxpool`'s reference and tolerance):
  * the fp32 stems on an image with W % 4 == 0 at 16-byte alignment (16-byte staging loads; `stem_s2d_kernel` for the 3x3 pool) and
    at 4-byte alignment, where `frmap_stem_s2d` declines the tensor and `stem_pool_kernel` stages it pixel by pixel;
  * the uint8 stems at 4-byte alignment, the least they take.
ONE EXCEPTION to the bit rule, found by the first GPU run of this file: `frmap_stem7x7_maxpool` (3x3 pool) on a W % 4 == 0 image
that is 4- but not 16-byte aligned.  The aligned call runs `stem_s2d_kernel`, whose K axis is the space-to-depth one; the other
runs `stem_pool_kernel`, whose K axis runs along (kw, c) of a kernel row: the same products summed in another order, 3 of 18432
fp16 outputs one unit in the last place apart at 2 x 61 x 36.  That case meets the bits of the same call on an unguarded tensor at
4 bytes instead, and both results lie within `test_kernels_gpu.py::test_fused_stem_maxpool`'s bound (2e-3 fp16, 1.6e-2 bf16).  The
2x2-pool stem has one kernel for both alignments (16-byte or pixel-wise staging of the same rows): bits equal, no exception.
Which kernel ran is not observable through this entry point; `test_place_model_gpu.py` reads it from `frmap_model_trace`.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import place_cases as pc  # noqa: E402
import conv_cases as cc  # noqa: E402
import test_guard_conv_gpu as tg  # noqa: E402
from frmap_amd import ops, synth  # noqa: E402

DEV = "cuda"

for _name in ("test_conv_case_is_guarded", "test_gelu_case_is_guarded", "test_linear_case_is_guarded", "test_pack_conv_weight_is_guarded",
              "test_pack_conv_weight_c3_is_guarded"):
    globals()[_name.replace("_is_guarded", "_at_minimum_alignment")] = pc.mirror(tg, _name)
    if _name not in ("test_conv_case_is_guarded", "test_linear_case_is_guarded"):
        globals()[_name.replace("_is_guarded", "_on_offset_views")] = pc.mirror_offset(tg, _name)

# (every conv case but the one that IS the exception below: the fp32 3x3-pool stem on a W % 4 == 0 image, whose view at 4 bytes runs
#  the other stem kernel; `test_fp32_stem_takes_its_path_from_the_pointer` holds it to the call at the same alignment)
OFFSET_CASES = [c for c in cc.CONV_CASES if c.name != "stem-s2d-pool3"]


@pytest.mark.parametrize("dtype", tg.DTYPES, ids=tg.DT_IDS)
@pytest.mark.parametrize("lc", cc.LINEAR_CASES, ids=[c.name for c in cc.LINEAR_CASES])
def test_linear_case_on_offset_views(lc, dtype):
    """(the guard test also counts the guard's allocations, which views do not have: `cc.run_linear` under the rule itself)"""
    o = cc.linear_operands(lc, "gauss" if lc.act == cc.ACT_GELU else "exact", dtype)
    pc.offset_rule(lambda place: cc.run_linear(lc, o, dtype, place=place), what=lc.name)


@pytest.mark.parametrize("dtype", tg.DTYPES, ids=tg.DT_IDS)
@pytest.mark.parametrize("case", OFFSET_CASES, ids=[c.name for c in OFFSET_CASES])
def test_conv_case_on_offset_views(case, dtype):
    with pc.on_offset_views():
        tg.test_conv_case_is_guarded(case, dtype)


def _tol(dtype):      # test_kernels_gpu.py's: one rounding of the output to the storage dtype + fp32 accumulation noise
    return (2e-3, 2e-3) if dtype == torch.float16 else (1.6e-2, 1.6e-2)


def _stem_operands(dtype, pool3, B=2, H=61, W=36):
    x = synth.randn(25, (B, 3, H, W), "x")
    w = (synth.randn(26, (64, 3, 7, 7), "w") * math.sqrt(2.0 / 147)).to(dtype)
    shift = synth.randn(27, (64,), "b") * 0.3
    conv = F.relu(F.conv2d(x.to(dtype).float(), w.float(), None, stride=2, padding=3) + shift.view(1, -1, 1, 1))
    ref = F.max_pool2d(conv.to(dtype).float(), 3, 2, 1) if pool3 else F.max_pool2d(conv.to(dtype).float(), 2, 2)
    return x, w, shift, ref


def _placed_runs(x_cpu, need, call):
    """`call(x on the device)` with x aligned to `need` and not to 2 `need`, under both fills; everything the wrapper allocates at its
    own minimum alignment.  Returns the two outputs (CPU)."""
    outs = []
    for fill in guard.FILLS:
        g = guard.Guard(fill, shift=guard.min_placement(lambda d, kind, who: need if kind == "operand" else pc.requirement(d, kind, who)))
        with g.patch(ops):
            xd = g.place(x_cpu)
            assert xd.data_ptr() % (2 * need) == need
            y = call(xd)
        g.check()
        outs.append(y.cpu())
    return outs


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("pool3", [True, False], ids=["pool3", "pool2"])
@pytest.mark.parametrize("need", [16, 4], ids=["x-at-16-vector-staging", "x-at-4-scalar-staging"])
def test_fp32_stem_takes_its_path_from_the_pointer(need, pool3, dtype):
    x, w, shift, ref = _stem_operands(dtype, pool3)
    wpk, sh = ops.pack_conv_weight_c3(w.float().to(DEV), dtype), shift.to(DEV)
    y0 = ops.stem7x7_maxpool(x.to(DEV), wpk, sh, dtype, pool3=pool3).cpu()
    if need == 4 and pool3:
        # THE EXCEPTION (module docstring): another kernel, another summation order.  The bits to meet are those of the same call on
        # an unguarded tensor at 4 bytes (`flat[1:]`), and both kernels' results lie within the reference's bound.
        xo = pc.offset_view(x, DEV)
        assert xo.data_ptr() % 8 == 4
        y4 = ops.stem7x7_maxpool(xo, wpk, sh, dtype, pool3=True).cpu()
    else:
        y4 = y0
    for y in _placed_runs(x, need, lambda xd: ops.stem7x7_maxpool(xd, wpk, sh, dtype, pool3=pool3)):
        assert guard.first_difference(y, y4) is None, guard.first_difference(y, y4)
    atol, rtol = _tol(dtype)             # test_kernels_gpu.py::test_fused_stem_maxpool / test_fused_stem_maxpool2x2
    for got in (y0.float().permute(0, 3, 1, 2), y4.float().permute(0, 3, 1, 2)):
        assert got.shape == ref.shape and torch.allclose(got, ref, atol=atol, rtol=rtol), (got - ref).abs().max()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("pool3", [True, False], ids=["pool3", "pool2"])
def test_u8_stem_at_four_bytes(pool3, dtype):
    B, H, W = 2, 61, 36
    g = torch.Generator().manual_seed(128)
    x8 = torch.randint(0, 256, (B, H, W, 3), generator=g).to(torch.uint8)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    _, w, shift, _ = _stem_operands(dtype, pool3)
    wpk, sh = ops.pack_conv_weight_c3(w.float().to(DEV), dtype), shift.to(DEV)
    y0 = ops.stem7x7_maxpool_u8(x8.to(DEV), wpk, sh, mean, std, dtype, pool3=pool3).cpu()
    for y in _placed_runs(x8, 4, lambda xd: ops.stem7x7_maxpool_u8(xd, wpk, sh, mean, std, dtype, pool3=pool3)):
        assert guard.first_difference(y, y0) is None, guard.first_difference(y, y0)
    # the fp32 entry on the normalised image rounded to `dtype`: the same bits (test_kernels_gpu.py's uint8 twin), hence the same reference
    xf = ops.normalize_u8(x8.to(DEV), mean, std)[0]
    assert torch.equal(ops.stem7x7_maxpool(xf.to(dtype).float(), wpk, sh, dtype, pool3=pool3).cpu(), y0)
    xr = xf.to(dtype).float().cpu()
    conv = F.relu(F.conv2d(xr, w.float(), None, stride=2, padding=3) + shift.view(1, -1, 1, 1))
    ref = F.max_pool2d(conv.to(dtype).float(), 3, 2, 1) if pool3 else F.max_pool2d(conv.to(dtype).float(), 2, 2)
    atol, rtol = _tol(dtype)
    assert torch.allclose(y0.float().permute(0, 3, 1, 2), ref, atol=atol, rtol=rtol)
