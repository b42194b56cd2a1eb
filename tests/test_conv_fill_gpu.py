"""GPU: the planner's fill step (`conv_fill`, csrc/conv_plan.cpp) changes which pixels share a tile and nothing else.

Each case runs twice through the op wrappers (`conv_cases.run_case`): with the planner's own tile - filled to the layout's
capacity, so tiles straddle images (up to three 14x14 images in one 224-pixel tile) - and with the tile forced to the
image-aligned size of the commit before through `frmap_conv_pp_tuning`.  The 224 px x 256 ch layouts keep the image-aligned tile
by default (measured no faster filled): there the first run forces the size the fill step would pick (224 px; 210 px
at stride 2) through the same hook, so the kernels are held to the same rule in every layout.  The two outputs must be `torch.equal`: every output element keeps
its k order.  The filled output must also meet the one-rounding bound of `conv_cases.py` against the float64 CPU reference (on the
rounded operands), and pass the guard-band rule of `guard.py` (all of the output written, nothing else, no byte read from
outside the operands).  The batches are small, so the layouts are forced on through the same hook (the default tile-count gates
would send these batches to the first generation); sizes are chosen so that the last tile is partial in every case.  `frmap_conv3x3_pp_tile_px` tells which tile a launch uses.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_cases as cc  # noqa: E402
import guard  # noqa: E402
from frmap_amd import _lib, ops  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]

# (case, filled tile, image-aligned tile, tile the planner picks by itself, key of the filled run, key of the image-aligned run: the
# kernel instantiations `ops.conv_plan_key` names - a larger tile can take more halo pieces).  tune = (1, -1, bn): layout forced on,
# tile left to the planner.
_c = cc._c
FILL_CASES = [
    # 224 x 256 layout: 1764 px = 7.875 tiles of 224, up to three images per tile
    (_c("fill-224x256-res", cc.PP, "conv", 9, 14, 14, 128, 256, res=True, tune=(1, -1, 256), query=("conv3x3_pp", (1,))), 224, 196, 196, "conv3x3_pp_kernel<7,2,3,1>", "conv3x3_pp_kernel<7,2,3,1>"),
    # 448 x 128 layout: 3920 px = 8.75 tiles of 448
    (_c("fill-448x128", cc.PP, "conv", 5, 28, 28, 128, 128, act=cc.ACT_NONE, tune=(1, -1, 128), query=("conv3x3_pp", (2,))), 448, 392, 448, "conv3x3_pp_kernel<7,4,5,1>", "conv3x3_pp_kernel<7,4,5,1>"),
    (_c("fill-448x128-res", cc.PP, "conv", 5, 28, 28, 128, 128, res=True, tune=(1, -1, 128), query=("conv3x3_pp", (2,))), 448, 392, 448, "conv3x3_pp_kernel<7,4,5,1>", "conv3x3_pp_kernel<7,4,5,1>"),
    # split-K 224 x 128: six halo pieces in place of four
    (_c("fill-splitk", cc.PP, "conv", 9, 14, 14, 256, 256, tune=(1, -1, 1282), query=("conv3x3_pp", (3,))), 224, 196, 224, "conv3x3_pp_kernel<7,2,6,2>", "conv3x3_pp_kernel<7,2,4,2>"),
    # fused shortcut from a 28x28x128 map (224 x 256) and from a 56x56x64 map (448 x 128), stride 2
    (_c("fill-shortcut-14", cc.PP, "ds", 9, 14, 14, 256, 256, ds=(128, 2), tune=(1, -1, 256), query=("conv3x3_pp_ds", (1,))), 224, 196, 196, "conv3x3_pp_kernel<7,2,3,1,DS>", "conv3x3_pp_kernel<7,2,3,1,DS>"),
    (_c("fill-shortcut-28", cc.PP, "ds", 5, 28, 28, 128, 128, ds=(64, 2), tune=(1, -1, 128), query=("conv3x3_pp_ds", (2,))), 448, 392, 448, "conv3x3_pp_kernel<7,4,5,1,DS>", "conv3x3_pp_kernel<7,4,5,1,DS>"),
    # stride 2, 28x28x128 -> 14x14x256 (224 x 256 layout): 15 rows are the largest tile whose halo fits the two 8 KB pieces there are
    # stride 2, 56x56x64 -> 28x28x128 (448 x 128 layout, filled by default): 15 rows = 420 px, 3920 px = 9.33 tiles
    (_c("fill-stride2-448x128", cc.PP, "conv", 5, 56, 56, 64, 128, stride=2, tune=(1, -1, 128), query=("conv3x3s2_pp", (2,))), 420, 392, 420, "conv3x3s2_pp_kernel<7,4,4>", "conv3x3s2_pp_kernel<7,4,4>"),
    (_c("fill-stride2", cc.PP, "conv", 9, 28, 28, 128, 256, stride=2, tune=(1, -1, 256), query=("conv3x3s2_pp", (1,))), 210, 196, 196, "conv3x3s2_pp_kernel<7,2,2>", "conv3x3s2_pp_kernel<7,2,2>"),
]


def _tile_px(lib, case):
    ds = (2 * case.H, 2 * case.W, case.ds[0], case.ds[1]) if case.ds is not None else (0, 0, 0, 0)
    return lib.frmap_conv3x3_pp_tile_px(case.B, case.H, case.W, case.Cin, case.Cout, case.stride, *ds)


def _planned_tile(case, px):
    """tile of the launch under the case's layout with tile size `px` forced (-1: the planner's own); hooks reset."""
    lib = _lib.load()
    try:
        lib.frmap_conv_pp_tuning(case.tune[0], px, case.tune[2])
        return _tile_px(lib, case)
    finally:
        lib.frmap_conv_pp_tuning(-1, -1, -1)


def fill_runs(entry):
    """(case of the filled run, case of the image-aligned run) of a FILL_CASES entry, each with its tile and its key."""
    case, filled_px, aligned_px, own_px, key_filled, key_aligned = entry
    first = case._replace(key=key_filled)
    if own_px != filled_px:                    # a layout the fill step skips: the filled size through the hook
        first = first._replace(tune=(case.tune[0], filled_px, case.tune[2]))
    return first, case._replace(tune=(case.tune[0], aligned_px, case.tune[2]), key=key_aligned)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("entry", FILL_CASES, ids=[c[0].name for c in FILL_CASES])
def test_filled_tiles_compute_what_image_aligned_tiles_compute(entry, dtype):
    case, filled_px, aligned_px, own_px = entry[:4]
    assert _planned_tile(case, -1) == own_px, (case.name, "the planner's own tile", _planned_tile(case, -1), "expected", own_px)
    assert _planned_tile(case, aligned_px) == aligned_px, (case.name, "the hook did not force the image-aligned tile")
    case, aligned = fill_runs(entry)           # (a layout the fill step skips: the filled size through the hook)
    own = _planned_tile(case, case.tune[1])
    assert own == filled_px, (case.name, "tile of the first run", own, "expected", filled_px)
    Ho, Wo = case.H // case.stride, case.W // case.stride
    M = case.B * Ho * Wo
    assert own % Wo == 0 and (Ho * Wo) % own != 0 and own % (Ho * Wo) != 0, (case.name, "whole rows, and tiles that straddle images")
    assert M % own, (case.name, "the last tile is not partial")

    seed = 8300 + 13 * [c[0].name for c in FILL_CASES].index(case.name)
    o = cc.float_operands("gauss", seed, case.B, case.H, case.W, case.Cin, case.Cout, 3, dtype, case.stride, 1, case.res, case.ds)
    want, S, act = cc.case_reference(case, o)
    # the filled run, three times between guard bands (unguarded, 0xFF, 0x5A): same bits, bands untouched
    y, = guard.two_fills(lambda place: cc.run_case(case, o, dtype, place=place), [ops], what=case.name)
    # the image-aligned run
    try:
        y0 = cc.run_case(aligned, o, dtype)
    finally:
        cc.reset_hooks(_lib.load())
    assert y.dtype == dtype and y0.dtype == dtype
    d = guard.first_difference(y.contiguous(), y0.contiguous())
    assert torch.equal(y, y0), f"{case.name}: tiles of {own} px and of {aligned_px} px differ: {d}"
    print(f"CONVFILL {str(dtype)[6:]} {case.name} tile {own} against {aligned_px}: "
          f"{cc.one_rounding_ratio(y, cc.act64(want, act), S, dtype):.3f} of the bound")
    cc.assert_one_rounding(y, want, S, dtype, act, f"{case.name} {str(dtype)[6:]}")


def test_switch_and_hooks_are_back_at_their_defaults():
    """After the cases above the default queries answer as planned (no hook left set)."""
    lib = _lib.load()
    assert lib.frmap_conv3x3_pp_tile_px(256, 14, 14, 256, 256, 1, 0, 0, 0, 0) == 196      # 224 x 256: not filled
    assert lib.frmap_conv3x3_pp_tile_px(128, 14, 14, 256, 256, 1, 0, 0, 0, 0) == 224      # split-K: filled
    assert lib.frmap_conv3x3_pp_tile_px(128, 28, 28, 128, 128, 1, 56, 56, 64, 2) == 448   # 448 x 128 with the shortcut: filled
    assert lib.frmap_conv3x3_pp_tile_px(128, 56, 56, 64, 128, 2, 0, 0, 0, 0) == 420       # stride 2, 448 x 128: 15 rows
    assert lib.frmap_conv3x3_pp_layout(256, 14, 14, 256, 256) == 1
