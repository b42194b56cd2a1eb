"""GPU: resize and the four crop entry points where their buffers start.

Every two-fill test of `test_guard_frames_gpu.py` and `test_guard_yuv_gpu.py` (packed and 4:2:0 frames, plain and eye-aligned
crops, the tall-ROI route through `resize_bilinear_u8`, the batched resize) runs again
  * under `guard.shifted`: the frames (uint8 operands) aligned to 4 bytes and not to 8, the crops and resized images the wrappers
    allocate to 1 byte and not to 2 - these kernels are byte-addressed through `src_pool`, the planes a frame record names and
    `out`; the record tables (`frames` | `mats` | `rois` in one upload, `items`, `tables`) are the wrapper's own uploads, whose
    8-byte records and float64 matrices the launchers now check - and
  * with every frame a view one BYTE into its allocation (`flat[1:1 + n].view(shape)` of a uint8 tensor),
and gives the bits of the aligned call, which those tests go on to compare with Pillow.  The tests of records that break the
contract and the positive controls use the guard directly and stay where they are.
"""
import pytest

pytestmark = pytest.mark.gpu

import place_cases as pc  # noqa: E402
import test_guard_frames_gpu as tf  # noqa: E402
import test_guard_yuv_gpu as ty  # noqa: E402

FRAME_TESTS = ["test_crop_resize", "test_crop_resize_tall_roi_and_batched_resize", "test_align_crop", "test_align_crop_tall_roi"]
YUV_TESTS = ["test_crop_resize_yuv", "test_align_crop_yuv", "test_tall_roi_of_a_yuv_frame"]

for _mod, _names, _tag in ((tf, FRAME_TESTS, ""), (ty, YUV_TESTS, "")):
    for _name in _names:
        globals()[_name + "_at_minimum_alignment"] = pc.mirror(_mod, _name)
        globals()[_name + "_on_offset_views"] = pc.mirror_offset(_mod, _name)
