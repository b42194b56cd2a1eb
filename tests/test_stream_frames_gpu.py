"""GPU: stream order of resize and the four crop entry points (`stream_cases.py`), late rule only.

Every two-fill test of `test_guard_frames_gpu.py` and `test_guard_yuv_gpu.py` (packed and 4:2:0 frames, plain and eye-aligned crops,
the tall-ROI route through `resize_bilinear_u8`, the batched resize) runs again with its frames late on a side stream, then with
the default stream blocked, and goes on to its own comparison with Pillow.  These wrappers build their record and tap tables on
the host and upload them with a blocking copy per call: they are declared uncapturable (`stream_cases.CAPTURABLE`), and because
that upload waits for the stream, variant (a) holds them to "the delay was running when each frame was handed over"
(`stream_cases.SYNCS`).  The tests of records that break the contract use the guard directly and stay where they are.
"""
import pytest

pytestmark = pytest.mark.gpu

import stream_cases as sc  # noqa: E402
import test_guard_frames_gpu as tf  # noqa: E402
import test_guard_yuv_gpu as ty  # noqa: E402

FRAME_TESTS = ["test_crop_resize", "test_crop_resize_tall_roi_and_batched_resize", "test_align_crop", "test_align_crop_tall_roi"]
YUV_TESTS = ["test_crop_resize_yuv", "test_align_crop_yuv", "test_tall_roi_of_a_yuv_frame"]
MIRRORED = FRAME_TESTS + YUV_TESTS

for _mod, _names in ((tf, FRAME_TESTS), (ty, YUV_TESTS)):
    for _name in _names:
        assert sc.CAPTURABLE[_name] is not True
        globals()[_name + "_late"] = sc.mirror_late(_mod, _name)


def test_stream_report(capsys):
    assert sc.CALLS["late"] > 0
    with capsys.disabled():
        print("\n[test_stream_frames_gpu] " + sc.report(MIRRORED))
