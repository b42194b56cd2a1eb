"""GPU: the seam of the shared crop body (csrc/crop_device.h) - every source of pixels (packed, packed + warp, YUV, YUV + warp)
crossed with every copy / resample branch of the two passes, at the smallest shapes where they can go wrong: one 37 x 53 picture
(odd both ways, one workgroup and several), ROIs down to 1 x 1, output sizes that resample both axes, copy one, copy both and
enlarge.  Every assertion is exact equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import align_cases as ac  # noqa: E402
import yuv_cases as yc  # noqa: E402
from frmap_amd import frames, resize  # noqa: E402

DEV = "cuda"
H, W = 37, 53
ROIS = [(0, 0, W, H), (52, 36, 53, 37), (26, 18, 53, 37), (0, 0, 53, 8), (5, 0, 13, 37)]
# both axes resampled; both copied for the whole frame; width copied for the full-width ROIs; height copied for the full-height
# ones; enlarging
SIZES = [(8, 8), (37, 53), (8, 53), (37, 8), (40, 60)]
TILT, CENTER = 20.0, (26, 18)
RGB = np.random.default_rng(20251103).integers(0, 256, (H, W, 3), dtype=np.uint8)
RGB.setflags(write=False)


@pytest.fixture(scope="module")
def held():
    """The picture on the device as RGB, as BGR and as a view with padded pitch; the I420 and NV12 frames of random planes, and
    their conversion as a packed device frame."""
    rgb = torch.from_numpy(RGB.copy()).to(DEV)
    wide = torch.full((H, W + 9, 3), 0xC3, dtype=torch.uint8, device=DEV)
    wide[:, 4:4 + W] = rgb
    return {"rgb": rgb, "bgr": rgb.flip(2).contiguous(), "padded": wide[:, 4:4 + W],
            "yuv": [yc.frame(fmt, H, W, 0, device=DEV) for fmt in ("i420", "nv12")],
            "converted": torch.from_numpy(yc.rgb(H, W, 0).copy()).to(DEV)}


def _same(a, b):
    return torch.equal(a, b) if isinstance(b, torch.Tensor) else np.array_equal(a.cpu().numpy(), b)


@pytest.mark.parametrize("size", SIZES)
def test_plain_sources(held, size):
    rois = np.array(ROIS)
    got = resize.crop_resize_u8(held["rgb"], rois, size, device=DEV)
    assert held["padded"].stride(0) > 3 * W and tuple(got.shape) == (len(ROIS), *size, 3)
    for i, roi in enumerate(ROIS):
        assert _same(got[i], ac.pil_crop(RGB, roi, *size)), roi
    assert _same(resize.crop_resize_u8(held["bgr"], rois, size, bgr=True, device=DEV), got)
    assert _same(resize.crop_resize_u8(held["padded"], rois, size, device=DEV), got)
    want = resize.crop_resize_u8(held["converted"], rois, size, device=DEV)
    for f in held["yuv"]:
        assert _same(resize.crop_resize_u8(f, rois, size, device=DEV), want), f


@pytest.mark.parametrize("size", SIZES)
def test_warped_sources(held, size):
    rois = np.array(ROIS)
    eye = np.tile(np.array(frames.rotation_matrix(0.0, CENTER), np.float64), (len(ROIS), 1))
    tilt = np.tile(np.array(frames.rotation_matrix(TILT, CENTER), np.float64), (len(ROIS), 1))
    assert eye[0].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert _same(resize.align_crop_resize_u8(held["rgb"], rois, eye, size, device=DEV), resize.crop_resize_u8(held["rgb"], rois, size, device=DEV))
    got = resize.align_crop_resize_u8(held["rgb"], rois, tilt, size, device=DEV)
    for i, roi in enumerate(ROIS):
        assert _same(got[i], ac.pil_chain(RGB, TILT, CENTER, roi, *size)), roi
    assert _same(resize.align_crop_resize_u8(held["bgr"], rois, tilt, size, bgr=True, device=DEV), got)
    assert _same(resize.align_crop_resize_u8(held["padded"], rois, tilt, size, device=DEV), got)
    for m in (eye, tilt):
        want = resize.align_crop_resize_u8(held["converted"], rois, m, size, device=DEV)
        for f in held["yuv"]:
            assert _same(resize.align_crop_resize_u8(f, rois, m, size, device=DEV), want), f
    for f in held["yuv"]:                                                   # the identity through the YUV warp is the plain YUV crop
        assert _same(resize.align_crop_resize_u8(f, rois, eye, size, device=DEV), resize.crop_resize_u8(f, rois, size, device=DEV)), f
