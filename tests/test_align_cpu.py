"""CPU: the host-checkable half of the aligned crops - the warp function the kernel runs (the same text, compiled for the CPU)
against the installed Pillow's `Image.rotate`, the host geometry of `frames` (eye rotation, Pillow's matrix, the reference's
margin rule) and the C ABI of the new entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from PIL import Image

import align_cases as ac
from frmap_amd import _lib, frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_rng = np.random.default_rng(20240917)
FRAMES = {hw: _rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in ((37, 53), (120, 97), (240, 320))}
_ROTATED = {}


def _pil_rotated(hw, angle, center):
    """Pillow's rotated frame, computed once per (frame, angle, centre) and shared by the tests."""
    key = (hw, angle, center)
    if key not in _ROTATED:
        a = ac.pil_rotate(FRAMES[hw], angle, center)
        a.setflags(write=False)
        _ROTATED[key] = a
    return _ROTATED[key]


def _warp_host(frame, m, roi, bgr=False, pitch=None):
    x1, y1, x2, y2 = roi
    H, W = frame.shape[:2]
    out = np.full((y2 - y1, x2 - x1, 3), 0xA5, np.uint8)
    m = np.ascontiguousarray(m, dtype=np.float64)
    rc = _lib.load().frmap_align_warp_host(frame.ctypes.data, H, W, frame.strides[0] if pitch is None else pitch, m.ctypes.data,
                                           x1, y1, x2, y2, int(bgr), out.ctypes.data)
    assert rc == 0, _lib.load().frmap_last_error()
    return out


def _rois(H, W):
    """The full frame, each corner, 1 x 1 (inside and in the last corner)."""
    return [(0, 0, W, H), (0, 0, W // 3, H // 2), (W - 17, 0, W, 11), (0, H - 9, 21, H), (W - W // 2, H - H // 3, W, H),
            (W // 2, H // 2, W // 2 + 1, H // 2 + 1), (W - 1, H - 1, W, H)]


@pytest.mark.parametrize("hw", list(FRAMES))
def test_warp_host_equals_pillow_rotate_on_every_byte(hw):
    """`frmap_align_warp_host` == `Image.rotate(angle, BILINEAR, center=c)` then crop, for every angle class and centres inside
    the frame, on a corner and outside it; the full frame, the corners and 1 x 1 boxes."""
    H, W = hw
    f = FRAMES[hw]
    for angle in ac.ANGLES:
        for center in ac.centers(H, W):
            want = _pil_rotated(hw, angle, center)
            m = frames.rotation_matrix(angle, center)
            for x1, y1, x2, y2 in _rois(H, W):
                got = _warp_host(f, m, (x1, y1, x2, y2))
                assert np.array_equal(got, want[y1:y2, x1:x2]), (hw, angle, center, (x1, y1, x2, y2))


def test_warp_host_bgr_padded_pitch_and_angle_zero():
    hw = (120, 97)
    H, W = hw
    f = FRAMES[hw]
    # BGR in, RGB out: the rotation acts per channel, so rotating the flipped frame must give Pillow's rotation of the RGB one
    bgr = np.ascontiguousarray(f[:, :, ::-1])
    for angle, center in ((-12.25, (W / 3.0, H * 0.61)), (171.3, (-15.5, H + 40.0)), (45.0, (W, H))):
        want = _pil_rotated(hw, angle, center)
        m = frames.rotation_matrix(angle, center)
        for roi in _rois(H, W):
            x1, y1, x2, y2 = roi
            assert np.array_equal(_warp_host(bgr, m, roi, bgr=True), want[y1:y2, x1:x2]), (angle, roi)
    # a view of a wider buffer: pitch > 3 W, the padding full of another value
    buf = np.full((H, W + 13, 3), 255, np.uint8)
    view = buf[:, 5:5 + W]
    view[:] = f
    assert view.strides[0] == 3 * (W + 13)
    for angle, center in ((3.7, (W // 2, H // 2)), (-90.0, (W - 10.5, 22.0)), (359.5, (0, 0))):
        want = _pil_rotated(hw, angle, center)
        m = frames.rotation_matrix(angle, center)
        for roi in _rois(H, W):
            x1, y1, x2, y2 = roi
            assert np.array_equal(_warp_host(view, m, roi), want[y1:y2, x1:x2]), (angle, roi)
    # angle 0: the plain slice, whatever the centre
    for center in ac.centers(H, W):
        m = frames.rotation_matrix(0.0, center)
        for roi in _rois(H, W):
            x1, y1, x2, y2 = roi
            assert np.array_equal(_warp_host(f, m, roi), f[y1:y2, x1:x2]), (center, roi)


def test_numpy_restatement_equals_pillow():
    """The restatement the tests' documentation rests on (align_cases.numpy_rotate) is Pillow's arithmetic."""
    hw = (37, 53)
    for angle in ac.ANGLES:
        for center in ac.centers(*hw):
            assert np.array_equal(ac.numpy_rotate(FRAMES[hw], ac.pil_matrix(angle, center)), _pil_rotated(hw, angle, center)), (angle, center)


def test_warp_host_rejects_bad_arguments():
    lib = _lib.load()
    f = FRAMES[(37, 53)]
    m = frames.rotation_matrix(10.0, (20, 20))
    out = np.zeros((37, 53, 3), np.uint8)
    call = lib.frmap_align_warp_host
    good = [f.ctypes.data, 37, 53, 3 * 53, m.ctypes.data, 0, 0, 53, 37, 0, out.ctypes.data]
    assert call(*good) == 0
    for pos in (0, 4, 10):                                               # null frame / matrix / out
        args = list(good)
        args[pos] = None
        assert call(*args) == -1 and b"null pointer" in lib.frmap_last_error()
    for roi in ((0, 0, 54, 37), (0, 0, 53, 38), (-1, 0, 53, 37), (0, -1, 53, 37), (5, 5, 5, 9), (5, 9, 8, 9)):
        args = list(good)
        args[5:9] = roi
        assert call(*args) == -1 and b"empty or leaves" in lib.frmap_last_error(), roi
    args = list(good)
    args[3] = 3 * 53 - 1                                                 # pitch below a row
    assert call(*args) == -1
    for bad in (np.nan, np.inf, -np.inf):
        mb = m.copy()
        mb[4] = bad
        args = list(good)
        args[4] = mb.ctypes.data
        assert call(*args) == -1 and b"not finite" in lib.frmap_last_error()


@pytest.mark.parametrize("hw", [(37, 53), (120, 97)])
def test_rotation_matrix_is_pillows(hw):
    """`Image.transform(size, AFFINE, rotation_matrix(...), BILINEAR)` == `Image.rotate(...)`: the matrix is the one Pillow builds,
    the `% 360.0` and the 15-decimal rounding included."""
    H, W = hw
    im = Image.fromarray(FRAMES[hw])
    for angle in ac.ANGLES:
        for center in ac.centers(H, W):
            m = frames.rotation_matrix(angle, center)
            assert m.dtype == np.float64 and m.shape == (6,)
            assert m.tolist() == ac.pil_matrix(angle, center)
            got = np.asarray(im.transform((W, H), Image.AFFINE, tuple(m.tolist()), Image.BILINEAR))
            assert np.array_equal(got, _pil_rotated(hw, angle, center)), (angle, center)
    # the rounding is visible: cos(90 degrees) is exactly 0 in the matrix, not 6e-17
    m = frames.rotation_matrix(90.0, (10, 10))
    assert m[0] == 0.0 and m[4] == 0.0 and m[1] == -1.0 and m[3] == 1.0
    assert frames.rotation_matrix(-400.0, (3, 4)).tolist() == frames.rotation_matrix(320.0, (3, 4)).tolist()


def _forward(m, p):
    """Where the rotation puts frame point p: the inverse of the output -> input matrix."""
    A = np.array([[m[0], m[1]], [m[3], m[4]]])
    return np.linalg.solve(A, np.asarray(p, np.float64) - np.array([m[2], m[5]]))


def test_eye_rotation_levels_the_eyes_about_their_centre():
    cases = [
        ((100.0, 120.0), (160.0, 150.0)),        # right eye lower: dY > 0
        ((100.0, 150.0), (160.0, 120.0)),        # right eye higher
        ((40.5, 60.25), (90.75, 61.0)),
        ((200.0, 100.0), (200.0, 170.0)),        # eyes on a vertical line
        ((160.0, 100.0), (100.0, 110.0)),        # "left" eye on the right: more than 90 degrees
    ]
    for le, re_ in cases:
        lm = np.array([le, re_, (130.0, 160.0), (110.0, 190.0), (150.0, 190.0)])
        angle, (cx, cy) = frames.eye_rotation(lm)
        assert angle == float(np.degrees(np.arctan2(re_[1] - le[1], re_[0] - le[0])))
        assert (cx, cy) == ((le[0] + re_[0]) // 2, (le[1] + re_[1]) // 2)
        m = frames.rotation_matrix(angle, (cx, cy))
        # the centre is a fixed point of the matrix
        assert abs(m[0] * cx + m[1] * cy + m[2] - cx) < 1e-9 and abs(m[3] * cx + m[4] * cy + m[5] - cy) < 1e-9
        # the eyes land on one row, left eye on the left, their distance kept: the tilt is removed, not doubled
        pl, pr = _forward(m, le), _forward(m, re_)
        assert abs(pl[1] - pr[1]) < 1e-9, (le, re_, pl, pr)
        assert pr[0] > pl[0] and abs((pr[0] - pl[0]) - np.hypot(re_[0] - le[0], re_[1] - le[1])) < 1e-9
    assert frames.eye_rotation(np.array([(100.0, 120.0), (160.0, 150.0)]))[0] > 0          # positive dY: positive angle
    # coincident eyes: angle 0
    angle, center = frames.eye_rotation(np.array([(50.5, 60.5), (50.5, 60.5)]))
    assert angle == 0.0 and center == (50.0, 60.0)
    # the `// 2` is a floor: half-integer and negative sums
    assert frames.eye_rotation(np.array([(10.0, 20.0), (13.0, 25.0)]))[1] == (11.0, 22.0)          # 23 // 2, 45 // 2
    assert frames.eye_rotation(np.array([(10.25, 20.5), (12.25, 24.0)]))[1] == (11.0, 22.0)        # 22.5 // 2, 44.5 // 2
    assert frames.eye_rotation(np.array([(-10.0, -3.0), (3.0, 0.0)]))[1] == (-4.0, -2.0)           # -7 // 2, -3 // 2: toward -inf
    assert frames.eye_rotation(np.array([(-0.5, -0.25), (0.0, 0.0)]))[1] == (-1.0, -1.0)
    # lists, float32 and more points than two are taken; fewer than two are not
    assert frames.eye_rotation([[1, 2], [5, 2], [3, 4]]) == (0.0, (3.0, 2.0))
    assert frames.eye_rotation(np.array([[1, 2], [5, 6]], np.float32))[0] == 45.0
    with pytest.raises(ValueError):
        frames.eye_rotation(np.array([[1.0, 2.0]]))


def _reference_margin(bbox, margin, img_shape):
    """`src/data_prep.py:89-106` restated literally."""
    height, width = img_shape[:2]
    x1, y1, x2, y2 = bbox
    width = x2 - x1
    height = y2 - y1
    margin_x = int(width * margin)
    margin_y = int(height * margin)
    x1 = max(0, x1 - margin_x)
    y1 = max(0, y1 - margin_y)
    x2 = min(img_shape[1], x2 + margin_x)
    y2 = min(img_shape[0], y2 + margin_y)
    return np.array([x1, y1, x2, y2])


def test_margin_boxes_is_the_references_rule():
    H, W = 360, 480
    boxes = np.array([
        [100.0, 50.0, 300.0, 250.0],           # plain
        [-20.5, 40.2, 90.9, 180.1],            # leaves on the left
        [400.0, 100.0, 520.0, 220.0],          # on the right
        [200.3, -30.7, 280.6, 60.0],           # at the top
        [150.0, 300.0, 260.0, 400.0],          # at the bottom
        [10.999999, 20.999999, 30.999999, 40.999999],
        [33.3, 44.4, 77.7, 99.9],              # fractional: int(width * margin) truncates
        [5.0, 5.0, 9.9, 9.9],                  # margin below one pixel
        [0.0, 0.0, 480.0, 360.0],              # the whole frame
        [-300.0, -300.0, 900.0, 900.0],        # larger than the frame
    ], dtype=np.float64)
    for margin in (0.0, 0.2, 1.0):
        got = frames.margin_boxes(boxes, margin, (H, W, 3))
        assert got.dtype == np.float64 and got.shape == boxes.shape
        want = np.stack([_reference_margin(b, margin, (H, W, 3)) for b in boxes])
        assert np.array_equal(got, want), margin
        assert np.array_equal(frames.margin_boxes(boxes.tolist(), margin, (H, W)), want)
    # what the comments say: 44.4 * 0.2 = 8.88 -> 8 pixels, not 9; clamped to the frame
    assert frames.margin_boxes(boxes[6:7], 0.2, (H, W))[0].tolist() == [33.3 - 8, 44.4 - 11, 77.7 + 8, 99.9 + 11]
    assert frames.margin_boxes(boxes[2:3], 0.2, (H, W))[0].tolist() == [376.0, 76.0, 480.0, 244.0]
    # margin 0 + clip_boxes == clip_boxes
    probs = np.array([0.99, 0.95, 0.91, 0.999, 0.93, 0.97, 0.5, 0.99, 0.99, 0.9])
    r0, k0 = frames.clip_boxes(boxes, probs, (H, W))
    r1, k1 = frames.clip_boxes(frames.margin_boxes(boxes, 0.0, (H, W)), probs, (H, W))
    assert np.array_equal(r0, r1) and np.array_equal(k0, k1) and len(k0) == 9
    # no boxes
    assert frames.margin_boxes(None, 0.2, (H, W)) is None
    assert frames.margin_boxes(np.zeros((0, 4)), 0.2, (H, W)).shape == (0, 4)


def test_align_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_align_crop_resize_u8", 12), ("frmap_align_warp_host", 11)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % sym, header)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
        assert hasattr(_lib.load(), sym)
    assert _lib.ABI_VERSION == 10 and _lib.load().frmap_abi_version() == 10
    assert C.sizeof(C.c_double) == 8
