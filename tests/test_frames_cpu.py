"""CPU: the host-checkable half of the frame front end - the filter-tap function the crop kernel runs (the same text, compiled for
the CPU), the reference's box rule, and the C ABI of the new entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from frmap_amd import _lib, frames, resize
from oracle import pil_resize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_coeffs(lib, in_size, out_size):
    ks = C.c_int(-1)
    assert lib.frmap_resize_coeffs_host(in_size, out_size, None, None, C.byref(ks)) == 0
    b = np.full((out_size, 2), -1, np.int32)
    k = np.full((out_size, ks.value), -1, np.int32)
    assert lib.frmap_resize_coeffs_host(in_size, out_size, b.ctypes.data, k.ctypes.data, None) == 0
    return b, k


@pytest.mark.parametrize("out_size", [1, 7, 112, 160, 224, 299])
def test_resize_coeffs_host_equals_pillow_tables(out_size):
    """`frmap_resize_coeffs_host` (resize_coeffs.h, the function the crop kernel calls on the device) == `resize.bilinear_coeffs`
    == the oracle's restatement of Pillow's precompute_coeffs + normalize_coeffs_8bpc, exactly, for every input size 1 .. 1300."""
    lib = _lib.load()
    for in_size in range(1, 1301):
        b, k = _host_coeffs(lib, in_size, out_size)
        rb, rk = resize.bilinear_coeffs(in_size, out_size)
        assert k.shape == rk.shape and np.array_equal(b, rb) and np.array_equal(k, rk), (in_size, out_size)
        ob, ok = pil_resize.precompute_coeffs(in_size, out_size)
        assert k.shape == ok.shape and np.array_equal(b, ob) and np.array_equal(k, ok), (in_size, out_size)


def test_resize_coeffs_host_rejects_bad_sizes():
    lib = _lib.load()
    ks = C.c_int()
    assert lib.frmap_resize_coeffs_host(0, 160, None, None, C.byref(ks)) == -1
    assert lib.frmap_resize_coeffs_host(10, 0, None, None, C.byref(ks)) == -1
    assert b"resize_coeffs_host" in lib.frmap_last_error()
    b = np.zeros((4, 2), np.int32)
    assert lib.frmap_resize_coeffs_host(10, 4, b.ctypes.data, None, C.byref(ks)) == -1


def _reference_rule(boxes, probs, frame_shape, det_thresh=0.9):
    """`src/app.py:190-200` restated literally (DET_THRESH = 0.9, `:18`)."""
    rois, kept = [], []
    for i, (box, prob) in enumerate(zip(boxes, probs)):
        if prob < det_thresh:
            continue
        x1, y1, x2, y2 = [int(b) for b in box]
        x1, y1 = max(0, x1), max(0, y1)
        x2, y2 = min(frame_shape[1], x2), min(frame_shape[0], y2)
        if x2 <= x1 or y2 <= y1:
            continue
        rois.append([x1, y1, x2, y2])
        kept.append(i)
    return rois, kept


def test_clip_boxes_is_the_references_rule():
    H, W = 720, 1280
    boxes = np.array([
        [100.0, 50.0, 300.0, 400.0],          # plain
        [-20.5, -3.2, 90.9, 80.1],            # negative corner: clamped to 0
        [1200.0, 600.0, 1400.0, 900.0],       # leaves the frame on the right / bottom: clamped to W / H
        [10.999999, 20.999999, 30.999999, 40.999999],   # just below integers: truncated down
        [-0.9, -0.999, 50.0, 60.0],           # negative fractions: int() gives 0 (toward zero), floor would give -1
        [-1.5, 5.0, -0.5, 50.0],              # int(-0.5) = 0, int(-1.5) = -1 -> x1 = x2 = 0: dropped (floor would differ)
        [200.0, 200.0, 200.0, 300.0],         # zero width
        [200.0, 300.0, 260.0, 300.9],         # zero height after truncation
        [1300.0, 10.0, 1350.0, 60.0],         # wholly outside: x1 = 1300 > x2 = 1280
        [5.0, 5.0, 50.0, 50.0],               # prob exactly at the threshold: kept (the rule is prob < thresh)
        [5.0, 5.0, 50.0, 50.0],               # just below the threshold
        [5.0, 5.0, 50.0, 50.0],               # well below
        [0.0, 0.0, 1280.0, 720.0],            # the whole frame
        [400.7, 300.2, 401.3, 301.9],         # 1 x 1 after truncation
    ], dtype=np.float64)
    probs = np.array([0.99, 0.95, 0.91, 0.999, 0.93, 0.97, 0.99, 0.99, 0.99, 0.9, np.nextafter(0.9, 0.0), 0.2, 1.0, 0.96], dtype=np.float64)
    want_r, want_k = _reference_rule(boxes, probs, (H, W, 3))
    rois, kept = frames.clip_boxes(boxes, probs, (H, W, 3))
    assert rois.dtype == np.int32 and rois.shape == (len(want_r), 4)
    assert rois.tolist() == want_r and kept.tolist() == want_k
    # the listed cases did what their comments say
    assert want_k == [0, 1, 2, 3, 4, 9, 12, 13]
    assert rois[kept.tolist().index(4)].tolist() == [0, 0, 50, 60] and rois[kept.tolist().index(3)].tolist() == [10, 20, 30, 40]
    assert rois[kept.tolist().index(13)].tolist() == [400, 300, 401, 301]
    # lists of python floats, another threshold, no probabilities, no boxes
    r2, k2 = frames.clip_boxes(boxes.tolist(), probs.tolist(), (H, W), det_thresh=0.5)
    w2 = _reference_rule(boxes.tolist(), probs.tolist(), (H, W), 0.5)
    assert r2.tolist() == w2[0] and k2.tolist() == w2[1]
    r3, k3 = frames.clip_boxes(boxes, None, (H, W))
    w3 = _reference_rule(boxes, np.ones(len(boxes)), (H, W))
    assert r3.tolist() == w3[0] and k3.tolist() == w3[1]
    r4, k4 = frames.clip_boxes(None, None, (H, W))           # `if boxes is not None and probs is not None` (`app.py:185`)
    assert r4.shape == (0, 4) and k4.shape == (0,)


def test_crop_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_crop_resize_u8", 11), ("frmap_resize_coeffs_host", 5)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % sym, header)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
    lib = _lib.load()
    assert hasattr(lib, "frmap_crop_resize_u8") and hasattr(lib, "frmap_resize_coeffs_host")
    assert resize.FRAME_DTYPE.itemsize == 24
