"""The host side of the reference's per-frame loop (`src/app.py:181-241`): from a detector's boxes to the integer crops
`matching.embed_boxes` / `matching.identify_boxes` cut out of the frame on the device - and, for aligned crops, the geometry of
the reference's dataset step (`src/data_prep.py:69-106`): the eye-line rotation, its matrix, the margin rule.  Pure host code;
the detector itself (MTCNN) and the IoU tracker (`app.py:126-147, 202-221`) are outside this package."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np

DET_THRESH = 0.9                       # `app.py:18`


def clip_boxes(boxes, probs, frame_shape: Sequence[int], det_thresh: float = DET_THRESH) -> Tuple[np.ndarray, np.ndarray]:
    """The reference's box rule (`app.py:190-200, 224-235`): skip a box whose ``prob < det_thresh``; ``int()`` every coordinate
    (truncation toward zero); clamp to the frame with ``max(0, .)`` / ``min(W or H, .)``; drop the box if ``x2 <= x1`` or ``y2 <= y1``.

    ``boxes``: ``[n, 4]`` = ``(x1, y1, x2, y2)`` as the detector returns them (or ``None``: no faces), ``probs``: ``[n]`` (``None``:
    every box is kept), ``frame_shape``: the frame's ``(H, W[, C])``.  Returns ``(rois int32 [m, 4], kept int64 [m])``: the integer
    crops ``frame[y1:y2, x1:x2]`` and the index of the box each came from, in the detector's order."""
    H, W = int(frame_shape[0]), int(frame_shape[1])
    rois, kept = [], []
    if boxes is not None:
        for i, box in enumerate(boxes):
            if probs is not None and probs[i] < det_thresh:
                continue
            x1, y1, x2, y2 = [int(b) for b in box]
            x1, y1 = max(0, x1), max(0, y1)
            x2, y2 = min(W, x2), min(H, y2)
            if x2 <= x1 or y2 <= y1:
                continue
            rois.append((x1, y1, x2, y2))
            kept.append(i)
    return np.asarray(rois, dtype=np.int32).reshape(-1, 4), np.asarray(kept, dtype=np.int64)


def eye_rotation(landmarks) -> Tuple[float, Tuple[float, float]]:
    """`align_face`'s rotation (`data_prep.py:71-81`): ``(angle_deg, (cx, cy))`` with ``angle_deg = degrees(arctan2(dY, dX))`` from
    ``landmarks[0]`` (left eye) to ``landmarks[1]`` (right eye) - positive when the right eye is lower in the image, which a
    counter-clockwise rotation by that angle levels - and the centre ``((lx + rx) // 2, (ly + ry) // 2)``: floor division of floats,
    as the reference writes it.  ``landmarks``: ``[>= 2, 2]`` in the detector's order; coincident eyes give angle 0."""
    lm = np.asarray(landmarks, dtype=np.float64)
    if lm.ndim != 2 or lm.shape[0] < 2 or lm.shape[1] != 2:
        raise ValueError("eye_rotation: landmarks must be [>= 2, 2] = (x, y) per point, eyes first")
    left_eye, right_eye = lm[0], lm[1]
    dY = right_eye[1] - left_eye[1]
    dX = right_eye[0] - left_eye[0]
    angle = float(np.degrees(np.arctan2(dY, dX)))
    return angle, (float((left_eye[0] + right_eye[0]) // 2), float((left_eye[1] + right_eye[1]) // 2))


def rotation_matrix(angle_deg: float, center) -> np.ndarray:
    """The output -> input affine matrix ``float64 [6] = (a, b, c, d, e, f)`` of ``PIL.Image.rotate(angle_deg, center=center)``
    (Image.py), Pillow's rule to the bit: ``angle % 360.0``, cos / sin of the negated angle rounded to 15 decimals, the translation
    that leaves ``center`` where it is.  Output pixel (x, y) samples the frame at ``(a (x + .5) + b (y + .5) + c, d (x + .5) +
    e (y + .5) + f)``.  DEPARTURE from the reference: `cv2.getRotationMatrix2D` + `cv2.warpAffine` rotate by the same angle about the
    same point but resample differently; `resize.align_crop_resize_u8` is pinned to Pillow."""
    angle = -math.radians(float(angle_deg) % 360.0)
    cx, cy = float(center[0]), float(center[1])
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return np.array(m, dtype=np.float64)


def margin_boxes(boxes, margin: float, frame_shape: Sequence[int]) -> Optional[np.ndarray]:
    """`get_face_bbox_with_margin` (`data_prep.py:89-106`) per box: widen by ``int(width * margin)`` / ``int(height * margin)`` on
    each side, clamp to ``[0, W]`` / ``[0, H]``.  Floats in, floats out (``float64 [n, 4]``; ``None`` stays ``None``): the ``int()``
    of the crop (`:144-145`) is `clip_boxes`' job, and with ``margin = 0`` `clip_boxes` of the result is `clip_boxes` of ``boxes``."""
    if boxes is None:
        return None
    H, W = int(frame_shape[0]), int(frame_shape[1])
    out = []
    for box in boxes:
        x1, y1, x2, y2 = [float(b) for b in box]
        margin_x = int((x2 - x1) * margin)
        margin_y = int((y2 - y1) * margin)
        out.append((max(0, x1 - margin_x), max(0, y1 - margin_y), min(W, x2 + margin_x), min(H, y2 + margin_y)))
    return np.asarray(out, dtype=np.float64).reshape(-1, 4)
