"""The host side of the reference's per-frame loop (`src/app.py:181-241`): from a detector's boxes to the integer crops
`matching.embed_boxes` / `matching.identify_boxes` cut out of the frame on the device.  Pure host code; the detector itself
(MTCNN) and the IoU tracker (`:126-147, 202-221`) are outside this package."""
from __future__ import annotations

from typing import Sequence, Tuple

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
