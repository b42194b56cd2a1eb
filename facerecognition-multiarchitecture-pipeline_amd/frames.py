"""The host side of the reference's per-frame loop (`src/app.py:181-241`): from a detector's boxes to the integer crops
`matching.embed_boxes` / `matching.identify_boxes` cut out of the frame on the device - and, for aligned crops, the geometry of
the reference's dataset step (`src/data_prep.py:69-106`): the eye-line rotation, its matrix, the margin rule - and the loop's IoU
tracker (`app.py:126-147, 183-247`: `box_iou`, `track_boxes`), the readable statement of the rule `ops.track_step` runs for many
streams in one launch - and the templates of its tracks (`fuse_tracks`: a track's embeddings pooled into a decayed sum and a
weight, the rule `ops.track_fuse` runs) - and the conversion rule of 4:2:0 YUV frames (`YUV_COEFFS`, `yuv_to_rgb`: what the YUV
crop kernels compute per pixel).  Pure host code; the detector itself (MTCNN) is outside this package.

The tracker departs from the reference in two places.  (a) The IoU is float64 arithmetic on the detector's float32 coordinates,
nothing fused: the reference mixes `np.float32` rows with Python floats from `tolist()`, so which of its operations run in float32
depends on which operand a `max` returned and on the NumPy major version; the two can differ only where an IoU lies within
float32 rounding of the threshold or of a competing IoU.  (b) The state keeps only boxes that received an id: the reference
rebuilds `prev_boxes` from every confident box but `face_ids` only from boxes with an id, so a confident box that is empty after
clipping puts its two lists out of step (wrong ids later, or an `IndexError` its loop swallows with the frame)."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

DET_THRESH = 0.9                       # `app.py:18`
TRACKING_THRESHOLD = 0.3               # `app.py:29`


def _yuv_row(kr: float, kb: float, full_range: bool) -> Tuple[int, int, int, int, int, int]:
    """One row of `YUV_COEFFS` from ``(Kr, Kb)``: float64 coefficients of R = Y' + rv V', G = Y' + gu U' + gv V', B = Y' + bu U',
    luma scaled by 255/219 (offset 16) and chroma by 255/224 for limited range, each as ``floor(c * 65536 + 0.5)``."""
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    q = lambda c: int(math.floor(c * 65536.0 + 0.5))
    return (0 if full_range else 16, q(sy), q(2.0 * (1.0 - kr) * sc), q(-2.0 * kb * (1.0 - kb) / kg * sc),
            q(-2.0 * kr * (1.0 - kr) / kg * sc), q(2.0 * (1.0 - kb) * sc))


YUV_KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
# csc code -> (y_off, cy, rv, gu, gv, bu): the table of csrc/yuv_pixel.h.  csc = 2 * (standard is bt709) + full_range.
YUV_COEFFS = {2 * si + int(fr): _yuv_row(*YUV_KR_KB[std], fr) for si, std in enumerate(("bt601", "bt709")) for fr in (False, True)}
assert YUV_COEFFS == {0: (16, 76309, 104597, -25675, -53279, 132201), 1: (0, 65536, 91881, -22553, -46802, 116130),
                      2: (16, 76309, 117489, -13975, -34925, 138438), 3: (0, 65536, 103206, -12276, -30679, 121609)}


def yuv_csc(standard: str = "bt601", full_range: bool = False) -> int:
    """The ``csc`` code of a (standard, range) pair: the row of `YUV_COEFFS`."""
    if standard not in YUV_KR_KB:
        raise ValueError(f"yuv: standard must be 'bt601' or 'bt709', got {standard!r}")
    return 2 * int(standard == "bt709") + int(bool(full_range))


def yuv_to_rgb(y, u, v, standard: str = "bt601", full_range: bool = False) -> np.ndarray:
    """A 4:2:0 frame of 8-bit samples as uint8 RGB ``[H, W, 3]``: the readable statement of the rule the YUV crop kernels apply per
    pixel (`resize.crop_resize_u8` on a `resize.YuvFrame` equals the same call on this array, bit for bit).

    ``y``: uint8 ``[H, W]``; ``u``, ``v``: uint8 ``[ceil(H/2), ceil(W/2)]``, arrays of any strides (the two halves of an NV12
    plane, say).  Pixel ``(x, y)`` takes chroma sample ``(x >> 1, y >> 1)`` - nearest replication, no interpolation.  Colour is
    16-bit fixed point in int32 with the row ``(y_off, cy, rv, gu, gv, bu)`` of `YUV_COEFFS` and an arithmetic shift:

        ``R = clip8((cy (Y - y_off) + rv (V - 128) + 32768) >> 16)``
        ``G = clip8((cy (Y - y_off) + gu (U - 128) + gv (V - 128) + 32768) >> 16)``
        ``B = clip8((cy (Y - y_off) + bu (U - 128) + 32768) >> 16)``

    which is at most 1 away from ``clip(floor(float64 formula + 0.5))`` for every ``(Y, U, V)``."""
    y, u, v = np.asarray(y), np.asarray(u), np.asarray(v)
    if y.dtype != np.uint8 or u.dtype != np.uint8 or v.dtype != np.uint8 or y.ndim != 2 or u.ndim != 2 or v.ndim != 2:
        raise ValueError("yuv_to_rgb: y, u and v must be uint8 planes")
    H, W = y.shape
    if H < 1 or W < 1 or u.shape != ((H + 1) // 2, (W + 1) // 2) or v.shape != u.shape:
        raise ValueError(f"yuv_to_rgb: a {H}x{W} luma plane needs chroma planes of {(H + 1) // 2}x{(W + 1) // 2}, got {u.shape} and {v.shape}")
    y_off, cy, rv, gu, gv, bu = YUV_COEFFS[yuv_csc(standard, full_range)]
    yi, xi = np.arange(H)[:, None] >> 1, np.arange(W)[None, :] >> 1
    l = cy * (y.astype(np.int32) - y_off) + 32768
    uu, vv = u[yi, xi].astype(np.int32) - 128, v[yi, xi].astype(np.int32) - 128
    rgb = np.stack([l + rv * vv, l + gu * uu + gv * vv, l + bu * uu], axis=-1) >> 16          # (numpy's >> on int32 is arithmetic)
    return np.clip(rgb, 0, 255).astype(np.uint8)


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


def box_iou(a, b) -> float:
    """`calc_iou` (`app.py:126-147`) of two raw boxes ``(x1, y1, x2, y2)`` in Python floats (float64): intersection corners by
    max / min, 0 when they cross, else ``inter / (a1 + a2 - inter)`` if that union is positive, else 0."""
    x1_1, y1_1, x2_1, y2_1 = [float(v) for v in a]
    x1_2, y1_2, x2_2, y2_2 = [float(v) for v in b]
    x_left, y_top = max(x1_1, x1_2), max(y1_1, y1_2)
    x_right, y_bottom = min(x2_1, x2_2), min(y2_1, y2_2)
    if x_right < x_left or y_bottom < y_top:
        return 0.0
    inter = (x_right - x_left) * (y_bottom - y_top)
    union = (x2_1 - x1_1) * (y2_1 - y1_1) + (x2_2 - x1_2) * (y2_2 - y1_2) - inter
    return inter / union if union > 0 else 0.0


class TrackState(NamedTuple):
    """One stream's tracker state: the previous step's tracked boxes (raw, float32 ``[P, 4]``), their ids (int64 ``[P]``) and the
    next id to hand out (the reference's ``prev_boxes``, ``face_ids``, ``face_id_counter``)."""
    boxes: np.ndarray
    ids: np.ndarray
    next_id: int


def new_track_state() -> TrackState:
    return TrackState(np.zeros((0, 4), np.float32), np.zeros(0, np.int64), 0)


def _tracked_roi(box, prob, H: int, W: int, det_thresh):
    """`clip_boxes`' verdict on one float32 box: its integer crop, or ``None`` when the box is skipped - below the threshold (in
    float32), a non-finite coordinate or probability (`clip_boxes` raises on those), or an empty crop."""
    if prob is not None and (not math.isfinite(prob) or np.float32(prob) < np.float32(det_thresh)):
        return None
    if not all(math.isfinite(v) for v in box):
        return None
    x1, y1, x2, y2 = [int(v) for v in box]
    x1, y1 = max(0, x1), max(0, y1)
    x2, y2 = min(W, x2), min(H, y2)
    if x2 <= x1 or y2 <= y1:
        return None
    return x1, y1, x2, y2


def track_boxes(state: Optional[TrackState], boxes, probs, frame_shape: Sequence[int], det_thresh: float = DET_THRESH,
                iou_thresh: float = TRACKING_THRESHOLD) -> Tuple[np.ndarray, TrackState]:
    """One step of the reference's tracker (`app.py:183-247`) for one stream: ``(ids int64 [n], new_state)``, ``ids[i]`` the
    ``face_id`` of box i or -1 for a box the loop skips.  ``state``: what the previous call returned (``None``: a fresh one);
    ``boxes`` / ``probs``: the detector's output, taken as float32 (``probs = None``: every box is confident; ``boxes = None`` or
    empty: nothing is returned and the state is left as it is - tracks survive empty frames, `:244`).

    The boxes are walked in the detector's order.  Box i is skipped when ``probs[i] < det_thresh`` (compared in float32, as
    `clip_boxes` does on a detector's float32 probabilities: one equal to ``float32(det_thresh)`` is kept), when a coordinate or the
    probability is not finite, or when its `clip_boxes` crop is empty.  Otherwise the previous boxes not yet matched in this step
    are scanned in ascending order and j replaces the best so far when ``box_iou(box_i, prev_j) > best`` (which starts at 0) and
    ``> iou_thresh``: the first maximum wins, ties go to the lowest j.  A winner hands over its id and becomes matched; without one
    the box takes ``next_id``.  The new state holds the raw boxes and ids of the boxes that received an id, in order (departure
    (b) of the module docstring); ``next_id`` is never reset."""
    if state is None:
        state = new_track_state()
    n = 0 if boxes is None else len(boxes)
    if n == 0:
        return np.zeros(0, np.int64), state
    b32 = np.asarray(boxes, dtype=np.float32).reshape(n, 4)
    p32 = None if probs is None else np.asarray(probs, dtype=np.float32).reshape(n)
    H, W = int(frame_shape[0]), int(frame_shape[1])
    prev = [[float(v) for v in pb] for pb in state.boxes]
    matched = [False] * len(prev)
    next_id = int(state.next_id)
    ids = np.full(n, -1, np.int64)
    for i in range(n):
        if _tracked_roi(b32[i].tolist(), None if p32 is None else float(p32[i]), H, W, det_thresh) is None:
            continue
        best, best_j = 0.0, -1
        for j, pb in enumerate(prev):
            if matched[j]:
                continue
            iou = box_iou(b32[i], pb)
            if iou > best and iou > iou_thresh:
                best, best_j = iou, j
        if best_j >= 0:
            ids[i] = state.ids[best_j]
            matched[best_j] = True
        else:
            ids[i] = next_id
            next_id += 1
    got = ids >= 0
    return ids, TrackState(b32[got].copy(), ids[got].copy(), next_id)


class TemplateState(NamedTuple):
    """One stream's track templates: per slot the track id (int64 ``[P]``), the weight (float32 ``[P]``) and the decayed sum of
    the track's embeddings (float32 ``[P, D]``).  After a step the slots are the detections that received an id, in detection
    order: `TrackState.ids` of the tracker after the same step."""
    ids: np.ndarray
    weights: np.ndarray
    sums: np.ndarray


def new_template_state(dim: int = 0) -> TemplateState:
    return TemplateState(np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros((0, dim), np.float32))


def fuse_tracks(state: Optional[TemplateState], ids, emb, det, decay: float = 1.0):
    """One step of the track templates for one stream, the readable statement of the rule `ops.track_fuse` runs for many streams
    in one launch: ``(fused float32 [r, D], frames float32 [r], new_state)``.  ``state``: what the previous call returned
    (``None``: a fresh one); ``ids``: the tracker's ids of this step's ``n`` detections (`track_boxes`; -1: skipped); ``emb``:
    float32 ``[r, D]``, the embeddings computed at this step; ``det``: int ``[r]``, the detection each row belongs to - not every
    detection needs a row; ``decay``: ``0 < decay <= 1``, taken as float32.

    ``n == 0`` leaves the state as it is (tracks survive empty frames, as in the tracker).  Otherwise the new state has one slot
    per detection with ``id >= 0``, in detection order; ids of the old state that are absent are dropped.  A detection whose id
    is in the old state and whose row holds only finite values pools it: ``w' = fl(fl(decay w) + 1)``, ``sum' = fl(fl(decay sum)
    + e)`` - float32, product then sum, two roundings; an id that is new starts at ``w' = 1``, ``sum' = e``.  Without a row, or
    with a row that holds an infinity or a NaN, the old slot is carried over unchanged (a new id: ``w' = 0``, ``sum' = 0``): one
    bad frame does not poison a track.  Row ``i`` comes back as the template ``sum' / w'`` (float32 division) of its track with
    ``frames[i] = w'`` - with ``decay = 1`` the number of embeddings pooled -; a row whose detection has ``id < 0``, that is not
    finite, or whose slot has ``w' == 0`` comes back as it came, with ``frames[i] = 0``.

    ``ValueError``, before anything is computed, for a ``det`` outside ``[0, n)`` and for two rows of the same detection."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    n = len(ids)
    emb = np.asarray(emb, dtype=np.float32)
    det = np.asarray(det, dtype=np.int64).reshape(-1)
    if emb.ndim != 2 or emb.shape[0] != len(det):
        raise ValueError(f"fuse_tracks: emb must be float32 [r, D] with one detection index per row, got {emb.shape} and {len(det)}")
    d32 = np.float32(decay)
    if not (np.float32(0) < d32 <= np.float32(1)):
        raise ValueError(f"fuse_tracks: decay = {decay} is outside (0, 1]")
    if len(det) and (det.min() < 0 or det.max() >= n):
        raise ValueError(f"fuse_tracks: a row names a detection outside [0, {n})")
    if len(np.unique(det)) != len(det):
        raise ValueError("fuse_tracks: two rows name the same detection")
    D = emb.shape[1]
    if state is None:
        state = new_template_state(D)
    fused, frames = emb.copy(), np.zeros(len(det), np.float32)
    if n == 0:
        return fused, frames, state
    if len(state.ids) and state.sums.shape[1] != D:
        raise ValueError(f"fuse_tracks: the state holds sums of {state.sums.shape[1]} values, the rows have {D}")
    row_of = {int(i): r for r, i in enumerate(det)}
    old = {}
    for j, tid in enumerate(state.ids.tolist()):
        old.setdefault(tid, j)                                # (ids of a state are distinct; the lowest slot if they were not)
    new_ids, new_w, new_sums = [], [], []
    one = np.float32(1)
    for i in range(n):
        tid = int(ids[i])
        if tid < 0:
            continue
        j = old.get(tid)
        r = row_of.get(i)
        if r is not None and np.isfinite(emb[r]).all():
            if j is None:
                w2, s2 = one, emb[r].copy()
            else:
                with np.errstate(all="ignore"):               # (a sum may overflow; the rule says what comes out, not that it is useful)
                    w2 = np.float32(np.float32(d32 * state.weights[j]) + one)
                    s2 = (d32 * state.sums[j]).astype(np.float32) + emb[r]
            if w2 != 0:
                with np.errstate(all="ignore"):
                    fused[r] = s2 / w2
                frames[r] = w2
        elif j is not None:
            w2, s2 = state.weights[j], state.sums[j].copy()
        else:
            w2, s2 = np.float32(0), np.zeros(D, np.float32)
        new_ids.append(tid)
        new_w.append(w2)
        new_sums.append(s2)
    return fused, frames, TemplateState(np.asarray(new_ids, np.int64), np.asarray(new_w, np.float32),
                                        np.asarray(new_sums, np.float32).reshape(len(new_ids), D))
