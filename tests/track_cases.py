"""Shared inputs of the tracker tests (test_track_cpu.py, test_track_gpu.py): a seeded moving scene for any number of streams and
box counts, the hand-built sequences - one per branch of the rule, with the ids the rule gives written out - and the helpers
that pad a step and run `frames.track_boxes` over it.  Everything is float32, as a detector returns it."""
import numpy as np

from frmap_amd import frames

F32 = np.float32
P9 = F32(0.9)                                   # the detection threshold as a float32 probability
GRID = [(1, 1), (3, 8), (2, 64), (2, 65), (1, 256)]           # (streams, max_boxes)
COUNTS = (0, 1, 63, 64, 65)                     # and max_boxes itself: the sizes at which the kernel's loops change trip counts


def scene_counts(S, M, steps, seed):
    """[steps][S] box counts: M, 0 (between busy steps) and then every value of COUNTS that fits, in a stream's first steps (six
    steps show them all); random after that."""
    rng = np.random.default_rng(seed)
    pool = [M, 0] + sorted({c for c in COUNTS if 0 < c < M}, reverse=True)
    out = rng.integers(0, M + 1, (steps, S))
    for k in range(min(steps, len(pool))):
        for s in range(S):
            out[k, s] = pool[(k + 2 * s) % len(pool)]
    return out


def moving_scene(S, M, steps, seed, hw=(240, 320), counts=None):
    """A seeded scene per stream: boxes drift, appear, vanish, drop below the detection threshold for a frame and leave the frame's
    edge; the detector's order is shuffled every frame.  Returns [steps][S] of (boxes float32 [n, 4], probs float32 [n])."""
    rng = np.random.default_rng(seed)
    H, W = hw
    counts = scene_counts(S, M, steps, seed + 1) if counts is None else counts
    objs = [np.zeros((0, 6)) for _ in range(S)]               # x, y, w, h, vx, vy
    out = []
    for k in range(steps):
        frame = []
        for s in range(S):
            o = objs[s]
            o[:, 0:2] += o[:, 4:6]                            # drift (some leave the frame: the crop shrinks, then is empty)
            o[:, 2:4] *= rng.uniform(0.97, 1.03, (len(o), 2))
            o = o[rng.random(len(o)) > 0.1]                   # vanish
            n = int(counts[k][s])
            if len(o) > n:
                o = o[:n]
            new = n - len(o)
            fresh = np.concatenate([rng.uniform(-30, [W, H], (new, 2)), rng.uniform(0.4, 70, (new, 2)), rng.uniform(-9, 9, (new, 2))], 1)
            o = objs[s] = np.concatenate([o, fresh])
            order = rng.permutation(n)
            boxes = np.concatenate([o[order, 0:2], o[order, 0:2] + o[order, 2:4]], 1).astype(F32)
            probs = np.where(rng.random(n) < 0.12, rng.uniform(0.3, 0.9, n), rng.uniform(0.9, 1.0, n)).astype(F32)
            probs[rng.random(n) < 0.05] = P9                  # exactly on the threshold: kept
            frame.append((boxes, probs))
        out.append(frame)
    return out


def pad_step(frame, M, use_probs=True):
    """One step of a scene as the padded arrays of `ops.track_step`: boxes [S, M, 4], probs [S, M] or None, counts [S]; the
    padding is filled with values that would be tracked if a kernel read them."""
    S = len(frame)
    boxes = np.tile(np.array([3, 3, 40, 40], F32), (S, M, 1))
    probs = np.ones((S, M), F32)
    counts = np.zeros(S, np.int32)
    for s, (b, p) in enumerate(frame):
        n = 0 if b is None else len(b)
        counts[s] = n
        if n:
            boxes[s, :n] = np.asarray(b, F32).reshape(n, 4)
            probs[s, :n] = 1.0 if p is None else np.asarray(p, F32)
    return boxes, (probs if use_probs else None), counts


def want_rois(boxes, probs, ids, shape):
    """[n, 4] int32: `frames.clip_boxes`' crop of every box that has an id, 0 for the others (clip_boxes raises on non-finite
    coordinates, which the tracker skips, so it is asked about the tracked boxes only)."""
    out = np.zeros((len(ids), 4), np.int32)
    for i in np.flatnonzero(np.asarray(ids) >= 0):
        r, kept = frames.clip_boxes(np.asarray(boxes)[i:i + 1], None if probs is None else np.asarray(probs)[i:i + 1], shape)
        assert kept.tolist() == [0], (i, boxes[i])
        out[i] = r[0]
    return out


def _b(*rows):
    return np.array(rows, F32).reshape(-1, 4)


def _p(*vals):
    return np.array(vals, F32)


A, B = (10, 10, 50, 50), (100, 100, 160, 160)
UP8 = np.nextafter(F32(8), F32(np.inf))
INF, NAN = np.inf, np.nan
_far = [(100 * j, 0, 100 * j + 10, 10) for j in range(70)]
_tie_a = list(_far)
_tie_a[5], _tie_a[69] = (500, 0, 510, 10), (510, 0, 520, 10)            # mirrored about x = 510: equal IoU with (505, 0, 515, 10)
_tie_b = list(_far)
_tie_b[10], _tie_b[67] = (1010, 0, 1020, 10), (1000, 0, 1010, 10)       # the lower index sits in the HIGHER lane (10 vs 67 % 64 = 3)

# name, frame (H, W), steps [(boxes, probs or None)], the ids the rule gives per step, next_id after the last step
HAND = [
    ("1 an empty frame between two frames: ids survive", (200, 200),
     [(_b(A, B), _p(.99, .99)), (None, None), (_b((101, 102, 161, 162), (12, 11, 52, 51)), _p(.95, .95)), (np.zeros((0, 4), F32), np.zeros(0, F32)),
      (_b(A, B), None)],
     [[0, 1], [], [1, 0], [], [0, 1]], 2),
    ("2 every box below the threshold: the state is cleared, next_id is not", (200, 200),
     [(_b(A, B), _p(.99, .99)), (_b(A, B), _p(.5, .89)), (_b(A, B), _p(.99, .99))],
     [[0, 1], [-1, -1], [2, 3]], 4),
    ("3 two boxes compete for one previous box: the earlier takes it, the later its second choice or a new id", (200, 200),
     [(_b((0, 0, 100, 100), (60, 0, 160, 100)), None),
      (_b((10, 0, 110, 100), (5, 0, 105, 100), (20, 0, 120, 100)), None)],       # IoUs with (P0, P1): (.82, .33) (.90, .29) (.67, .43)
     [[0, 1], [0, 2, 1]], 3),
    ("4a two previous boxes with equal IoU: the lower index wins", (200, 200),
     [(_b((10, 0, 20, 10), (0, 0, 10, 10)), None), (_b((5, 0, 15, 10)), None), (_b((10, 0, 20, 10), (0, 0, 10, 10)), None)],
     [[0, 1], [0], [0, 2]], 3),
    ("4b equal IoU in two 64-box slots: index 5 beats index 69", (20, 8000),
     [(_b(*_tie_a), None), (_b((505, 0, 515, 10)), None)], [list(range(70)), [5]], 70),
    ("4c equal IoU, the lower index in the higher lane: index 10 beats index 67", (20, 8000),
     [(_b(*_tie_b), None), (_b((1005, 0, 1015, 10)), None)], [list(range(70)), [10]], 70),
    ("5a IoU exactly at the threshold (3 / 10 == 0.3 in float64): no match", (4, 20),
     [(_b((5, 0, 10, 1)), None), (_b((0, 0, 8, 1)), None)], [[0], [1]], 2),
    ("5b one float32 ulp more: a match", (4, 20),
     [(_b((5, 0, 10, 1)), None), (_b((0, 0, UP8, 1)), None)], [[0], [0]], 1),
    ("6 a confident zero-area box and one outside the frame are skipped and the state stays aligned", (100, 100),
     [(_b(A, (30.2, 30, 30.9, 60), (500, 500, 600, 600), (60, 60, 90, 90)), _p(.99, .99, .99, .99)),
      (_b((61, 60, 91, 90), (11, 10, 51, 50)), _p(.99, .99))],
     [[0, -1, -1, 1], [1, 0]], 2),
    ("7 a probability of exactly float32(0.9) is kept, the float32 below it is skipped", (200, 200),
     [(_b(A, B, (60, 10, 90, 40)), _p(P9, np.nextafter(P9, F32(0)), np.nextafter(P9, F32(1))))], [[0, -1, 1]], 2),
    ("8 NaN and infinite coordinates, NaN and infinite probabilities: skipped", (200, 200),
     [(_b((NAN, 10, 50, 50), (10, 10, INF, 50), (10, -INF, 50, 50), A, B, B), _p(.99, .99, .99, .99, NAN, INF)),
      (_b(A, (10, 10, 50, NAN)), None)],
     [[-1, -1, -1, 0, -1, -1], [0, -1]], 1),
    ("9 a coordinate of -3.7 truncates to -3 and clamps to 0; 50.4 .. 50.6 truncates to an empty crop", (100, 100),
     [(_b((-3.7, -0.5, 20.5, 20.9), (-3.7, 30, -0.2, 60), (50.4, 10, 50.6, 30)), None)], [[0, -1, -1]], 1),
    ("10 coordinates beyond 2^31", (100, 120),
     [(_b((-3e9, -5e9, 4e9, 1e10), (3e9, 0, 4e9, 10), (-4e9, 0, -3e9, 10), (0, 2.2e9, 10, 2.3e9)), None),
      (_b((-3e9, -5e9, 4e9, 1e10)), None)],
     [[0, -1, -1, -1], [0]], 1),
]
HAND_ROIS = {                                    # crops worth writing out: (case prefix, step, box) -> (x1, y1, x2, y2)
    ("9", 0, 0): (0, 0, 20, 20),
    ("10", 0, 0): (0, 0, 120, 100),
    ("6", 0, 3): (60, 60, 90, 90),
    ("5b", 1, 0): (0, 0, 8, 1),
}


def hand_max_boxes(case):
    return max(1, max(0 if b is None else len(b) for b, _ in case[2]))


def run_python(frames_of_stream, shape, state=None, **kw):
    """`frames.track_boxes` over one stream's steps: ([ids per step], [state after each step])."""
    ids, states = [], []
    for boxes, probs in frames_of_stream:
        i, state = frames.track_boxes(state, boxes, probs, shape, **kw)
        ids.append(i)
        states.append(state)
    return ids, states


BROKEN = ("last_max", "ge_thresh", "no_matched_flag", "iou_in_float32", "clear_on_empty_frame", "reset_next_id", "round_coords",
          "prob_in_float64", "ties_by_lane", "keep_untracked_in_state")


def broken_track_boxes(variant, state, boxes, probs, shape, det_thresh=0.9, iou_thresh=0.3):
    """`frames.track_boxes` with ONE deliberate mistake - the mistakes a kernel of this rule is likely to make.  Every variant must
    get some hand-built sequence wrong (test_track_cpu.py): that is what shows the sequences bite."""
    state = frames.new_track_state() if state is None else state
    n = 0 if boxes is None else len(boxes)
    if n == 0:
        return np.zeros(0, np.int64), (frames.new_track_state()._replace(next_id=state.next_id) if variant == "clear_on_empty_frame" else state)
    b32 = np.asarray(boxes, F32).reshape(n, 4)
    p32 = None if probs is None else np.asarray(probs, F32)
    H, W = shape[0], shape[1]
    prev, matched, next_id = state.boxes, [False] * len(state.ids), state.next_id
    ids = np.full(n, -1, np.int64)
    in_state = np.zeros(n, bool)
    for i in range(n):
        if p32 is not None:
            low = float(p32[i]) < det_thresh if variant == "prob_in_float64" else p32[i] < F32(det_thresh)
            if low or not np.isfinite(p32[i]):
                continue
        if not np.isfinite(b32[i]).all():
            continue
        in_state[i] = True                                    # "confident": what the reference's prev_boxes keeps
        x1, y1, x2, y2 = [int(round(float(v))) if variant == "round_coords" else int(v) for v in b32[i]]
        if min(W, x2) <= max(0, x1) or min(H, y2) <= max(0, y1):
            continue
        best, best_j = 0.0, -1
        order = sorted(range(len(prev)), key=lambda j: (j % 64, j)) if variant == "ties_by_lane" else range(len(prev))
        for j in order:
            if matched[j] and variant != "no_matched_flag":
                continue
            if variant == "iou_in_float32":
                a, b = b32[i], prev[j]
                xl, yt, xr, yb = max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])
                inter = (xr - xl) * (yb - yt) if not (xr < xl or yb < yt) else F32(0)
                union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
                iou = float(inter / union) if union > 0 else 0.0
            else:
                iou = frames.box_iou(b32[i], prev[j])
            better = iou >= best and iou > 0 if variant == "last_max" else iou > best
            if better and (iou >= iou_thresh if variant == "ge_thresh" else iou > iou_thresh):
                best, best_j = iou, j
        if best_j >= 0:
            ids[i] = state.ids[best_j]
            matched[best_j] = True
        else:
            ids[i] = next_id
            next_id += 1
    if variant == "reset_next_id" and not (ids >= 0).any():
        next_id = 0
    if variant == "keep_untracked_in_state":                  # the reference's two lists, out of step: boxes of all confident
        got = ids >= 0                                        # detections, ids of the tracked ones, padded with fresh ids
        extra = np.arange(next_id, next_id + int(in_state.sum() - got.sum()))
        return ids, frames.TrackState(b32[in_state].copy(), np.concatenate([ids[got], extra]), next_id)
    got = ids >= 0
    return ids, frames.TrackState(b32[got].copy(), ids[got].copy(), next_id)
