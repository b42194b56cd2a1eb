"""Shared inputs of the track-template tests (test_track_fuse_cpu.py, test_track_fuse_gpu.py): the hand-built sequences - one per
branch of the rule, with the state and the templates the rule gives written out -, seeded random sequences for any number of
streams, boxes and embedding lengths, and the helpers that run `frames.fuse_tracks` over a padded step and compare bit for bit.
The ids and counts are built here, as a tracker would emit them: no test of the fuse step needs the tracker itself."""
import itertools

import numpy as np

from frmap_amd import frames

F32 = np.float32
NAN, INF = np.nan, np.inf
S_GRID, M_GRID, D_GRID = (1, 5), (1, 64, 65, 256), (1, 3, 36, 64, 65, 512, 513)
GRID = list(itertools.product(S_GRID, M_GRID))
COUNTS = (0, 1, 3, 4, 5, 63, 64, 65)            # and max_boxes itself: fewer / as many / more faces than the workgroup's 4 waves; 64-id chunks


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
# hand-built sequences of ONE stream, D = 2: name, decay, steps [(ids, [(detection, embedding)])], and per step the result written
# out: (state ids, state weights, state sums, fused rows, frames) - rows in the order they are given
# ---------------------------------------------------------------------------------------------------------------------------------
HAND = [
    ("1 a new track", 1.0,
     [([0], [(0, (1, 2))])],
     [([0], [1], [(1, 2)], [(1, 2)], [1])]),
    ("2 a continued track: the mean of 2 and of 3 frames", 1.0,
     [([0], [(0, (1, 2))]), ([0], [(0, (3, 6))]), ([0], [(0, (2, 1))])],
     [([0], [1], [(1, 2)], [(1, 2)], [1]), ([0], [2], [(4, 8)], [(2, 4)], [2]), ([0], [3], [(6, 9)], [(2, 3)], [3])]),
    ("3 two tracks whose detection order reverses: the slots swap", 1.0,
     [([0, 1], [(0, (1, 2)), (1, (10, 20))]), ([1, 0], [(0, (30, 40)), (1, (3, 4))]), ([0, 1], [(1, (2, 0)), (0, (5, 6))])],
     [([0, 1], [1, 1], [(1, 2), (10, 20)], [(1, 2), (10, 20)], [1, 1]),
      ([1, 0], [2, 2], [(40, 60), (4, 6)], [(20, 30), (2, 3)], [2, 2]),
      ([0, 1], [3, 3], [(9, 12), (42, 60)], [(14, 20), (3, 4)], [3, 3])]),
    ("4 a track vanishes while a new one appears at a lower slot", 1.0,
     [([0, 1], [(0, (1, 2)), (1, (10, 20))]), ([2, 1], [(0, (5, 5)), (1, (30, 40))]), ([1], [(0, (2, 2))])],
     [([0, 1], [1, 1], [(1, 2), (10, 20)], [(1, 2), (10, 20)], [1, 1]),
      ([2, 1], [1, 2], [(5, 5), (40, 60)], [(5, 5), (20, 30)], [1, 2]),
      ([1], [3], [(42, 62)], [(14, 62 / 3)], [3])]),
    ("5 an empty frame: the state is kept", 1.0,
     [([0], [(0, (1, 2))]), ([], []), ([0], [(0, (3, 6))])],
     [([0], [1], [(1, 2)], [(1, 2)], [1]), ([0], [1], [(1, 2)], [], []), ([0], [2], [(4, 8)], [(2, 4)], [2])]),
    ("6 a frame whose boxes are all skipped: the state is cleared", 1.0,
     [([0], [(0, (1, 2))]), ([-1, -1], [(0, (7, 7))]), ([1], [(0, (3, 6))])],
     [([0], [1], [(1, 2)], [(1, 2)], [1]), ([], [], [], [(7, 7)], [0]), ([1], [1], [(3, 6)], [(3, 6)], [1])]),
    ("7 a tracked detection without a row: its slot is carried over", 1.0,
     [([0, 1], [(0, (1, 2)), (1, (10, 20))]), ([0, 1], [(1, (30, 40))]), ([1, 0], [(1, (3, 6))])],
     [([0, 1], [1, 1], [(1, 2), (10, 20)], [(1, 2), (10, 20)], [1, 1]),
      ([0, 1], [1, 2], [(1, 2), (40, 60)], [(20, 30)], [2]),
      ([1, 0], [2, 2], [(40, 60), (4, 8)], [(2, 4)], [2])]),
    ("8 a NaN row and an inf row: carried over, the rows returned as they are", 1.0,
     [([0, 1], [(0, (1, 2)), (1, (10, 20))]), ([0, 1], [(0, (NAN, 5)), (1, (6, -INF))]), ([0, 1], [(0, (3, 6)), (1, (30, 40))])],
     [([0, 1], [1, 1], [(1, 2), (10, 20)], [(1, 2), (10, 20)], [1, 1]),
      ([0, 1], [1, 1], [(1, 2), (10, 20)], [(NAN, 5), (6, -INF)], [0, 0]),
      ([0, 1], [2, 2], [(4, 8), (40, 60)], [(2, 4), (20, 30)], [2, 2])]),
    ("9 a row of a detection with id -1", 1.0,
     [([0, -1], [(0, (1, 2)), (1, (9, 9))]), ([-1, 0], [(0, (8, 8)), (1, (3, 6))])],
     [([0], [1], [(1, 2)], [(1, 2), (9, 9)], [1, 0]), ([0], [2], [(4, 8)], [(8, 8), (2, 4)], [0, 2])]),
    ("10 a new id without a row, a new id with a NaN row; their rows come a step later", 1.0,
     [([0, 1], [(1, (NAN, NAN))]), ([0, 1], [(0, (3, 6)), (1, (5, 7))]), ([0, 1], [(0, (1, 0)), (1, (1, 1))])],
     [([0, 1], [0, 0], [(0, 0), (0, 0)], [(NAN, NAN)], [0]),
      ([0, 1], [1, 1], [(3, 6), (5, 7)], [(3, 6), (5, 7)], [1, 1]),
      ([0, 1], [2, 2], [(4, 6), (6, 8)], [(2, 3), (3, 4)], [2, 2])]),
    ("11 decay 0.5: the weight and the sum halve before the new frame is added", 0.5,
     [([0], [(0, (1, 2))]), ([0], [(0, (3, 6))]), ([0], [(0, (1, 1))])],
     [([0], [1], [(1, 2)], [(1, 2)], [1]), ([0], [1.5], [(3.5, 7)], [(F32(3.5) / F32(1.5), F32(7) / F32(1.5))], [1.5]),
      ([0], [1.75], [(2.75, 4.5)], [(F32(2.75) / F32(1.75), F32(4.5) / F32(1.75))], [1.75])]),
]


def hand_step_arrays(step, M=None):
    """One hand-built step as the padded arrays of a 1-stream call: ids [1, M], counts [1], emb [r, 2], rows [r, 2]."""
    ids, rws = step
    M = max(1, len(ids)) if M is None else M
    pad = np.zeros((1, M), np.int32)                          # padding holds an id that would be pooled if it were read
    pad[0, :len(ids)] = ids
    emb = np.array([e for _, e in rws], F32).reshape(len(rws), 2)
    rows = np.array([(0, d) for d, _ in rws], np.int32).reshape(len(rws), 2)
    return pad, np.array([len(ids)], np.int32), emb, rows


def hand_max_boxes(case):
    return max(1, max(len(ids) for ids, _ in case[2]))


def check_hand_step(label, want, fused, nframes, state):
    """A hand-built step's result against what is written out: floats by value where they are finite (the written values are
    exact in float32), NaN for NaN, and the state slot by slot."""
    w_ids, w_w, w_sums, w_fused, w_frames = want
    assert state.ids.tolist() == list(w_ids), label
    assert same_bits(state.weights, np.array(w_w, F32)), (label, state.weights)
    assert same_bits(state.sums.reshape(-1), np.array(w_sums, F32).reshape(-1)), (label, state.sums)
    assert same_bits(np.asarray(nframes), np.array(w_frames, F32)), (label, nframes)
    got, exp = np.asarray(fused, F32).reshape(-1), np.array(w_fused, F32).reshape(-1)
    assert got.shape == exp.shape and np.array_equal(np.isnan(got), np.isnan(exp)), (label, got)
    assert same_bits(got[~np.isnan(got)], exp[~np.isnan(exp)]), (label, got, exp)


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded random sequences of S streams
# ---------------------------------------------------------------------------------------------------------------------------------
def scene_counts(S, M, steps, seed):
    rng = np.random.default_rng(seed)
    pool = [M, 0] + sorted({c for c in COUNTS if 0 < c < M}, reverse=True)
    out = rng.integers(0, M + 1, (steps, S))
    for k in range(min(steps, len(pool))):
        for s in range(S):
            out[k, s] = pool[(k + 2 * s) % len(pool)]
    return out


def random_steps(S, M, D, steps, seed, counts=None, bad=0.04):
    """[steps] of (ids int32 [S, M], counts int32 [S], emb float32 [N, D], rows int32 [N, 2]).  Per stream the ids move as a
    tracker's do: most live ids survive in a shuffled order, some vanish for good, new ones take the stream's next id, some
    detections are skipped (-1); the padding beyond a stream's count holds ids that would be pooled if a kernel read them.  About
    four detections in five have a row - skipped ones too -, a few rows hold a NaN or an infinity, and the rows of all streams
    are shuffled together."""
    rng = np.random.default_rng(seed)
    counts = scene_counts(S, M, steps, seed + 1) if counts is None else counts
    live, next_id, out = [[] for _ in range(S)], [0] * S, []
    for k in range(steps):
        ids = np.zeros((S, M), np.int32)
        rows = []
        for s in range(S):
            n = int(counts[k][s])
            if n == 0:
                continue
            keep = [t for t in live[s] if rng.random() < 0.8][:n]
            fresh = list(range(next_id[s], next_id[s] + n - len(keep)))
            next_id[s] += len(fresh)
            cur = np.array(keep + fresh, np.int32)[rng.permutation(n)]
            cur[rng.random(n) < 0.15] = -1
            ids[s, :n] = cur
            live[s] = [int(t) for t in cur if t >= 0]
            rows += [(s, i) for i in range(n) if rng.random() < 0.8]
        rows = np.array(rows, np.int32).reshape(-1, 2)[rng.permutation(len(rows))]
        emb = (rng.standard_normal((len(rows), D)) * rng.choice([1e-3, 1.0, 40.0], (len(rows), 1))).astype(F32)
        for r in np.flatnonzero(rng.random(len(rows)) < bad):
            emb[r, rng.integers(0, D)] = rng.choice([NAN, INF, -INF])
        out.append((ids, np.asarray(counts[k], np.int32).copy(), emb, rows))
    return out


def python_step(states, step, decay):
    """`frames.fuse_tracks` stream by stream over one padded step: (fused [N, D], frames [N]); ``states`` is updated in place."""
    ids, counts, emb, rows = step
    fused, nframes = np.empty_like(emb), np.empty(len(emb), F32)
    for s in range(len(states)):
        sel = np.flatnonzero(rows[:, 0] == s) if len(rows) else np.zeros(0, np.int64)
        f, n, states[s] = frames.fuse_tracks(states[s], ids[s, :counts[s]], emb[sel], rows[sel, 1], decay)
        fused[sel], nframes[sel] = f, n
    return fused, nframes


def check_states(label, got, want, D):
    """The logical state - ids, weights and sums per slot - of every stream, bit for bit (``want``: None = a fresh stream)."""
    for s, (g, w) in enumerate(zip(got, want)):
        w = frames.new_template_state(D) if w is None else w
        assert g.ids.tolist() == w.ids.tolist(), (label, s, g.ids, w.ids)
        assert same_bits(g.weights, w.weights), (label, s)
        assert same_bits(g.sums, w.sums.reshape(len(w.ids), D)), (label, s)


def long_track(steps=300, D=8, seed=9):
    """One track (id 0) followed for ``steps`` steps next to a second one (id 1) that swaps places with it now and then and misses
    a frame now and then: [steps] of padded 1-stream steps with M = 2."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(steps):
        order = [0, 1] if rng.random() < 0.7 else [1, 0]
        ids = np.array([order], np.int32)
        have = [i for i in range(2) if order[i] == 0 or rng.random() < 0.8]
        emb = rng.standard_normal((len(have), D)).astype(F32)
        out.append((ids, np.array([2], np.int32), emb, np.array([(0, i) for i in have], np.int32).reshape(-1, 2)))
    return out
