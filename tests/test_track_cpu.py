"""CPU: the frame loop's IoU tracker - `frames.box_iou` and `frames.track_boxes` (the rule in plain Python) on hand values and on
the hand-built sequences, the kernel's host twin (`ops.track_step_host`: the same header the kernel compiles) against the Python
rule integer for integer, `matching.StreamTracker`'s padding with the twin in place of the launch, the C ABI of the new entry
points, and the twin under the address / undefined-behaviour sanitizers as a stand-alone program."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import track_cases as tc
from frmap_amd import _lib, frames, matching, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_box_iou_hand_values():
    iou = frames.box_iou
    assert iou((0, 0, 10, 10), (0, 0, 10, 10)) == 1.0
    assert iou((0, 0, 10, 10), (5, 0, 15, 10)) == 50 / 150
    assert iou((0, 0, 8, 1), (5, 0, 10, 1)) == 0.3 == 3 / 10                 # exactly the tracking threshold
    assert iou((0, 0, 10, 10), (10, 0, 20, 10)) == 0.0                        # touching: zero intersection over a positive union
    assert iou((0, 0, 10, 10), (11, 0, 20, 10)) == 0.0                        # apart
    assert iou((0, 0, 10, 10), (2, 2, 4, 4)) == 4 / 100                       # contained
    assert iou((0, 0, 0, 0), (0, 0, 0, 0)) == 0.0                             # union 0: the `else 0`
    assert iou((10, 10, 0, 0), (10, 10, 0, 0)) == 0.0                         # inverted boxes cross
    assert iou((0, 0, 10, 10), (5, 0, 15, 10)) == iou((5, 0, 15, 10), (0, 0, 10, 10))
    # float32 inputs are widened, the arithmetic is float64: 0.1f is not 0.1
    a, b = np.array([0, 0, 0.1, 1], F32), np.array([0, 0, 1, 1], F32)
    assert iou(a, b) == float(F32(0.1)) != 0.1
    assert isinstance(iou(a, b), float)
    assert frames.TRACKING_THRESHOLD == 0.3 and frames.DET_THRESH == 0.9


@pytest.mark.parametrize("case", tc.HAND, ids=[c[0].split()[0] for c in tc.HAND])
def test_track_boxes_on_the_hand_built_sequences(case):
    name, shape, steps, want_ids, want_next = case
    ids, states = tc.run_python(steps, shape)
    assert [i.tolist() for i in ids] == want_ids, name
    assert states[-1].next_id == want_next
    for k, (i, st) in enumerate(zip(ids, states)):
        assert i.dtype == np.int64
        if len(i):                                                            # the state is exactly the boxes that got an id
            got = i >= 0
            assert st.ids.tolist() == i[got].tolist() and np.array_equal(st.boxes, np.asarray(steps[k][0], F32)[got])
        else:                                                                 # an empty frame leaves the state as it is
            assert st is (states[k - 1] if k else st)
    for (prefix, k, i), roi in tc.HAND_ROIS.items():
        if name.startswith(prefix + " "):
            assert tc.want_rois(steps[k][0], steps[k][1], ids[k], shape)[i].tolist() == list(roi)


def _broken_run(variant, case):
    state, out = None, []
    for b, p in case[2]:
        i, state = tc.broken_track_boxes(variant, state, b, p, case[1])
        out.append(i.tolist())
    return out, state.next_id


def test_every_likely_mistake_fails_a_hand_built_sequence():
    """The hand-built sequences bite: the rule with any ONE of the mistakes a kernel is likely to make - the last of equal maxima,
    `>=` at the threshold, no matched flag, float32 IoU, tracks dropped on an empty frame, ids restarted, rounded coordinates, the
    probability compared in float64, ties resolved by lane instead of by index, untracked boxes kept in the state - gets at least
    one of them wrong, and the mistake-free restatement gets all of them right."""
    for case in tc.HAND:
        assert _broken_run(None, case) == (case[3], case[4]), case[0]
    caught = {v: [c[0].split()[0] for c in tc.HAND if _broken_run(v, c) != (c[3], c[4])] for v in tc.BROKEN}
    print(caught)
    assert all(caught.values()), caught
    assert "4a" in caught["last_max"] and "5a" in caught["ge_thresh"] and "3" in caught["no_matched_flag"]
    assert "1" in caught["clear_on_empty_frame"] and "2" in caught["reset_next_id"] and "7" in caught["prob_in_float64"]
    assert "4c" in caught["ties_by_lane"] and "6" in caught["keep_untracked_in_state"] and "9" in caught["round_coords"]


def test_track_boxes_state_and_arguments():
    st0 = frames.new_track_state()
    ids, st = frames.track_boxes(None, None, None, (100, 100))
    assert ids.shape == (0,) and st.next_id == 0 and st.boxes.shape == (0, 4)
    ids, st1 = frames.track_boxes(st0, [[10, 10, 50, 50]], [0.95], (100, 100, 3))           # lists, a 3-tuple shape
    assert ids.tolist() == [0] and st1.boxes.dtype == F32 and st1.next_id == 1 and st0.next_id == 0
    ids, st2 = frames.track_boxes(st1, [[10, 10, 50, 50]], [0.95], (100, 100), iou_thresh=1.0)   # IoU 1.0 is not > 1.0
    assert ids.tolist() == [1]
    ids, st2 = frames.track_boxes(st1, [[10, 10, 50, 50]], [0.95], (100, 100), det_thresh=0.96)
    assert ids.tolist() == [-1] and len(st2.ids) == 0 and st2.next_id == 1


def _compare_step(label, got_ids, got_rois, frame, counts, py_ids, shapes, M):
    for s, (boxes, probs) in enumerate(frame):
        n = counts[s]
        assert got_ids[s, :n].tolist() == py_ids[s].tolist(), (label, s)
        assert (got_ids[s, n:] == -1).all(), (label, s)
        want = np.zeros((M, 4), np.int32)
        want[:n] = tc.want_rois(boxes, probs, py_ids[s], shapes[s])
        assert np.array_equal(got_rois[s], want), (label, s)


def _compare_states(label, got, want):
    for s, (g, w) in enumerate(zip(got, want)):
        w = frames.new_track_state() if w is None else w
        assert g.next_id == w.next_id and g.ids.tolist() == w.ids.tolist() and np.array_equal(g.boxes, w.boxes), (label, s)


@pytest.mark.parametrize("use_probs", [True, False])
@pytest.mark.parametrize("S,M", tc.GRID)
def test_host_twin_equals_the_python_rule(S, M, use_probs):
    """`ops.track_step_host` == `frames.track_boxes` stream by stream over a moving scene: ids, crops (against `clip_boxes`) and the
    state after every step; half way the Python states are packed into a fresh buffer and the twin goes on from that."""
    steps = 6
    scene = tc.moving_scene(S, M, steps, 100 * S + M)
    seen = {int(c) for f in scene for b, _ in f for c in [len(b)]}
    assert {c for c in tc.COUNTS if c <= M} | {M} <= seen
    shapes = [(240, 320)] * S
    hw = np.array(shapes, np.int32)
    state = ops.track_state_host(S, M)
    py = [None] * S
    for k, frame in enumerate(scene):
        if not use_probs:
            frame = [(b, None) for b, _ in frame]
        boxes, probs, counts = tc.pad_step(frame, M, use_probs)
        ids, rois = ops.track_step_host(state, boxes, probs, counts, hw)
        py_ids = []
        for s, (b, p) in enumerate(frame):
            i, py[s] = frames.track_boxes(py[s], b, p, shapes[s])
            py_ids.append(i)
        _compare_step((S, M, k), ids, rois, frame, counts, py_ids, shapes, M)
        _compare_states((S, M, k), ops.track_state_unpack(state, S, M), py)
        if k == steps // 2:
            state = ops.track_state_pack(py, M)
    assert all(st.next_id > (1 if M > 1 else 0) for st in py)                # ids were handed out


@pytest.mark.parametrize("case", tc.HAND, ids=[c[0].split()[0] for c in tc.HAND])
def test_host_twin_on_the_hand_built_sequences(case):
    name, shape, steps, want_ids, want_next = case
    M = tc.hand_max_boxes(case)
    state = ops.track_state_host(2, M)                                       # the case in stream 1, stream 0 stays idle
    hw = np.array([(50, 50), shape], np.int32)
    for k, (b, p) in enumerate(steps):
        use_probs = any(q is not None for _, q in steps)
        boxes, probs, counts = tc.pad_step([(None, None), (b, p)], M, use_probs)
        ids, rois = ops.track_step_host(state, boxes, probs, counts, hw)
        assert ids[1, :counts[1]].tolist() == want_ids[k], (name, k)
        assert (ids[0] == -1).all() and (ids[1, counts[1]:] == -1).all() and not rois[0].any()
        assert np.array_equal(rois[1, :counts[1]], tc.want_rois(b, p, want_ids[k], shape)) and not rois[1, counts[1]:].any()
    got = ops.track_state_unpack(state, 2, M)
    assert got[1].next_id == want_next and got[0].next_id == 0 and len(got[0].ids) == 0


def test_host_twin_rejects_before_it_writes():
    S, M = 2, 8
    state = ops.track_state_host(S, M)
    scene = tc.moving_scene(S, M, 1, 5, counts=[[8, 3]])
    boxes, probs, counts = tc.pad_step(scene[0], M)
    hw = np.array([(240, 320)] * S, np.int32)
    ops.track_step_host(state, boxes, probs, counts, hw)
    before = state.copy()
    assert before.any()
    for bad in ([9, 3], [8, -1], [8, 1 << 30]):
        with pytest.raises(ValueError, match="count"):
            ops.track_step_host(state, boxes, probs, np.array(bad, np.int32), hw)
        assert np.array_equal(state, before)
    big = ops.track_state_host(1, 256)
    snap = big.copy()
    for m in (257, 1024):
        with pytest.raises(ValueError, match="max_boxes"):
            ops.track_step_host(big, np.zeros((1, m, 4), F32), None, np.zeros(1, np.int32), np.array([[10, 10]], np.int32))
    with pytest.raises(ValueError):
        ops.track_step_host(big, np.zeros((1, 0, 4), F32), None, np.zeros(1, np.int32), np.array([[10, 10]], np.int32))
    assert np.array_equal(big, snap)
    with pytest.raises(ValueError):
        ops.track_step_host(state[:-4], boxes, probs, counts, hw)                              # a state buffer that is too small
    with pytest.raises(ValueError):
        ops.track_state_bytes(1, 257)
    # the raw entry point: null pointers, and the library's usual error code
    lib = _lib.load()
    ids, rois = np.zeros((S, M), np.int32), np.zeros((S, M, 4), np.int32)
    good = [state.ctypes.data, boxes.ctypes.data, probs.ctypes.data, counts.ctypes.data, hw.ctypes.data, S, M, 0.9, 0.3, ids.ctypes.data,
            rois.ctypes.data]
    for pos in (0, 1, 3, 4, 9, 10):
        args = list(good)
        args[pos] = None
        assert lib.frmap_track_step_host(*args) == -1 and b"null pointer" in lib.frmap_last_error()
    assert np.array_equal(state, before)
    assert lib.frmap_track_step_host(None, None, None, None, None, 0, M, 0.9, 0.3, None, None) == 0     # no streams: nothing to do
    assert lib.frmap_track_state_bytes(3, 8) == 32 + 3 * 8 * 20 and lib.frmap_track_state_bytes(1, 257) == 0
    assert not ops.track_state_host(5, 7).any() and ops.track_state_host(5, 7).ctypes.data % 16 == 0


def test_stream_tracker_pads_and_unpads_with_the_host_twin():
    """`StreamTracker(device="cpu")` runs the twin where the launch would be: lists of different lengths, `None` streams, streams
    without probabilities, one frame shape for all or one per stream, reset and the id counters."""
    S, M = 4, 8
    scene = tc.moving_scene(S, M, 5, 77, counts=[[3, 0, 8, 1], [4, 2, 0, 1], [0, 0, 0, 0], [5, 3, 8, 2], [2, 8, 1, 0]])
    shapes = [(240, 320), (240, 320, 3), (200, 300), (240, 320)]
    tr = matching.StreamTracker(S, M, device="cpu")
    py = [None] * S
    for k, frame in enumerate(scene):
        boxes = [None if len(b) == 0 else (b.tolist() if s == 0 else b.astype(np.float64)) for s, (b, _) in enumerate(frame)]
        probs = [None if (len(b) == 0 or s == 3) else p for s, (b, p) in enumerate(frame)]     # stream 3 never has probabilities
        ids, rois = tr.step(boxes, probs, shapes)
        assert ids.shape == (S, M) and rois.shape == (S, M, 4)
        got = tr.unpad(ids)
        for s in range(S):
            want, py[s] = frames.track_boxes(py[s], boxes[s], probs[s], shapes[s])
            assert got[s].dtype == np.int64 and got[s].tolist() == want.tolist(), (k, s)
            r = np.zeros((M, 4), np.int32)
            r[:len(want)] = tc.want_rois(frame[s][0], probs[s], want, shapes[s])
            assert np.array_equal(rois[s], r), (k, s)
        assert tr.next_ids() == [0 if st is None else st.next_id for st in py]
    # all probabilities absent: the NULL path; one shape for all
    tr2 = matching.StreamTracker(2, 4, device="cpu", det_thresh=0.5, iou_thresh=0.5)
    b_pad, p_pad, c_pad, hw = tr2.pad([tc._b(tc.A), None], None, (100, 120))
    assert p_pad is None and c_pad.tolist() == [1, 0] and hw.tolist() == [[100, 120]] * 2 and b_pad.base is c_pad.base
    assert tr2.unpad(tr2.step([tc._b(tc.A), None], None, (100, 120))[0])[0].tolist() == [0]
    assert [i.tolist() for i in tr2.unpad(tr2.step([tc._b((20, 10, 60, 50)), tc._b(tc.A)], None, (100, 120))[0])] == [[0], [0]]   # IoU .6
    assert tr2.unpad(tr2.step([tc._b((40, 10, 80, 50)), None], None, (100, 120))[0])[0].tolist() == [1]                           # IoU .33
    assert tr2.next_ids() == [2, 1]
    tr2.reset(1)
    assert tr2.next_ids() == [2, 0] and len(ops.track_state_unpack(tr2.state, 2, 4)[1].ids) == 0
    tr2.reset()
    assert tr2.next_ids() == [0, 0]
    # too many boxes, too few entries, no shapes: refused before the state moves
    tr2.step([tc._b(tc.A), None], None, (100, 120))
    snap = tr2.state.copy()
    with pytest.raises(ValueError, match="max_boxes"):
        tr2.step([np.zeros((5, 4)), None], None, (100, 120))
    with pytest.raises(ValueError):
        tr2.step([None], None, (100, 120))
    with pytest.raises(ValueError):
        tr2.step([None, None], None)
    with pytest.raises(ValueError):
        tr2.reset(2)
    with pytest.raises(ValueError):
        matching.StreamTracker(1, 257, device="cpu")
    assert np.array_equal(tr2.state, snap)


def test_track_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_track_state_bytes", 2), ("frmap_track_step", 12), ("frmap_track_step_host", 11)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % sym, header)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
        assert hasattr(_lib.load(), sym)
    assert _lib.ABI_VERSION == 10 and _lib.load().frmap_abi_version() == 10
    build = open(os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc", "build.sh")).read()
    # track.hip is compiled, and an edit of track_rule.h (any header next to the sources) rebuilds the objects
    assert " track.hip " in build and 'for h in *.h ../../include/frmap_hip.h' in build and '[ "$h" -nt "$o" ]' in build
    assert os.path.isfile(os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc", "track_rule.h"))


def _hex(v):
    return "%08x" % np.asarray(v, F32).view(np.uint32)


def _seq_text(S, M, steps, use_probs, shapes):
    out = [f"seq {S} {M} {len(steps)} {int(use_probs)} 0.9 0.3"]
    for frame in steps:
        for s, (b, p) in enumerate(frame):
            n = 0 if b is None else len(b)
            words = [str(n), str(shapes[s][0]), str(shapes[s][1])]
            for i in range(n):
                words += [_hex(v) for v in np.asarray(b, F32)[i]]
                if use_probs:
                    words.append(_hex(1.0 if p is None else p[i]))
            out.append(" ".join(words))
    return "\n".join(out) + "\n"


SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _gpu_present():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_gpu_present(), reason="a sanitizer build is host-only work: nothing of it runs on a machine with a GPU")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to build the stand-alone sanitizer program with")
def test_twin_is_sanitizer_clean_as_a_stand_alone_program(tmp_path):
    """tools/track_twin_check.cpp (its own `main`, the twin's source and track_rule.h, nothing else) built with
    -fsanitize=address,undefined (runtimes linked statically: the program needs nothing from its environment, which is passed on
    as it is) and run directly on the hand-built sequences and the size grid: no report, and the output is `frames.track_boxes`'
    integer for integer.  Decided before any work: not on a machine with a GPU, and only where g++ can link an empty program with
    the sanitizers."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link an empty program with -fsanitize=address,undefined: no sanitizer runtimes installed")
    exe = str(tmp_path / "track_twin_check")
    csrc = os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN_FLAGS, "-I" + csrc, os.path.join(ROOT, "tools", "track_twin_check.cpp"),
           "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    jobs = []                                                                 # (S, M, steps [[(boxes, probs)] per stream], use_probs, shapes)
    for case in tc.HAND:
        use_probs = any(q is not None for _, q in case[2])
        jobs.append((1, tc.hand_max_boxes(case), [[st] for st in case[2]], use_probs, [case[1]]))
    for S, M in tc.GRID:
        for use_probs in (True, False):
            jobs.append((S, M, tc.moving_scene(S, M, 4, 9 * S + M), use_probs, [(240, 320)] * S))
    text = "".join(_seq_text(S, M, steps, up, shapes) for S, M, steps, up, shapes in jobs)
    text += "reject 2 8 9\nreject 2 8 -1\nreject 1 257 0\nreject 1 0 0\nreject -1 8 0\n"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], input=text, capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
    lines = iter(run.stdout.splitlines())
    for S, M, steps, use_probs, shapes in jobs:
        assert next(lines) == f"seq {S} {M} {len(steps)}"
        py = [None] * S
        for k, frame in enumerate(steps):
            for s, (b, p) in enumerate(frame):
                want, py[s] = frames.track_boxes(py[s], b, p if use_probs else None, shapes[s])
                n = len(want)
                ids = [int(v) for v in next(lines).split()[2:]]
                rois = np.array([int(v) for v in next(lines).split()[2:]], np.int32).reshape(M, 4)
                st = next(lines).split()
                assert ids == want.tolist() + [-1] * (M - n), (S, M, k, s)
                r = np.zeros((M, 4), np.int32)
                r[:n] = tc.want_rois(b, p if use_probs else None, want, shapes[s])
                assert np.array_equal(rois, r), (S, M, k, s)
                w = frames.new_track_state() if py[s] is None else py[s]
                assert [int(st[1]), int(st[2])] == [len(w.ids), w.next_id], (S, M, k, s)
                assert [int(v) for v in st[7::5]] == w.ids.tolist()
                assert [v for j in range(len(w.ids)) for v in st[3 + 5 * j:7 + 5 * j]] == [_hex(v) for v in w.boxes.reshape(-1)]
    assert [next(lines) for _ in range(5)] == ["reject refused untouched"] * 5
    # and on its own, without input: the program's self check
    alone = subprocess.run([exe], stdin=subprocess.DEVNULL, capture_output=True, text=True, env=env)
    assert alone.returncode == 0 and "self check passed" in alone.stdout, alone.stdout + alone.stderr
