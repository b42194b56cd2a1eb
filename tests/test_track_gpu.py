"""GPU: the tracker kernel (`ops.track_step`) against its host twin integer for integer - the size grid, 300 streams, every
hand-built sequence, a non-default stream - and `matching.identify_streams` (one tracker launch, one crop launch, one model call,
one match, one copy for S streams) against per-frame `identify_boxes` and per-stream `frames.track_boxes`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import frmap_amd  # noqa: E402
import track_cases as tc  # noqa: E402
from frmap_amd import frames, matching, ops, synth  # noqa: E402
from test_configs_gpu import DIST_BOUND  # noqa: E402  (the project's gate on a distance's error per compute dtype)

DEV = "cuda"
F32 = np.float32


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _run_both(scene, S, M, shapes, use_probs, label):
    """Step the kernel and the twin through a scene: ids and crops equal at every step, the state buffers equal at the end."""
    hw = np.array([s[:2] for s in shapes], np.int32)
    host, dev = ops.track_state_host(S, M), ops.track_state(S, M, DEV)
    hw_d = _dev(hw)
    for k, frame in enumerate(scene):
        boxes, probs, counts = tc.pad_step(frame, M, use_probs)
        want_ids, want_rois = ops.track_step_host(host, boxes, probs, counts, hw)
        ids, rois = ops.track_step(dev, _dev(boxes), _dev(probs), _dev(counts), hw_d)
        assert ids.shape == (S, M) and rois.shape == (S, M, 4) and ids.dtype == rois.dtype == torch.int32
        assert np.array_equal(ids.cpu().numpy(), want_ids), (label, k)
        assert np.array_equal(rois.cpu().numpy(), want_rois), (label, k)
    got, want = ops.track_state_unpack(dev, S, M), ops.track_state_unpack(host, S, M)
    for s in range(S):
        assert got[s].next_id == want[s].next_id and got[s].ids.tolist() == want[s].ids.tolist(), (label, s)
        assert np.array_equal(got[s].boxes, want[s].boxes), (label, s)
    return want


@pytest.mark.parametrize("use_probs", [True, False])
@pytest.mark.parametrize("S,M", tc.GRID)
def test_kernel_equals_the_host_twin_on_the_grid(S, M, use_probs):
    scene = tc.moving_scene(S, M, 5, 100 * S + M)
    states = _run_both(scene, S, M, [(240, 320)] * S, use_probs, (S, M))
    assert all(st.next_id > (1 if M > 1 else 0) for st in states)


def test_kernel_300_streams_with_idle_streams_between_busy_ones():
    """More wavefronts than one pass of workgroups; every third stream has no detections at a step, so its state must survive
    while its neighbours in the same workgroup move."""
    S, M, steps = 300, 8, 5
    rng = np.random.default_rng(300)
    counts = rng.integers(1, M + 1, (steps, S))
    for k in range(steps):
        counts[k, (k % 3)::3] = 0
    scene = tc.moving_scene(S, M, steps, 301, counts=counts)
    shapes = [(240 - (s % 5) * 20, 320 - (s % 7) * 10) for s in range(S)]          # frame sizes differ per stream
    states = _run_both(scene, S, M, shapes, True, "S=300")
    assert sum(len(st.ids) for st in states) > S                                   # tracks were alive at the end


def test_kernel_on_every_hand_built_sequence():
    """All hand-built sequences at once: case c is stream c of one tracker (its own frame size), shorter cases idle at the end.
    Against the ids written out in track_cases, not only against the twin."""
    S, M = len(tc.HAND), max(tc.hand_max_boxes(c) for c in tc.HAND)
    steps = max(len(c[2]) for c in tc.HAND)
    scene = [[c[2][k] if k < len(c[2]) else (None, None) for c in tc.HAND] for k in range(steps)]
    shapes = [c[1] for c in tc.HAND]
    hw_d = _dev(np.array(shapes, np.int32))
    dev = ops.track_state(S, M, DEV)
    for k, frame in enumerate(scene):
        boxes, probs, counts = tc.pad_step(frame, M)
        ids, rois = ops.track_step(dev, _dev(boxes), _dev(probs), _dev(counts), hw_d)
        ids, rois = ids.cpu().numpy(), rois.cpu().numpy()
        for c, case in enumerate(tc.HAND):
            want = case[3][k] if k < len(case[3]) else []
            assert ids[c, :counts[c]].tolist() == want and (ids[c, counts[c]:] == -1).all(), (case[0], k)
            r = np.zeros((M, 4), np.int32)
            r[:counts[c]] = tc.want_rois(frame[c][0], frame[c][1], want, shapes[c])
            assert np.array_equal(rois[c], r), (case[0], k)
    got = ops.track_state_unpack(dev, S, M)
    assert [st.next_id for st in got] == [c[4] for c in tc.HAND]
    _run_both(scene, S, M, shapes, False, "hand, no probabilities")               # the NULL-probs launch on the same inputs


def test_kernel_on_a_side_stream_and_rejections():
    S, M = 3, 8
    scene = tc.moving_scene(S, M, 3, 55, counts=[[8, 3, 5]] * 3)
    hw = np.array([(240, 320)] * S, np.int32)
    host, dev = ops.track_state_host(S, M), ops.track_state(S, M, DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for frame in scene:
            boxes, probs, counts = tc.pad_step(frame, M)
            want_ids, want_rois = ops.track_step_host(host, boxes, probs, counts, hw)
            ids, rois = ops.track_step(dev, _dev(boxes), _dev(probs), _dev(counts), _dev(hw))
            ids_h = ids.to("cpu", non_blocking=False)                              # a read on the same stream
            assert np.array_equal(ids_h.numpy(), want_ids) and np.array_equal(rois.cpu().numpy(), want_rois)
    side.synchronize()
    # rejected before any launch: the state is untouched
    before = dev.clone()
    b, p, c, h = _dev(boxes), _dev(probs), _dev(counts), _dev(hw)
    with pytest.raises(ValueError, match="max_boxes"):
        ops.track_step(dev, torch.zeros((1, 257, 4), device=DEV), None, c[:1], h[:1])
    with pytest.raises(ValueError):
        ops.track_step(dev, b, p[:, :4], c, h)
    with pytest.raises(ValueError):
        ops.track_step(dev[:64], b, p, c, h)
    with pytest.raises(RuntimeError):
        ops.track_step(dev, b.cpu(), p, c, h)
    tr = matching.StreamTracker(S, M, DEV)
    with pytest.raises(ValueError, match="max_boxes"):
        tr.step([np.zeros((9, 4), F32), None, None], None, (240, 320))
    torch.cuda.synchronize()
    assert torch.equal(dev, before) and not bool(tr.state.any())
    # device counts beyond max_boxes are data the host never saw: clamped by the kernel, nothing outside a stream's slots moves
    big = _dev(np.array([8, M + 1, -1], np.int32))                            # just outside: the padding behind it is benign
    ids, rois = ops.track_step(dev, b, p, big, h)
    want_ids, _ = ops.track_step_host(host, boxes, probs, np.array([8, 8, 0], np.int32), hw)
    assert np.array_equal(ids.cpu().numpy(), want_ids)


# --------------------------------------------------------------------------------------------------------------------------------
# identify_streams
# --------------------------------------------------------------------------------------------------------------------------------
_rng = np.random.default_rng(20250301)


def _blocks(H, W):
    """Coloured 16-pixel blocks under noise (as test_frames_gpu's frame): crops of different places embed differently."""
    base = np.kron(_rng.integers(0, 256, ((H + 15) // 16, (W + 15) // 16, 3)), np.ones((16, 16, 1)))[:H, :W]
    return (0.75 * base + 0.25 * _rng.integers(0, 256, (H, W, 3))).astype(np.uint8)


FRAMES = [_blocks(720, 1280), _blocks(480, 640), _blocks(360, 500)]
_BASE = [np.array([[100.3, 50.9, 300.2, 400.7], [-20.5, -3.2, 90.9, 80.1], [640.0, 200.0, 890.0, 460.0], [1200.0, 600.0, 1400.0, 900.0],
                   [500.0, 300.0, 500.4, 380.0]]),                                 # the last one is empty after truncation
         np.array([[30.0, 40.0, 200.0, 260.0], [300.5, 100.5, 460.5, 260.5], [500.0, 300.0, 700.0, 520.0]]),
         np.array([[10.0, 10.0, 120.0, 150.0], [250.0, 100.0, 420.0, 330.0]])]
_PROBS = [np.array([0.99, 0.95, 0.999, 0.93, 0.99], F32), np.array([0.97, 0.92, 0.5], F32), np.array([0.9, 0.98], F32)]


def _steps():
    """3 steps of 3 streams: the boxes move by a few pixels (tracks persist) and change their order; stream 1 has no detection
    at the second step; at the third a box of stream 0 drops below the threshold and a new one appears in stream 2."""
    out = []
    for k in range(3):
        step = []
        for s in range(3):
            b = (_BASE[s] + k * np.array([3.25, -2.5, 3.25, -2.5])).astype(F32)
            p = _PROBS[s].copy()
            if k == 2 and s == 0:
                p[2] = 0.4
            if k == 2 and s == 2:
                b, p = np.concatenate([b, np.array([[300, 20, 380, 95]], F32)]), np.concatenate([p, np.array([0.96], F32)])
            order = np.roll(np.arange(len(b)), k)
            step.append((b[order], p[order]))
        if k == 1:
            step[1] = (None, None)
        out.append(step)
    return out


def _landmarks(boxes, tilt):
    if boxes is None:
        return None
    x1, y1, x2, y2 = boxes.T.astype(np.float64)
    w, h = x2 - x1, y2 - y1
    pts = np.stack([np.stack([x1 + .3 * w, y1 + .4 * h + tilt * h], 1), np.stack([x1 + .7 * w, y1 + .4 * h - tilt * h], 1),
                    np.stack([x1 + .5 * w, y1 + .6 * h], 1)], 1)
    return pts


def _model(mt, sd, dtype):
    m = frmap_amd.get_model(mt, 36)
    m.load_state_dict(sd)
    return m.to(DEV).eval().set_compute_dtype(dtype)


def _count_calls(obj, name):
    """Count the calls of ``obj.name`` through a wrapper set on the instance; returns the list that grows by one per call."""
    calls = []
    orig = getattr(obj, name)

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    setattr(obj, name, counted)
    return calls


def _count_forward(m):
    return _count_calls(m, "forward")


def _per_frame(m, steps, refs, thresh, lms=None, **kw):
    """The path that exists without this feature: `identify_boxes` per frame."""
    return [[matching.identify_boxes(m, FRAMES[s], b, refs, thresh, probs=p, landmarks=None if lms is None else lms[k][s], **kw)
             for s, (b, p) in enumerate(step)] for k, step in enumerate(steps)]


def _gallery_and_threshold(m, steps, dtype, seed, lms=None, **kw):
    """Enrol every second kept face of the first step among unrelated unit rows; the threshold sits in the middle of the widest gap
    between the distances the per-frame path reports, and that gap is many times the gate - so no name hangs on rounding."""
    other = synth.unit_rows(seed, 13, 512)
    mk = dict(kw)
    mk.pop("what", None), mk.pop("normalize", None)
    embs = []
    for s, (b, p) in enumerate(steps[0]):
        if kw.get("what") == "embedding":
            e = m.get_embedding(ops.normalize_u8(matching._box_crops(m, FRAMES[s], b, p, (160, 160), frames.DET_THRESH)[0], (.5,) * 3, (.5,) * 3)[0])
            e = ops.l2_normalize(e.to(torch.float32), 1e-12)
        else:
            e = matching.embed_boxes(m, FRAMES[s], b, p, landmarks=None if lms is None else lms[0][s], **mk)[0]
        embs.extend(e[i:i + 1].detach().float().cpu() for i in range(0, e.shape[0], 2))
    refs = [{"name": f"other{i}", "embedding": other[i:i + 1]} for i in range(6)]
    refs += [{"name": f"face{i}", "embedding": e} for i, e in enumerate(embs)]
    refs += [{"name": f"other{i}", "embedding": other[i:i + 1]} for i in range(6, 13)]
    d = sorted(r[1] for step in _per_frame(m, steps, refs, float("inf"), lms, **kw) for res, _ in step for r in res)
    gaps = [(b - a, (a + b) / 2) for a, b in zip(d, d[1:])]
    gap, thresh = max(gaps)
    assert gap > 16 * DIST_BOUND[dtype], (gap, d)
    return refs, thresh


def _check_streams(got, want, py_ids, exact, dtype, label):
    for s, ((res, kept, fid), (wres, wkept)) in enumerate(zip(got, want)):
        assert kept.tolist() == wkept.tolist() and len(res) == len(wres), (label, s)
        assert [(r[0], r[2]) for r in res] == [(w[0], w[2]) for w in wres], (label, s)
        err = max([abs(r[1] - w[1]) for r, w in zip(res, wres)], default=0.0)
        print(f"identify_streams {label} stream {s}: max |dist - per-frame identify_boxes| = {err:.3e} (gate {DIST_BOUND[dtype]:.1e}; "
              f"{'bit-equal required' if exact else 'default planning'}); names {[r[0] for r in res]}; face_ids {None if fid is None else fid.tolist()}")
        assert err == 0.0 if exact else err < DIST_BOUND[dtype], (label, s, err)
        if py_ids is None:
            assert fid is None
        else:
            assert fid.dtype == np.int64 and fid.tolist() == py_ids[s][kept].tolist(), (label, s)


def _run_streams(m, steps, refs, thresh, dtype, label, lms=None, calls=None, **kw):
    """3 steps of `identify_streams` with a tracker, under batch-invariant planning (bit-equal distances) and under default planning
    (within the gate), against per-frame `identify_boxes` and per-stream `frames.track_boxes`."""
    want = _per_frame(m, steps, refs, thresh, lms, **kw)
    assert {r[0][:4] for step in want for res, _ in step for r in res} >= {"face", "Unkn"}
    calls = _count_forward(m) if calls is None else calls
    for exact in (True, False):
        ops.set_batch_invariant(True if exact else None)
        try:
            if exact:
                want_x = _per_frame(m, steps, refs, thresh, lms, **kw)
            tr = matching.StreamTracker(3, 8, DEV)
            py = [None] * 3
            for k, step in enumerate(steps):
                if calls is not None:
                    del calls[:]
                frames_in = FRAMES if k % 2 == 0 else [torch.from_numpy(f).to(DEV) for f in FRAMES]      # host frames, device frames
                got = matching.identify_streams(m, frames_in, [b for b, _ in step], refs, tr, thresh, probs=[p for _, p in step],
                                                landmarks=None if lms is None else lms[k], **kw)
                if calls is not None:
                    assert len(calls) == 1, (label, k, len(calls))
                py_ids = []
                for s, (b, p) in enumerate(step):
                    i, py[s] = frames.track_boxes(py[s], b, p, FRAMES[s].shape)
                    py_ids.append(i)
                _check_streams(got, (want_x if exact else want)[k], py_ids, exact, dtype, f"{label} step {k}")
                if k == 1:
                    assert got[1][0] == [] and got[1][1].shape == (0,) and got[1][2].shape == (0,)
            assert tr.next_ids() == [st.next_id for st in py]
            assert py[0].next_id == 4 and py[2].next_id == 3 and py[1].next_id == 2        # ids persisted; one new face in stream 2
        finally:
            ops.set_batch_invariant(None)
            if calls is not None:
                del calls[:]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_identify_streams_equals_per_frame_identify_boxes_and_track_boxes(dtype, calibrated_sd):
    m = _model("arcface", calibrated_sd("arcface"), dtype)
    steps = _steps()
    refs, thresh = _gallery_and_threshold(m, steps, dtype, 5151)
    _run_streams(m, steps, refs, thresh, dtype, f"arcface forward {dtype}")
    # without a tracker: the same results, face_ids None; a [S, H, W, 3] stack of equal frames, on the host and on the device
    got = matching.identify_streams(m, FRAMES, [b for b, _ in steps[0]], refs, None, thresh, probs=[p for _, p in steps[0]])
    _check_streams(got, _per_frame(m, steps[:1], refs, thresh)[0], None, False, dtype, "no tracker")
    stack = np.stack([FRAMES[1], FRAMES[1][::-1].copy()])
    b, p = steps[0][1]
    want = [matching.identify_boxes(m, stack[i], b, refs, thresh, probs=p) for i in range(2)]
    for st in (stack, torch.from_numpy(stack).to(DEV)):
        got = matching.identify_streams(m, st, [b, b], refs, None, thresh, probs=[p, p])
        _check_streams(got, want, None, False, dtype, "stack")
    # embed_streams: embed_boxes' rows per stream, and the row offsets
    ops.set_batch_invariant(True)
    try:
        emb, kepts, offsets, ids = matching.embed_streams(m, FRAMES, [b for b, _ in steps[0]], [p for _, p in steps[0]])
        assert ids is None and offsets.tolist() == [0, 4, 6, 8] and emb.shape[0] == 8
        for s, (b, p) in enumerate(steps[0]):
            e, kept = matching.embed_boxes(m, FRAMES[s], b, p)
            assert kept.tolist() == kepts[s].tolist() and torch.equal(e, emb[offsets[s]:offsets[s + 1]])
    finally:
        ops.set_batch_invariant(None)


def test_identify_streams_with_landmarks_and_margin(calibrated_sd):
    dtype = torch.float16
    m = _model("arcface", calibrated_sd("arcface"), dtype)
    steps = _steps()
    lms = [[_landmarks(b, 0.04 * (s + 1) * (-1) ** k) for s, (b, _) in enumerate(step)] for k, step in enumerate(steps)]
    refs, thresh = _gallery_and_threshold(m, steps, dtype, 5252, lms, margin=0.4)
    _run_streams(m, steps, refs, thresh, dtype, "arcface aligned, margin 0.4", lms, margin=0.4)


def test_identify_streams_embedding_mode_feeds_the_handle_uint8_crops(calibrated_sd):
    dtype = torch.bfloat16
    m = _model("cnn", calibrated_sd("cnn"), dtype).set_input_normalization((.5, .5, .5), (.5, .5, .5))
    assert m.model_handle() is not None
    steps = _steps()
    refs, thresh = _gallery_and_threshold(m, steps, dtype, 5353, what="embedding", normalize=True)
    # on this path the model call is the handle's `embed_and_match` (model.forward is never entered): exactly one per step
    calls = _count_calls(m.model_handle(), "embed_and_match")
    _run_streams(m, steps, refs, thresh, dtype, "cnn embedding (uint8 handle path)", calls=calls, what="embedding", normalize=True)


def test_identify_streams_with_no_kept_box_makes_no_model_call(calibrated_sd):
    m = _model("arcface", calibrated_sd("arcface"), torch.float16)
    calls = _count_forward(m)
    tr = matching.StreamTracker(3, 8, DEV)
    steps = _steps()
    refs = [{"name": "x", "embedding": synth.unit_rows(1, 1, 512)}]
    matching.identify_streams(m, FRAMES, [b for b, _ in steps[0]], refs, tr, probs=[p for _, p in steps[0]])
    assert len(calls) == 1 and tr.next_ids() == [4, 2, 2]
    del calls[:]
    low = [(b, np.full(len(b), 0.3, F32)) for b, _ in steps[0]]
    got = matching.identify_streams(m, FRAMES, [b for b, _ in low], refs, tr, probs=[p for _, p in low])
    assert len(calls) == 0
    for res, kept, fid in got:
        assert res == [] and kept.shape == (0,) and fid.shape == (0,)
    assert all(len(st.ids) == 0 for st in ops.track_state_unpack(tr.state, 3, 8)) and tr.next_ids() == [4, 2, 2]   # cleared, not reset
    got = matching.identify_streams(m, FRAMES, [None] * 3, refs, tr)
    assert len(calls) == 0 and [g[0] for g in got] == [[], [], []]
    got = matching.identify_streams(m, FRAMES, [b for b, _ in steps[0]], [], tr, probs=[p for _, p in steps[0]])       # empty refs
    assert len(calls) == 0 and got[0][0] == [("Unknown", float("inf"), None)] * 4 and got[0][2].tolist() == [4, 5, 6, 7]
    with pytest.raises(ValueError):
        matching.identify_streams(m, FRAMES[:2], [None] * 2, refs, tr)                                                   # 2 frames, 3 streams
    with pytest.raises(ValueError):
        matching.identify_streams(m, FRAMES, [None] * 3, refs, tr, what="logits")
    # a probability that is not finite, a tracker on another device: refused before the tracker's state moves
    snap = tr.state.clone()
    bad = [p.copy() for _, p in steps[0]]
    bad[2][1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        matching.identify_streams(m, FRAMES, [b for b, _ in steps[0]], refs, tr, probs=bad)
    with pytest.raises(ValueError, match="lives on"):
        matching.identify_streams(m, FRAMES, [b for b, _ in steps[0]], refs, matching.StreamTracker(3, 8, "cpu"))
    torch.cuda.synchronize()
    assert torch.equal(tr.state, snap) and len(calls) == 0
