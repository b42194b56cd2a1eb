"""GPU: the track-template kernel (`ops.track_fuse`) against its host twin bit for bit - every hand-built sequence, the size grid,
a 300-step track, D = 4096, a non-default stream, untouched guard bytes around everything it writes - with ids and counts built
by the test (no tracker kernel runs), and `matching.identify_streams(..., templates=)` over a 6-frame clip of 3 streams against
the same call without templates, `frames.fuse_tracks` + `compare_faces`, and the tracker's own state."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import frmap_amd  # noqa: E402
import fuse_cases as fc  # noqa: E402
from frmap_amd import _lib, frames, matching, ops, synth  # noqa: E402

DEV = "cuda"
F32 = np.float32


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _run_both(label, S, M, D, steps, decay, host_rows=False):
    """Step the kernel and the twin through a sequence: templates, weights and the logical state equal at every step."""
    host, dev = ops.track_fuse_state_host(S, M, D), ops.track_fuse_state(S, M, D, DEV)
    for k, (ids, counts, emb, rows) in enumerate(steps):
        want_fused, want_frames = ops.track_fuse_host(host, ids, counts, emb, rows, decay)
        if host_rows:
            fused, nframes = ops.track_fuse(dev, _dev(ids), _dev(counts), _dev(emb), rows, decay, host_counts=counts)
        else:
            fused, nframes = ops.track_fuse(dev, _dev(ids), _dev(counts), _dev(emb), _dev(rows), decay)
        assert fused.shape == (len(rows), D) and nframes.shape == (len(rows),) and fused.dtype == nframes.dtype == torch.float32
        assert fc.same_bits(fused.cpu().numpy(), want_fused), (label, k)
        assert fc.same_bits(nframes.cpu().numpy(), want_frames), (label, k)
        fc.check_states((label, k), ops.track_fuse_state_unpack(dev, S, M, D), ops.track_fuse_state_unpack(host, S, M, D), D)
    return ops.track_fuse_state_unpack(host, S, M, D)


@pytest.mark.parametrize("case", fc.HAND, ids=[c[0].split()[0] for c in fc.HAND])
def test_kernel_on_the_hand_built_sequences(case):
    """Against the sums written out in fuse_cases, not only against the twin; the case is stream 1 of 2, stream 0 stays idle."""
    name, decay, steps, wants = case
    M = fc.hand_max_boxes(case)
    dev = ops.track_fuse_state(2, M, 2, DEV)
    for k, (step, want) in enumerate(zip(steps, wants)):
        ids, counts, emb, rows = fc.hand_step_arrays(step, M)
        ids2, counts2 = np.concatenate([np.zeros_like(ids), ids]), np.concatenate([[0], counts]).astype(np.int32)
        rows2 = rows + np.array([1, 0], np.int32)
        fused, nframes = ops.track_fuse(dev, _dev(ids2), _dev(counts2), _dev(emb), rows2, decay, host_counts=counts2)
        got = ops.track_fuse_state_unpack(dev, 2, M, 2)
        fc.check_hand_step((name, k), want, fused.cpu().numpy(), nframes.cpu().numpy(), got[1])
        assert len(got[0].ids) == 0


@pytest.mark.parametrize("S,M", fc.GRID)
def test_kernel_equals_the_host_twin_on_the_grid(S, M):
    """S = 5 streams, up to 256 faces per stream for the workgroup's 4 waves, counts on both sides of 4 and of 64, every D of the
    grid (float4 rows and element-wise rows), rows of all streams shuffled together."""
    for D in fc.D_GRID:
        decay = (1.0, 0.9, 0.5)[(S + M + D) % 3]
        steps = fc.random_steps(S, M, D, 5, 1000 * S + 10 * M + D)
        states = _run_both((S, M, D), S, M, D, steps, decay, host_rows=D % 2 == 0)
        assert any(len(st.ids) for st in states) or M == 1


def test_kernel_follows_one_track_for_300_steps():
    states = _run_both("300 steps", 1, 2, 8, fc.long_track(300), 0.9)
    assert 9.99 < states[0].weights[states[0].ids.tolist().index(0)] <= 10.0


def test_kernel_at_dim_4096():
    _run_both("D = 4096", 2, 2, 4096, fc.random_steps(2, 2, 4096, 4, 4096, counts=[[2, 1], [2, 2], [0, 2], [2, 2]]), 0.9)


def test_kernel_on_a_side_stream_and_rejections():
    S, M, D = 3, 8, 64
    steps = fc.random_steps(S, M, D, 3, 77, counts=[[8, 3, 5]] * 3)
    host, dev = ops.track_fuse_state_host(S, M, D), ops.track_fuse_state(S, M, D, DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for ids, counts, emb, rows in steps:
            want_fused, want_frames = ops.track_fuse_host(host, ids, counts, emb, rows, 0.9)
            fused, nframes = ops.track_fuse(dev, _dev(ids), _dev(counts), _dev(emb), _dev(rows), 0.9)
            assert fc.same_bits(fused.to("cpu", non_blocking=False).numpy(), want_fused)     # a read on the same stream
            assert fc.same_bits(nframes.cpu().numpy(), want_frames)
    side.synchronize()
    # rejected before any launch: the state is untouched
    before = dev.clone()
    i, c, e = _dev(ids), _dev(counts), _dev(emb)
    s1 = int(np.flatnonzero(rows[:, 0] == 1)[0])
    for match, bad in (("detection", (s1, 1, 3)), ("detection", (s1, 1, -1)), ("stream", (0, 0, 3)), ("same detection", None)):
        r = rows.copy()
        if bad is None:
            r[1] = r[0]
        else:
            r[bad[0], bad[1]] = bad[2]
        with pytest.raises(ValueError, match=match):
            ops.track_fuse(dev, i, c, e, r, 0.9, host_counts=counts)
    with pytest.raises(ValueError, match="host_counts"):
        ops.track_fuse(dev, i, c, e, rows, 0.9)
    for decay in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            ops.track_fuse(dev, i, c, e, _dev(rows), decay)
    with pytest.raises(ValueError, match="state holds"):
        ops.track_fuse(dev[:64], i, c, e, _dev(rows), 0.9)
    with pytest.raises(ValueError):
        ops.track_fuse(dev, i, c[:2], e, _dev(rows), 0.9)
    with pytest.raises(ValueError):
        ops.track_fuse(dev, i, c, e, _dev(rows[:-1]), 0.9)
    with pytest.raises(RuntimeError):
        ops.track_fuse(dev, i, c, e.cpu(), _dev(rows), 0.9)
    with pytest.raises(ValueError, match="max_boxes"):
        ops.track_fuse(dev, torch.zeros((1, 257), dtype=torch.int32, device=DEV), c[:1], e, _dev(rows), 0.9)
    torch.cuda.synchronize()
    assert torch.equal(dev, before)


def test_kernel_leaves_everything_else_untouched():
    """The raw entry point on buffers cut out of one guarded allocation: the bytes before and after the state, after `fused` and
    after `frames`, and every byte of an idle stream's slots between two busy streams stay as they were - also when `counts` and
    `rows` are device data no host checked: counts beyond max_boxes, rows that name another stream's detections beyond its
    count, negative indices and streams that do not exist."""
    S, M, D, G = 3, 8, 36, 4096
    nbytes = ops.track_fuse_state_bytes(S, M, D)
    pitch = (D + 3) & ~3
    steps = fc.random_steps(S, M, D, 4, 5, counts=[[8, 0, 8], [5, 0, 8], [8, 0, 3], [8, 0, 8]], bad=0.0)
    N = max(len(st[3]) for st in steps) + 6
    f_off = G + nbytes + G
    n_off = f_off + 4 * N * D + G
    total = n_off + 4 * N + G
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device=DEV)
    state = buf[G:G + nbytes]
    state.zero_()
    # the idle stream 1: a live-looking meta record and a pattern in all of its slots, both banks
    layout = np.zeros(nbytes, np.uint8)
    s_off = nbytes - 8 * S * M * pitch
    w_off, i_off = s_off - 8 * S * M, s_off - 16 * S * M
    layout[8:16] = 1
    layout[i_off + 8 * M:i_off + 16 * M] = 1
    layout[w_off + 8 * M:w_off + 16 * M] = 1
    layout[s_off + 8 * M * pitch:s_off + 16 * M * pitch] = 1
    idle = torch.from_numpy(layout.astype(bool)).to(DEV)
    state[idle] = torch.arange(int(layout.sum()), device=DEV).to(torch.uint8)
    state[8:16] = torch.tensor([2, 0, 0, 0, 1, 0, 0, 0], dtype=torch.uint8, device=DEV)          # P = 2, bank 1
    snap = buf.clone()
    lib = _lib.load()
    for k, (ids, counts, emb, rows) in enumerate(steps):
        rows = np.concatenate([rows, np.array([[1, 0], [1, 7], [0, 8], [2, -1], [3, 0], [-1, 2]], np.int32)])   # none names a detection
        emb = np.concatenate([emb, np.full((6, D), 3.5, F32)])
        counts = counts.copy()
        counts[2] += 100 * (k % 2)                                           # beyond max_boxes at every other step: clamped
        n = len(rows)
        buf[f_off:] = snap[f_off:]                                           # the steps have different n: the pattern again behind `fused` and `frames`
        d_ids, d_counts, d_emb, d_rows = _dev(ids), _dev(counts), _dev(emb), _dev(rows)
        lib_rc = lib.frmap_track_fuse(state.data_ptr(), d_ids.data_ptr(), d_counts.data_ptr(), d_emb.data_ptr(), d_rows.data_ptr(), n, S, M, D,
                                      0.9, buf[f_off:].data_ptr(), buf[n_off:].data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert lib_rc == 0
        torch.cuda.synchronize()
        fused = buf[f_off:f_off + 4 * n * D].view(torch.float32).view(n, D).cpu().numpy()
        nframes = buf[n_off:n_off + 4 * n].view(torch.float32).cpu().numpy()
        assert fc.same_bits(fused[-6:], emb[-6:]) and not nframes[-6:].any(), k          # passed through
        assert nframes[:-6].any()
        for lo, hi in ((0, G), (G + nbytes, f_off), (f_off + 4 * n * D, n_off), (n_off + 4 * n, total)):
            assert torch.equal(buf[lo:hi], snap[lo:hi]), (k, lo)
        assert torch.equal(state[idle], snap[G:G + nbytes][idle]), k
    got = ops.track_fuse_state_unpack(state, S, M, D)
    assert len(got[0].ids) and len(got[2].ids) and got[1].ids.shape == (2,)


def test_kernel_passes_the_loser_of_two_rows_of_one_detection_through():
    """Device `rows` no host checked that name one detection twice: one of the two rows (either) is pooled, the other comes back as
    it came with frames = 0 - no row of `fused` is left unwritten."""
    S, M, D = 1, 4, 8
    dev = ops.track_fuse_state(S, M, D, DEV)
    ids, counts = np.array([[0, 1, 0, 0]], np.int32), np.array([2], np.int32)
    rows = np.array([[0, 0], [0, 1], [0, 0]], np.int32)
    emb = np.arange(3 * D, dtype=F32).reshape(3, D) + 1
    fused, nframes = ops.track_fuse(dev, _dev(ids), _dev(counts), _dev(emb), _dev(rows), 1.0)
    nframes = nframes.cpu().numpy()
    assert fc.same_bits(fused.cpu().numpy(), emb)                            # w = 1: the template is the row; passed through: the row
    assert nframes[1] == 1.0 and sorted(nframes[[0, 2]].tolist()) == [0.0, 1.0]
    st = ops.track_fuse_state_unpack(dev, S, M, D)[0]
    assert st.ids.tolist() == [0, 1] and st.weights.tolist() == [1.0, 1.0]
    assert fc.same_bits(st.sums[0], emb[0 if nframes[0] else 2]) and fc.same_bits(st.sums[1], emb[1])


# --------------------------------------------------------------------------------------------------------------------------------
# identify_streams(..., templates=)
# --------------------------------------------------------------------------------------------------------------------------------
_rng = np.random.default_rng(20250917)


def _blocks(H, W):
    base = np.kron(_rng.integers(0, 256, ((H + 15) // 16, (W + 15) // 16, 3)), np.ones((16, 16, 1)))[:H, :W]
    return (0.75 * base + 0.25 * _rng.integers(0, 256, (H, W, 3))).astype(np.uint8)


FRAMES = [_blocks(360, 640), _blocks(240, 320), _blocks(300, 500)]
_BASE = [np.array([[100.3, 50.9, 300.2, 300.7], [-20.5, -3.2, 90.9, 80.1], [400.0, 100.0, 600.0, 330.0], [300.0, 200.0, 300.4, 280.0]]),
         np.array([[30.0, 40.0, 150.0, 200.0], [170.5, 60.5, 300.5, 220.5]]),
         np.array([[10.0, 10.0, 120.0, 150.0], [250.0, 100.0, 420.0, 290.0]])]       # stream 0's last box is empty after truncation
_PROBS = [np.array([0.99, 0.95, 0.999, 0.99], F32), np.array([0.97, 0.92], F32), np.array([0.9, 0.98], F32)]


def _clip():
    """6 steps of 3 streams: the boxes move by a few pixels (tracks persist) and change their order; stream 1 has no detection
    at the third step; at the fifth a box of stream 0 drops below the threshold (its track ends) and a new face appears in
    stream 2."""
    out = []
    for k in range(6):
        step = []
        for s in range(3):
            b = (_BASE[s] + k * np.array([3.25, -2.5, 3.25, -2.5])).astype(F32)
            p = _PROBS[s].copy()
            if k == 4 and s == 0:
                p[2] = 0.4
            if k >= 4 and s == 2:
                b, p = np.concatenate([b, np.array([[300, 20, 380, 95]], F32)]), np.concatenate([p, np.array([0.96], F32)])
            order = np.roll(np.arange(len(b)), k)
            step.append((b[order], p[order]))
        if k == 2:
            step[1] = (None, None)
        out.append(step)
    return out


def _counted(monkeypatch, obj, name):
    calls = []
    orig = getattr(obj, name)

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    monkeypatch.setattr(obj, name, counted)
    return calls


@pytest.mark.parametrize("what,normalize", [("forward", False), ("embedding", True)])
def test_identify_streams_with_templates(what, normalize, calibrated_sd, monkeypatch):
    m = frmap_amd.get_model("arcface", 36)
    m.load_state_dict(calibrated_sd("arcface"))
    m = m.to(DEV).eval().set_compute_dtype(torch.float16)
    clip = _clip()
    kw = dict(what=what, normalize=normalize)
    # a small gallery: every second face of the first step among unrelated unit rows
    e0 = matching.embed_streams(m, FRAMES, [b for b, _ in clip[0]], [p for _, p in clip[0]])[0].float().cpu()
    other = synth.unit_rows(77, 9, 512)
    refs = [{"name": f"other{i}", "embedding": other[i:i + 1]} for i in range(5)]
    refs += [{"name": f"face{i}", "embedding": e0[i:i + 1]} for i in range(0, e0.shape[0], 2)]
    refs += [{"name": f"other{i}", "embedding": other[i:i + 1]} for i in range(5, 9)]
    thresh, decay, S, M = 0.9, 0.9, 3, 8
    plain, tr = matching.StreamTracker(S, M, DEV), matching.StreamTracker(S, M, DEV)
    tpl = matching.TrackTemplates(tr, 512, decay)
    counters = {n: _counted(monkeypatch, ops, n) for n in ("track_step", "track_fuse", "match_top1")}
    counters["forward"] = _counted(monkeypatch, m, "forward" if what == "forward" else "get_embedding")
    py_track, py_tpl = [None] * S, [None] * S
    seen_frames = set()
    for k, step in enumerate(clip):
        boxes, probs = [b for b, _ in step], [p for _, p in step]
        want = matching.identify_streams(m, FRAMES, boxes, refs, plain, thresh, probs=probs, **kw)
        emb, kepts, offsets, _ = matching.embed_streams(m, FRAMES, boxes, probs)                # the per-frame embeddings
        if normalize:                                                        # (ArcFaceNet's eval forward IS get_embedding)
            emb = ops.l2_normalize(emb.to(torch.float32), 1e-12)
        for c in counters.values():
            del c[:]
        got = matching.identify_streams(m, FRAMES, boxes, refs, tr, thresh, probs=probs, templates=tpl, **kw)
        assert {n: len(c) for n, c in counters.items()} == {"track_step": 1, "track_fuse": 1, "match_top1": 1, "forward": 1}, k
        emb = emb.cpu().numpy()
        states = tpl.unpack()
        tracker_states = ops.track_state_unpack(tr.state, S, M)
        for s, (b, p) in enumerate(step):
            res, kept, fid, tres, tframes = got[s]
            assert res == want[s][0] and kept.tolist() == want[s][1].tolist() and fid.tolist() == want[s][2].tolist(), (k, s)
            assert fid.dtype == np.int64 and tframes.dtype == F32 and len(tres) == len(res) == len(kept)
            ids, py_track[s] = frames.track_boxes(py_track[s], b, p, FRAMES[s].shape)
            rows = emb[offsets[s]:offsets[s + 1]]
            fused, nfr, py_tpl[s] = frames.fuse_tracks(py_tpl[s], ids, rows, kept, decay)
            assert fc.same_bits(tframes, nfr), (k, s, tframes, nfr)
            if k == 0:                                                       # a first frame's template is the frame's embedding
                assert tres == res and nfr.tolist() == [1.0] * len(kept)
            for i in range(len(kept)):
                probe = torch.from_numpy(fused[i:i + 1]).to(DEV)
                if normalize:
                    probe = ops.l2_normalize(probe, 1e-12)
                assert tres[i] == matching.compare_faces(probe, refs, thresh), (k, s, i)
            seen_frames.update(float(v) for v in nfr)
            assert states[s].ids.tolist() == tracker_states[s].ids.tolist() == ([] if py_track[s] is None else py_track[s].ids.tolist()), (k, s)
        fc.check_states(k, states, py_tpl, 512)
        if k == 2:
            assert got[1][0] == [] and got[1][3] == [] and got[1][4].shape == (0,)
    assert len(seen_frames) >= 5 and 1.0 in seen_frames                      # tracks grew old, and new ones began
    # no kept box at all: no model call, no match - the templates still follow the tracker (cleared, like its state)
    for c in counters.values():
        del c[:]
    low = [np.full(len(b), 0.3, F32) for b, _ in clip[0]]
    got = matching.identify_streams(m, FRAMES, [b for b, _ in clip[0]], refs, tr, thresh, probs=low, templates=tpl, **kw)
    assert {n: len(c) for n, c in counters.items()} == {"track_step": 1, "track_fuse": 1, "match_top1": 0, "forward": 0}
    assert all(g[0] == [] and g[3] == [] and g[4].shape == (0,) for g in got) and all(len(st.ids) == 0 for st in tpl.unpack())
    # embed_streams with templates: a first frame's template is the embedding itself
    out = matching.embed_streams(m, FRAMES, [b for b, _ in clip[0]], [p for _, p in clip[0]], tracker=tr, templates=tpl)
    assert len(out) == 6 and torch.equal(out[4], out[0].to(torch.float32)) and out[5].tolist() == [1.0] * out[0].shape[0]
    assert any(len(st.ids) for st in tpl.unpack())
    # refused before the tracker's state moves
    snap, tsnap = tr.state.clone(), tpl.state.clone()
    args = (m, FRAMES, [b for b, _ in clip[1]], refs)
    with pytest.raises(ValueError, match="tracker"):
        matching.identify_streams(*args, None, thresh, probs=[p for _, p in clip[1]], templates=tpl, **kw)
    with pytest.raises(ValueError, match="built on this tracker"):
        matching.identify_streams(*args, plain, thresh, probs=[p for _, p in clip[1]], templates=tpl, **kw)
    with pytest.raises(ValueError, match="hold 64 values"):
        matching.identify_streams(*args, tr, thresh, probs=[p for _, p in clip[1]], templates=matching.TrackTemplates(tr, 64), **kw)
    with pytest.raises(ValueError, match="tracker"):
        matching.embed_streams(m, FRAMES, [b for b, _ in clip[1]], templates=tpl)
    torch.cuda.synchronize()
    assert torch.equal(tr.state, snap) and torch.equal(tpl.state, tsnap)
    # StreamTracker.reset clears the templates with the tracks: the ids restart at 0
    tr.reset(0)
    assert len(tpl.unpack()[0].ids) == 0 and any(len(st.ids) for st in tpl.unpack())
    tr.reset()
    assert not bool(tpl.state.any()) and tr.next_ids() == [0] * S
