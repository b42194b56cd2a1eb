"""CPU: track templates - `frames.fuse_tracks` (the rule in plain Python) on the hand-built sequences with every sum written out,
the decay's two roundings against numpy float32 and against a deliberately fused emulation, the kernel's host twin
(`ops.track_fuse_host`: the same headers the kernel compiles) against the Python rule bit for bit over the size grid and a
300-step track, `matching.TrackTemplates` on a CPU tracker, the rejections, the C ABI of the new entry points, and the twin under
the address / undefined-behaviour sanitizers as a stand-alone program.  Every comparison is on the bits of the float32 values."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fuse_cases as fc
from frmap_amd import _lib, frames, matching, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
HAND_IDS = [c[0].split()[0] for c in fc.HAND]


@pytest.mark.parametrize("case", fc.HAND, ids=HAND_IDS)
def test_fuse_tracks_on_the_hand_built_sequences(case):
    name, decay, steps, wants = case
    state = None
    for k, ((ids, rws), want) in enumerate(zip(steps, wants)):
        emb = np.array([e for _, e in rws], F32).reshape(len(rws), 2)
        before = state
        fused, nframes, state = frames.fuse_tracks(state, ids, emb, [d for d, _ in rws], decay)
        assert fused.dtype == F32 and nframes.dtype == F32 and state.weights.dtype == F32 and state.sums.dtype == F32
        fc.check_hand_step((name, k), want, fused, nframes, state)
        if len(ids) == 0:
            assert state is before                                           # an empty frame hands the same state back


def test_fuse_tracks_arguments():
    with pytest.raises(ValueError, match="outside"):
        frames.fuse_tracks(None, [0, 1], np.zeros((1, 2), F32), [2])          # a detection index >= n
    with pytest.raises(ValueError, match="outside"):
        frames.fuse_tracks(None, [0, 1], np.zeros((1, 2), F32), [-1])
    with pytest.raises(ValueError, match="outside"):
        frames.fuse_tracks(None, [], np.zeros((1, 2), F32), [0])              # an empty frame has no detection to name
    with pytest.raises(ValueError, match="same detection"):
        frames.fuse_tracks(None, [0, 1], np.zeros((2, 2), F32), [1, 1])
    for decay in (0.0, -0.5, 1.5, np.nan):
        with pytest.raises(ValueError, match="decay"):
            frames.fuse_tracks(None, [0], np.zeros((1, 2), F32), [0], decay)
    with pytest.raises(ValueError):
        frames.fuse_tracks(None, [0], np.zeros(2, F32), [0])                  # emb must be [r, D]
    _, _, st = frames.fuse_tracks(None, [0], np.ones((1, 2), F32), [0])
    with pytest.raises(ValueError, match="values"):
        frames.fuse_tracks(st, [0], np.ones((1, 3), F32), [0])
    fused, nframes, st2 = frames.fuse_tracks(st, [0], np.zeros((0, 2), F32), [])           # no rows at all: carried over
    assert fused.shape == (0, 2) and nframes.shape == (0,) and st2.ids.tolist() == [0] and st2.weights.tolist() == [1.0]


def _decay_inputs(D=64, steps=12, seed=4):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(D) * 3).astype(F32) for _ in range(steps)]


@pytest.mark.parametrize("decay", [1.0, 0.5, 0.9])
def test_decay_is_a_float32_product_then_a_float32_sum(decay):
    """The reference is numpy float32, product then sum - two roundings.  For 0.9 a deliberately FUSED emulation (decay * s + e in
    float64, rounded once - what a contracted FMA returns) must differ on these inputs, so an implementation that fuses fails."""
    es = _decay_inputs()
    d32 = F32(decay)
    s, w = es[0].copy(), F32(1)
    s_fused, state = es[0].copy(), None
    differs = False
    for k, e in enumerate(es):
        fused, nframes, state = frames.fuse_tracks(state, [0], e[None], [0], decay)
        if k:
            t = d32 * s                                                      # float32 array * float32 scalar: rounded once
            assert t.dtype == F32
            s = t + e
            w = F32(F32(d32 * w) + F32(1))
            s_fused = (np.float64(d32) * s_fused.astype(np.float64) + e.astype(np.float64)).astype(F32)
        assert fc.same_bits(state.sums[0], s) and fc.same_bits(state.weights, [w]) and fc.same_bits(nframes, [w]), k
        assert fc.same_bits(fused[0], s / w), k
        differs |= not fc.same_bits(s, s_fused)
    assert differs == (decay == 0.9), "0.5 and 1.0 scale exactly (fusing changes nothing); 0.9 does not"
    # the twin makes the same two roundings
    host = ops.track_fuse_state_host(1, 1, len(es[0]))
    for e in es:
        ops.track_fuse_host(host, np.zeros((1, 1), np.int32), np.ones(1, np.int32), e[None], np.zeros((1, 2), np.int32), decay)
    got = ops.track_fuse_state_unpack(host, 1, 1, len(es[0]))[0]
    assert fc.same_bits(got.sums[0], s) and fc.same_bits(got.weights, [w])
    assert (decay != 0.9) or not fc.same_bits(got.sums[0], s_fused)


def _run_twin_against_python(label, S, M, D, steps, decay):
    host, py = ops.track_fuse_state_host(S, M, D), [None] * S
    assert not host.any() and host.ctypes.data % 16 == 0
    for k, step in enumerate(steps):
        ids, counts, emb, rows = step
        fused, nframes = ops.track_fuse_host(host, ids, counts, emb, rows, decay)
        want_fused, want_frames = fc.python_step(py, step, decay)
        assert fc.same_bits(fused, want_fused) and fc.same_bits(nframes, want_frames), (label, k)
        fc.check_states((label, k), ops.track_fuse_state_unpack(host, S, M, D), py, D)
    return py


@pytest.mark.parametrize("case", fc.HAND, ids=HAND_IDS)
def test_host_twin_on_the_hand_built_sequences(case):
    name, decay, steps, wants = case
    M = fc.hand_max_boxes(case)
    host = ops.track_fuse_state_host(1, M, 2)
    for k, (step, want) in enumerate(zip(steps, wants)):
        ids, counts, emb, rows = fc.hand_step_arrays(step, M)
        fused, nframes = ops.track_fuse_host(host, ids, counts, emb, rows, decay)
        fc.check_hand_step((name, k), want, fused, nframes, ops.track_fuse_state_unpack(host, 1, M, 2)[0])


@pytest.mark.parametrize("S,M", fc.GRID)
def test_host_twin_equals_the_python_rule(S, M):
    for D in fc.D_GRID:
        decay = (1.0, 0.9, 0.5)[(S + M + D) % 3]
        steps = fc.random_steps(S, M, D, 5, 1000 * S + 10 * M + D)
        py = _run_twin_against_python((S, M, D), S, M, D, steps, decay)
        seen = {int(c) for st in steps for c in st[1]}
        assert {M, 0} <= seen
        assert any(st is not None and len(st.ids) for st in py) or M == 1


def test_host_twin_follows_one_track_for_300_steps():
    steps = fc.long_track(300)
    py = _run_twin_against_python("300 steps", 1, 2, 8, steps, 0.9)
    w = py[0].weights[py[0].ids.tolist().index(0)]
    assert 9.99 < w <= 10.0                                                  # 1 / (1 - 0.9): the weight of a long track converges


def test_host_twin_rejects_before_it_writes():
    S, M, D = 2, 8, 6
    host = ops.track_fuse_state_host(S, M, D)
    ids, counts, emb, rows = fc.random_steps(S, M, D, 1, 3, counts=[[8, 3]], bad=0.0)[0]
    ops.track_fuse_host(host, ids, counts, emb, rows, 1.0)
    before = host.copy()
    assert before.any() and len(rows) >= 3

    def refused(match, ids=ids, counts=counts, emb=emb, rows=rows, decay=1.0, state=host):
        with pytest.raises(ValueError, match=match):
            ops.track_fuse_host(state, ids, counts, emb, rows, decay)
        assert np.array_equal(host, before)
    s1 = int(np.flatnonzero(rows[:, 0] == 1)[0])
    bad = rows.copy()
    bad[s1, 1] = 3                                                            # == counts[1]
    refused("detection", rows=bad)
    bad[s1, 1] = -1
    refused("detection", rows=bad)
    bad = rows.copy()
    bad[0, 0] = 2
    refused("stream", rows=bad)
    bad = rows.copy()
    bad[1] = bad[0]
    refused("same detection", rows=bad)
    for c in ([9, 3], [8, -1]):
        refused("count", counts=np.array(c, np.int32))
    refused("detection", counts=np.array([8, 0], np.int32))                  # an empty frame has no detection to name
    for decay in (0.0, -1.0, 1.0001, np.nan):
        refused("decay", decay=decay)
    refused("state holds", state=host[:-4])
    with pytest.raises(ValueError, match="max_boxes"):
        ops.track_fuse_host(host, np.zeros((1, 257), np.int32), np.zeros(1, np.int32), np.zeros((0, D), F32), np.zeros((0, 2), np.int32))
    with pytest.raises(ValueError, match="dim"):
        ops.track_fuse_host(host, np.zeros((1, 8), np.int32), np.zeros(1, np.int32), np.zeros((0, 4097), F32), np.zeros((0, 2), np.int32))
    for args in ((1, 257, 4), (1, 0, 4), (1, 4, 0), (1, 4, 4097), (-1, 4, 4)):
        with pytest.raises(ValueError):
            ops.track_fuse_state_bytes(*args)
    assert np.array_equal(host, before)
    # the raw entry points: null pointers, the library's usual error code, and the stated layout
    lib = _lib.load()
    fused, nframes = np.zeros((len(rows), D), F32), np.zeros(len(rows), F32)
    good = [host.ctypes.data, ids.ctypes.data, counts.ctypes.data, emb.ctypes.data, rows.ctypes.data, len(rows), S, M, D, 1.0,
            fused.ctypes.data, nframes.ctypes.data]
    for pos in (0, 1, 2, 3, 4, 10, 11):
        args = list(good)
        args[pos] = None
        assert lib.frmap_track_fuse_host(*args) == -1 and b"null pointer" in lib.frmap_last_error()
    assert np.array_equal(host, before)
    assert lib.frmap_track_fuse_host(None, None, None, None, None, 0, 0, M, D, 1.0, None, None) == 0          # no streams: nothing to do
    assert lib.frmap_track_fuse_state_bytes(3, 8, 6) == 32 + 3 * 2 * 8 * (4 + 4 + 4 * 8)
    assert lib.frmap_track_fuse_state_bytes(1, 257, 4) == 0 and lib.frmap_track_fuse_state_bytes(1, 4, 4097) == 0
    # the device entry refuses host tensors and unchecked host rows without a GPU
    import torch
    with pytest.raises(RuntimeError):
        ops.track_fuse(torch.zeros(64, dtype=torch.uint8), torch.zeros((1, 1), dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                       torch.zeros((1, 4)), np.zeros((1, 2), np.int32), host_counts=np.ones(1, np.int32))


def test_track_templates_on_a_cpu_tracker_follow_its_ids():
    """`TrackTemplates` on a `StreamTracker(device="cpu")`: the twin where the launch would be.  After every step the template ids
    are the tracker state's ids, the templates are `fuse_tracks` of the rows, and `StreamTracker.reset` clears them."""
    import track_cases as tc
    S, M, D = 3, 8, 5
    tr = matching.StreamTracker(S, M, device="cpu")
    assert tr.device_counts is None
    tpl = matching.TrackTemplates(tr, D, decay=0.9)
    rng = np.random.default_rng(8)
    scene = tc.moving_scene(S, M, 6, 21, counts=[[3, 8, 1], [4, 0, 2], [3, 8, 2], [0, 0, 0], [5, 3, 8], [2, 8, 1]])
    py = [None] * S
    for k, frame in enumerate(scene):
        ids, _ = tr.step([b for b, _ in frame], [p for _, p in frame], (240, 320))
        assert np.array_equal(tr.device_counts, tr.counts)
        rows = np.array([(s, i) for s in range(S) for i in range(tr.counts[s]) if (i + k) % 3], np.int32).reshape(-1, 2)
        emb = rng.standard_normal((len(rows), D)).astype(F32)
        fused, nframes = tpl.step(ids, emb, rows)
        want_fused, want_frames = fc.python_step(py, (ids, tr.counts, emb, rows), 0.9)
        assert fc.same_bits(fused, want_fused) and fc.same_bits(nframes, want_frames), k
        got = tpl.unpack()
        fc.check_states(k, got, py, D)
        assert [g.ids.tolist() for g in got] == [t.ids.tolist() for t in ops.track_state_unpack(tr.state, S, M)]
    assert any(len(g.ids) for g in tpl.unpack())
    with pytest.raises(ValueError, match="detection"):
        tpl.step(ids, emb[:1], np.array([[0, M]], np.int32))
    with pytest.raises(ValueError, match="values"):
        tpl.step(ids, np.zeros((1, D + 1), F32), np.array([[0, 0]], np.int32))
    tr.reset(1)
    assert len(tpl.unpack()[1].ids) == 0 and any(len(g.ids) for g in tpl.unpack())
    tr.reset()
    assert not tpl.state.any() and tr.next_ids() == [0] * S
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError, match="decay"):
            matching.TrackTemplates(tr, D, decay=bad)
    with pytest.raises(ValueError):
        matching.TrackTemplates(None, D)
    with pytest.raises(ValueError):
        matching.TrackTemplates(tr, 4097)
    with pytest.raises(ValueError, match="not stepped"):
        matching.TrackTemplates(matching.StreamTracker(1, 2, device="cpu"), D).step(np.zeros((1, 2), np.int32), np.zeros((0, D), F32),
                                                                                    np.zeros((0, 2), np.int32))


def test_track_fuse_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_track_fuse_state_bytes", 3), ("frmap_track_fuse", 13), ("frmap_track_fuse_host", 12)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % sym, header)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
        assert hasattr(_lib.load(), sym)
    assert _lib.ABI_VERSION == 10 and _lib.load().frmap_abi_version() == 10
    build = open(os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc", "build.sh")).read()
    # track_fuse.hip is compiled, and an edit of its rule or twin header (any header next to the sources) rebuilds the objects
    assert " track_fuse.hip " in build and 'for h in *.h ../../include/frmap_hip.h' in build and '[ "$h" -nt "$o" ]' in build
    for h in ("track_fuse_rule.h", "track_fuse_twin.h"):
        assert os.path.isfile(os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc", h))
    for name in ("track_fuse_state", "track_fuse", "track_fuse_host"):
        assert callable(getattr(ops, name))
    assert matching.TrackTemplates is __import__("frmap_amd").TrackTemplates


def _hex(v):
    return "%08x" % np.asarray(v, F32).view(np.uint32)


def _seq_text(S, M, D, decay, steps):
    out = [f"seq {S} {M} {D} {len(steps)} {_hex(decay)}"]
    for ids, counts, emb, rows in steps:
        for s in range(S):
            out.append(" ".join([str(int(counts[s]))] + [str(int(v)) for v in ids[s]]))
        out.append(str(len(rows)))
        for r in range(len(rows)):
            out.append(" ".join([str(int(rows[r, 0])), str(int(rows[r, 1]))] + [_hex(v) for v in emb[r]]))
    return "\n".join(out) + "\n"


SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
SAN_SHAPES = [(1, 1, 1), (5, 64, 3), (2, 65, 36), (1, 256, 65), (2, 5, 513), (1, 2, 4096)]


def _gpu_present():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_gpu_present(), reason="a sanitizer build is host-only work: nothing of it runs on a machine with a GPU")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to build the stand-alone sanitizer program with")
def test_twin_is_sanitizer_clean_as_a_stand_alone_program(tmp_path):
    """tools/track_fuse_check.cpp (its own `main`, the twin's source and the rule headers, nothing else) built with
    -fsanitize=address,undefined (runtimes linked statically) and run directly on the hand-built sequences and on random ones in
    buffers of exactly the stated sizes: no report, and the output is `frames.fuse_tracks`' bit for bit.  Decided before any work:
    not on a machine with a GPU, and only where g++ can link an empty program with the sanitizers."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link an empty program with -fsanitize=address,undefined: no sanitizer runtimes installed")
    exe = str(tmp_path / "track_fuse_check")
    csrc = os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN_FLAGS, "-I" + csrc, os.path.join(ROOT, "tools", "track_fuse_check.cpp"),
           "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    jobs = []                                                                 # (S, M, D, decay, steps)
    for name, decay, steps, _ in fc.HAND:
        M = fc.hand_max_boxes((name, decay, steps))
        jobs.append((1, M, 2, decay, [fc.hand_step_arrays(st, M) for st in steps]))
    for S, M, D in SAN_SHAPES:
        jobs.append((S, M, D, 0.9, fc.random_steps(S, M, D, 4, 7 * S + M + D)))
    text = "".join(_seq_text(*job) for job in jobs)
    text += "reject 2 8 4 3 1 3\nreject 2 8 4 3 2 0\nreject 2 8 4 3 0 -1\nreject 2 8 4 9 0 0\nreject 2 8 4 3 dup 0\nreject 1 257 4 1 0 0\nreject 1 8 4097 1 0 0\n"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], input=text, capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
    lines = iter(run.stdout.splitlines())
    for S, M, D, decay, steps in jobs:
        assert next(lines) == f"seq {S} {M} {D} {len(steps)}"
        py = [None] * S
        for k, step in enumerate(steps):
            want_fused, want_frames = fc.python_step(py, step, decay)
            assert next(lines).split()[1:] == [_hex(v) for v in want_fused.reshape(-1)], (S, M, D, k)
            assert next(lines).split()[1:] == [_hex(v) for v in want_frames], (S, M, D, k)
            for s in range(S):
                w = frames.new_template_state(D) if py[s] is None else py[s]
                st = next(lines).split()
                assert int(st[1]) == len(w.ids), (S, M, D, k, s)
                per = 2 + D
                assert [int(v) for v in st[2::per]] == w.ids.tolist()
                assert st[3::per] == [_hex(v) for v in w.weights]
                assert [v for j in range(len(w.ids)) for v in st[4 + per * j:4 + per * j + D]] == [_hex(v) for v in w.sums.reshape(-1)]
    assert [next(lines) for _ in range(7)] == ["reject refused untouched"] * 7
    # and on its own, without input: the program's self check
    alone = subprocess.run([exe], stdin=subprocess.DEVNULL, capture_output=True, text=True, env=env)
    assert alone.returncode == 0 and "self check passed" in alone.stdout, alone.stdout + alone.stderr
