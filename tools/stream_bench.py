#!/usr/bin/env python3
"""The frame loop as a step over S streams, two ways, on one device in one process.

Set-up: S in {1, 8, 32} streams of 1280x720 BGR frames, 4 boxes per frame with sides of 60 .. 400 px, 'cnn' in bf16 at 160x160
with get_embedding's 0.5 / 0.5 input normalisation, a 36-entry gallery.  Every step the boxes move by a few pixels (tracks
persist) and their sizes are redrawn within +-3 px (live video: no resize shape repeats).
  a   the path without the stream step: per stream `identify_boxes(what="embedding", normalize=True)` + `frames.track_boxes` -
      S crop launches, S model calls, S matches, S copies, the tracker in Python.
  b   `identify_streams` with a `StreamTracker`: one tracker launch, one crop launch, one model call, one match, one copy.
Measured with the frames on the host (as a capture delivers them: uploaded inside the timed call) and resident on the device.
Timing: host clock around one step ending in a device synchronise; every shape warmed up first; a and b alternate inside each
repeat (on the same boxes, each with its own tracker state); per (S, residence, path) the median over the repeats of the repeat's
mean step time, and the spread (max - min) of those.  Conditions, against path a: at S = 8 and S = 32 b is below a by more than the
larger spread; at S = 1 b is not slower than a beyond that spread.

--kernels-only S N: instead, run S streams x N boxes for a kernel trace taken from outside - N <= 8: 20 steps of `identify_streams`;
larger N: 5 steps of the tracker launch and the crop launch alone."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import frmap_amd
from frmap_amd import frames, matching, resize, synth

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32])
ap.add_argument("--boxes", type=int, default=4)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=10, help="timed steps per repeat")
ap.add_argument("--out", default=None, help="write the results as JSON here")
ap.add_argument("--kernels-only", type=int, nargs=2, metavar=("S", "N"), default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "stream_bench needs a GPU"
DEV, H, W, SIZE, NORM = "cuda", 720, 1280, (160, 160), ((.5, .5, .5), (.5, .5, .5))

rng = np.random.default_rng(17)
m = frmap_amd.get_model("cnn", 36)
m.load_state_dict(synth.calibrated_state_dict("cnn", synth.shapes_of(m), 1002))
m = m.to(DEV).eval().set_compute_dtype(torch.bfloat16).set_input_normalization(*NORM)
gal = frmap_amd.Gallery([f"id{i}" for i in range(36)], synth.unit_rows(3001, 36, 512), DEV)


class Scene:
    """S streams of n faces: centres drift, sizes are redrawn around each face's own size every step."""

    def __init__(self, S, n):
        self.size = rng.uniform(63, 397, (S, n, 2))
        self.pos = rng.uniform(0, [W - 400, H - 400], (S, n, 2))
        self.probs = np.full((S, n), 0.99, np.float32)

    def step(self):
        self.pos = np.clip(self.pos + rng.uniform(-4, 4, self.pos.shape), 0, [W - 400, H - 400])
        wh = self.size + rng.uniform(-3, 3, self.size.shape)
        return np.concatenate([self.pos, self.pos + wh], 2).astype(np.float32)


def path_a(fr, boxes, probs, states):
    out = []
    for s in range(len(fr)):
        res, kept = matching.identify_boxes(m, fr[s], boxes[s], gal, 1.0, probs=probs[s], what="embedding", normalize=True)
        ids, states[s] = frames.track_boxes(states[s], boxes[s], probs[s], fr[s].shape)
        out.append((res, kept, ids[kept]))
    return out


def path_b(fr, boxes, probs, tracker):
    return matching.identify_streams(m, fr, list(boxes), gal, tracker, 1.0, probs=list(probs), what="embedding", normalize=True)


if args.kernels_only:
    S, n = args.kernels_only
    sc = Scene(S, n)
    fr = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(DEV)] * S
    tr = matching.StreamTracker(S, max(n, 1), DEV)
    steps = 20 if n <= 8 else 5
    for _ in range(steps):
        boxes = sc.step()
        if n <= 8:
            path_b(fr, boxes, sc.probs, tr)
        else:                                                  # the tracker and the crop launch alone
            tr.step(list(boxes), list(sc.probs), (H, W))
            r5 = np.concatenate([np.concatenate([np.full((n, 1), s, np.int32), frames.clip_boxes(boxes[s], sc.probs[s], (H, W))[0]], 1)
                                 for s in range(S)])
            resize.crop_resize_u8(fr, r5, SIZE, bgr=True, device=DEV)
    torch.cuda.synchronize()
    print(f"kernels-only: {steps} steps of {S} streams x {n} boxes done")
    sys.exit(0)

results = []
for S in args.streams:
    host_frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(S)]
    dev_frames = [torch.from_numpy(f).to(DEV) for f in host_frames]
    for where, fr in (("host", host_frames), ("device", dev_frames)):
        sc = Scene(S, args.boxes)
        st_a, tr_b = [None] * S, matching.StreamTracker(S, max(args.boxes, 1), DEV)
        for _ in range(3):                                     # warm-up: kernels, plans, allocator pools for this S
            boxes = sc.step()
            ra, rb = path_a(fr, boxes, sc.probs, st_a), path_b(fr, boxes, sc.probs, tr_b)
        torch.cuda.synchronize()
        for (a_res, a_kept, a_ids), (b_res, b_kept, b_ids) in zip(ra, rb):      # the two paths agree on what they return
            assert a_kept.tolist() == b_kept.tolist() and a_ids.tolist() == b_ids.tolist()
            assert [r[0] for r in a_res] == [r[0] for r in b_res]
        per_rep = {"a": [], "b": []}
        for rep in range(args.reps):
            total = {"a": 0.0, "b": 0.0}
            for _ in range(args.iters):
                boxes = sc.step()
                for p in (("a", "b") if rep % 2 == 0 else ("b", "a")):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if p == "a":
                        path_a(fr, boxes, sc.probs, st_a)
                    else:
                        path_b(fr, boxes, sc.probs, tr_b)
                    torch.cuda.synchronize()
                    total[p] += time.perf_counter() - t0
            for p in total:
                per_rep[p].append(1e3 * total[p] / args.iters)
        row = {"S": S, "boxes": args.boxes, "frames": where}
        for p in ("a", "b"):
            row[p] = {"median_ms": statistics.median(per_rep[p]), "spread_ms": max(per_rep[p]) - min(per_rep[p])}
        gap, sp = row["a"]["median_ms"] - row["b"]["median_ms"], max(row["a"]["spread_ms"], row["b"]["spread_ms"])
        row["a_minus_b_ms"], row["condition_met"] = gap, bool(gap > sp if S > 1 else gap > -sp)
        results.append(row)
        print(f"S={S:3d} {where:6s} frames  a: {row['a']['median_ms']:8.3f} ms (spread {row['a']['spread_ms']:6.3f})  "
              f"b: {row['b']['median_ms']:8.3f} ms (spread {row['b']['spread_ms']:6.3f})  a - b = {gap:+.3f} ms against {sp:.3f}: "
              f"condition {'met' if row['condition_met'] else 'NOT met'}", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
