#!/usr/bin/env python3
"""What track templates add to a step of the frame loop, on one device in one process.

Set-up (stream_bench.py's): S in {1, 8, 32} streams of 1280x720 BGR frames resident on the device, 4 boxes per frame with sides of
60 .. 400 px, 'cnn' in bf16 at 160x160 with get_embedding's 0.5 / 0.5 input normalisation, a 36-entry gallery,
`what="embedding", normalize=True`.  Every step the boxes move by a few pixels (tracks persist) and their sizes are redrawn
within +-3 px.
  a   `identify_streams` with a `StreamTracker`, the model's input normalisation set: tracker, crops, model + match as one call on
      the model handle (uint8 crops), one copy.
  c   the same call on a model without `set_input_normalization`: the embed-then-match route (normalise, model, normalise, match).
  b   c with `templates=`: crops, model, tracker, ONE `track_fuse` launch, normalise, one match over 2N probes, one copy.
b - c is what the templates add on the route they run on; c - a is what that route costs against the handle's fused call, which
is no cost of the templates.  b and c must agree bit for bit on what they share (checked after the warm-up).
Timing: host clock around one step ending in a device synchronise; every shape warmed up first; the paths alternate inside each
repeat (on the same boxes, each with its own tracker); per (S, path) the median over the repeats of the repeat's mean step time,
and the spread (max - min) of those.  Reported: b - c against the larger of their spreads, and c - a.

--kernels-only S: instead, 20 steps of path b for S streams, for a kernel trace taken from outside."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import frmap_amd
from frmap_amd import matching, synth

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32])
ap.add_argument("--boxes", type=int, default=4)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=10, help="timed steps per repeat")
ap.add_argument("--decay", type=float, default=0.9)
ap.add_argument("--out", default=None, help="write the results as JSON here")
ap.add_argument("--kernels-only", type=int, metavar="S", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "track_fuse_bench needs a GPU"
DEV, H, W, NORM = "cuda", 720, 1280, ((.5, .5, .5), (.5, .5, .5))

rng = np.random.default_rng(17)
m = frmap_amd.get_model("cnn", 36)
sd = synth.calibrated_state_dict("cnn", synth.shapes_of(m), 1002)
m.load_state_dict(sd)
m = m.to(DEV).eval().set_compute_dtype(torch.bfloat16).set_input_normalization(*NORM)
m2 = frmap_amd.get_model("cnn", 36)                           # the same weights, no input normalisation set: the embed-then-match route
m2.load_state_dict(sd)
m2 = m2.to(DEV).eval().set_compute_dtype(torch.bfloat16)
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


def step(model, fr, boxes, probs, tracker, templates=None):
    return matching.identify_streams(model, fr, list(boxes), gal, tracker, 1.0, probs=list(probs), what="embedding", normalize=True,
                                     templates=templates)


def trackers(S):
    tr = [matching.StreamTracker(S, max(args.boxes, 1), DEV) for _ in range(3)]
    return tr[0], tr[1], tr[2], matching.TrackTemplates(tr[1], 512, args.decay)


if args.kernels_only:
    S = args.kernels_only
    sc = Scene(S, args.boxes)
    fr = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(DEV)] * S
    _, tr, _, tpl = trackers(S)
    for _ in range(20):
        step(m2, fr, sc.step(), sc.probs, tr, tpl)
    torch.cuda.synchronize()
    print(f"kernels-only: 20 steps of {S} streams x {args.boxes} boxes with templates done")
    sys.exit(0)

results = []
for S in args.streams:
    fr = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(DEV) for _ in range(S)]
    sc = Scene(S, args.boxes)
    tr_a, tr_b, tr_c, tpl = trackers(S)
    run = {"a": lambda bx: step(m, fr, bx, sc.probs, tr_a), "b": lambda bx: step(m2, fr, bx, sc.probs, tr_b, tpl),
           "c": lambda bx: step(m2, fr, bx, sc.probs, tr_c)}
    for _ in range(3):                                         # warm-up: kernels, plans, allocator pools for this S
        boxes = sc.step()
        ra, rb, rc = run["a"](boxes), run["b"](boxes), run["c"](boxes)
    torch.cuda.synchronize()
    for a, b, c in zip(ra, rb, rc):                            # b and c share a route: bit for bit; a: the same boxes and ids
        assert c[0] == b[0] and c[1].tolist() == b[1].tolist() and c[2].tolist() == b[2].tolist()
        assert a[1].tolist() == b[1].tolist() and a[2].tolist() == b[2].tolist()
        assert len(b[3]) == len(b[1]) and (b[4] >= 1).all()     # every face has a template
    per_rep = {p: [] for p in "abc"}
    for rep in range(args.reps):
        total = {p: 0.0 for p in "abc"}
        for _ in range(args.iters):
            boxes = sc.step()
            for p in ("abc", "bca", "cab")[rep % 3]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run[p](boxes)
                torch.cuda.synchronize()
                total[p] += time.perf_counter() - t0
        for p in total:
            per_rep[p].append(1e3 * total[p] / args.iters)
    row = {"S": S, "boxes": args.boxes, "frames": "device"}
    for p in "abc":
        row[p] = {"median_ms": statistics.median(per_rep[p]), "spread_ms": max(per_rep[p]) - min(per_rep[p])}
    row["b_minus_c_ms"] = row["b"]["median_ms"] - row["c"]["median_ms"]
    row["c_minus_a_ms"] = row["c"]["median_ms"] - row["a"]["median_ms"]
    row["larger_spread_ms"] = max(row["b"]["spread_ms"], row["c"]["spread_ms"])
    row["within_spread"] = bool(row["b_minus_c_ms"] <= row["larger_spread_ms"])
    results.append(row)
    print(f"S={S:3d}  " + "  ".join(f"{p}: {row[p]['median_ms']:8.3f} ms (spread {row[p]['spread_ms']:6.3f})" for p in "abc")
          + f"  b - c = {row['b_minus_c_ms']:+.3f} ms against {row['larger_spread_ms']:.3f}: "
          f"{'within' if row['within_spread'] else 'beyond'} the spread;  c - a = {row['c_minus_a_ms']:+.3f} ms", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
