#!/usr/bin/env python3
"""From one frame and a detector's boxes to matched names, three ways, on one device in one process.

Set-up: one 1280x720 BGR frame on the host (as a capture delivers it), N in {1, 4, 16, 64} boxes with sides of 60 .. 400 px,
'cnn' in bf16 with get_embedding's 0.5 / 0.5 input normalisation, a 36-entry gallery.
  a     the reference's loop (src/app.py:224-241): `get_embedding` + `compare_faces` per box.  It matches `model(x)` (36 logits)
        against a 36 x 36 gallery - context, not the bar.
  b     the best batching without the crop kernel: `resize_bilinear_u8` on the list of slices + `normalize_u8` +
        `embed_and_match` (unit-norm 512-d embeddings, 36 x 512 gallery) + one copy of the ids.
  b_u8  b without the fp32 input pass (the uint8 batch goes into `embed_and_match`): separates what (c) gains from the crop
        kernel from what it gains by skipping `normalize_u8`.
  c     `identify_boxes(what="embedding", normalize=True)`: the same embeddings and gallery as b.
Regimes: "redrawn" - every call sees box sizes it has not seen (live video: a box changes by a pixel or two per frame); the
per-size table cache of `resize.bilinear_coeffs` is emptied before each timed call of a / b (outside the timed span), so all
paths see the same boxes.  "fixed" - the same boxes every call, tables cached.
Timing: host clock around one call ending in a device synchronise; every shape warmed up first; the paths alternate inside each
repeat; per (regime, N, path) the median over the repeats of the repeat's mean call time, and the spread (max - min) of those."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import frmap_amd
from frmap_amd import frames, matching, ops, resize, synth

ap = argparse.ArgumentParser()
ap.add_argument("--ns", type=int, nargs="+", default=[1, 4, 16, 64])
ap.add_argument("--paths", nargs="+", default=["a", "b", "b_u8", "c"])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=10, help="timed calls per repeat (a: a fifth of it)")
ap.add_argument("--out", default=None, help="write the results as JSON here")
args = ap.parse_args()
assert torch.cuda.is_available(), "frame_bench needs a GPU"
DEV, H, W, SIZE, NORM = "cuda", 720, 1280, (160, 160), ((.5, .5, .5), (.5, .5, .5))

rng = np.random.default_rng(11)
frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
m = frmap_amd.get_model("cnn", 36)
m.load_state_dict(synth.calibrated_state_dict("cnn", synth.shapes_of(m), 1002))
m = m.to(DEV).eval().set_compute_dtype(torch.bfloat16).set_input_normalization(*NORM)
names = [f"id{i}" for i in range(36)]
gal512 = frmap_amd.Gallery(names, synth.unit_rows(3001, 36, 512), DEV)
refs36 = [{"name": names[i], "embedding": r.reshape(1, -1)} for i, r in enumerate(synth.unit_rows(3002, 36, 36))]


def draw(n):
    w, h = rng.uniform(60, 400, n), rng.uniform(60, 400, n)
    x1, y1 = rng.uniform(0, W - w), rng.uniform(0, H - h)
    return np.stack([x1, y1, x1 + w, y1 + h], 1), np.full(n, 0.99)


def _names(ids):
    return [names[i] if i >= 0 else "Unknown" for i in ids.cpu().tolist()]


def path_a(boxes, probs):
    rois, _ = frames.clip_boxes(boxes, probs, frame.shape)
    return [matching.compare_faces(matching.get_embedding(frame[y1:y2, x1:x2], m), refs36, 1.0)[0] for x1, y1, x2, y2 in rois.tolist()]


def _b_crops(boxes, probs):
    rois, _ = frames.clip_boxes(boxes, probs, frame.shape)
    return resize.resize_bilinear_u8([np.ascontiguousarray(frame[y1:y2, x1:x2, ::-1]) for x1, y1, x2, y2 in rois.tolist()], SIZE, DEV)


def path_b(boxes, probs):
    x = ops.normalize_u8(_b_crops(boxes, probs), *NORM)[0]
    with torch.no_grad():
        return _names(matching.embed_and_match(m, x, gal512, 1.0, normalize=True)[0])


def path_b_u8(boxes, probs):
    with torch.no_grad():
        return _names(matching.embed_and_match(m, _b_crops(boxes, probs), gal512, 1.0, normalize=True)[0])


def path_c(boxes, probs):
    return [r[0] for r in matching.identify_boxes(m, frame, boxes, gal512, 1.0, probs=probs, what="embedding", normalize=True)[0]]


PATHS = {"a": path_a, "b": path_b, "b_u8": path_b_u8, "c": path_c}
results = []
for n in args.ns:
    fixed = draw(n)
    for regime in ("redrawn", "fixed"):
        for p in args.paths:                                   # warm-up: kernels, plans, allocator pools for this N
            for _ in range(3):
                PATHS[p](*(draw(n) if regime == "redrawn" else fixed))
        torch.cuda.synchronize()
        per_rep = {p: [] for p in args.paths}
        for rep in range(args.reps):
            sets = [draw(n) if regime == "redrawn" else fixed for _ in range(args.iters)]
            order = args.paths[rep % len(args.paths):] + args.paths[:rep % len(args.paths)]
            for p in order:
                total, calls = 0.0, sets[: max(2, args.iters // 5)] if p == "a" else sets
                for boxes, probs in calls:
                    if regime == "redrawn":
                        resize.bilinear_coeffs.cache_clear()   # these sizes have not been seen before
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    PATHS[p](boxes, probs)
                    torch.cuda.synchronize()
                    total += time.perf_counter() - t0
                per_rep[p].append(1e3 * total / len(calls))
        row = {"N": n, "regime": regime}
        for p in args.paths:
            row[p] = {"median_ms": statistics.median(per_rep[p]), "spread_ms": max(per_rep[p]) - min(per_rep[p])}
        results.append(row)
        print(f"N={n:3d} {regime:8s} " + "  ".join(f"{p}: {row[p]['median_ms']:8.3f} ms (spread {row[p]['spread_ms']:6.3f})" for p in args.paths),
              flush=True)
        if "b" in row and "c" in row:
            gap, sp = row["b"]["median_ms"] - row["c"]["median_ms"], max(row["b"]["spread_ms"], row["c"]["spread_ms"])
            verdict = gap > sp if regime == "redrawn" else gap > -sp
            print(f"      b - c = {gap:+.3f} ms against a spread of {sp:.3f} ms: condition {'met' if verdict else 'NOT met'}", flush=True)
            row["b_minus_c_ms"], row["condition_met"] = gap, bool(verdict)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
