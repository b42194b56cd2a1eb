#!/usr/bin/env python3
"""What the accumulate step of an evaluation costs per batch, on one device in one process: `ops.classify_tally` against what
`evaluate.evaluate_model` does today.

B = 1024 rows of C in {36, 1000, 10 000} logits (`synth.randn * 3`, the target raised by 2), resident on the device.
  tally     one `classify_tally` launch into a resident state (the confusion matrix kept up to C = 2048, as
            `ClassificationTally` decides); nothing leaves the device
  today     `softmax_argmax` with probabilities, then the device-to-host copies `evaluate_model` makes per batch: the [B, C]
            probabilities, the [B, C] logits (for the loss) and the [B] predictions, into pageable host memory as `.cpu()` does
  argmax    `softmax_argmax(want_probs=False)` alone: the least any accumulate step could launch
Timing: HIP events around `--iters` back-to-back calls of one path (the copies of `today` synchronise by themselves), every shape
warmed up first, the paths alternating inside each repeat; per path the median over `--reps` repeats of the repeat's mean time
per call, and the spread (max - min) of those.  Reported per C: the three medians with their spreads, today / tally and
tally / argmax, and the bytes `today` moves over PCIe per batch.  The state of the timed tally is checked against a fresh one
(iters x the counts of one call) after the run.  No pass / fail gate on time."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from frmap_amd import ops, synth

ap = argparse.ArgumentParser()
ap.add_argument("--classes", type=int, nargs="+", default=[36, 1000, 10000])
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=50, help="timed calls per repeat")
ap.add_argument("--out", default=None, help="write the results as JSON here")
args = ap.parse_args()
assert torch.cuda.is_available(), "tally_bench needs a GPU"
DEV, B = "cuda", args.batch


def timed(fn, iters):
    """Milliseconds per call of `iters` back-to-back calls, by device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


results = []
for C in args.classes:
    y = torch.from_numpy(np.random.default_rng([41, C]).integers(0, C, B).astype(np.int32))
    z = synth.randn(4100 + C, (B, C), "tally-bench") * 3
    z[torch.arange(B), y.long()] += 2.0
    zd, yd = z.to(DEV), y.to(DEV)
    keep = C <= 2048
    state = torch.zeros((ops.classify_tally_words(C, 6, 10, keep),), dtype=torch.int64, device=DEV)

    def tally():
        ops.classify_tally(zd, yd, state, 6, 10, keep)

    def today():
        probs, pred = ops.softmax_argmax(zd)
        return probs.cpu(), zd.cpu(), pred.cpu()

    def argmax():
        ops.softmax_argmax(zd, want_probs=False)

    run = {"tally": tally, "today": today, "argmax": argmax}
    for _ in range(3):                                          # warm-up: code objects, allocator pools, the host buffers
        for fn in run.values():
            fn()
    torch.cuda.synchronize()
    state.zero_()
    calls = 0
    per_rep = {p: [] for p in run}
    for rep in range(args.reps):
        for p in (("tally", "today", "argmax"), ("today", "argmax", "tally"), ("argmax", "tally", "today"))[rep % 3]:
            per_rep[p].append(timed(run[p], args.iters))
            calls += args.iters if p == "tally" else 0
    one = ops.classify_tally(zd, yd, None, 6, 10, keep)
    torch.cuda.synchronize()
    assert torch.equal(state, one * calls), "the timed tally is not `calls` times the tally of one batch"
    row = {"B": B, "C": C, "confusion_kept": keep, "pcie_bytes_today": 2 * B * C * 4 + B * 4}
    for p in run:
        row[p] = {"median_ms": statistics.median(per_rep[p]), "spread_ms": max(per_rep[p]) - min(per_rep[p])}
    row["today_over_tally"] = row["today"]["median_ms"] / row["tally"]["median_ms"]
    row["tally_over_argmax"] = row["tally"]["median_ms"] / row["argmax"]["median_ms"]
    results.append(row)
    print(f"B={B} C={C:6d}  " + "  ".join(f"{p}: {1e3 * row[p]['median_ms']:9.1f} us (spread {1e3 * row[p]['spread_ms']:7.1f})" for p in run)
          + f"  today / tally = {row['today_over_tally']:.1f}x  tally / argmax = {row['tally_over_argmax']:.2f}x  "
          f"({row['pcie_bytes_today'] / 1e6:.1f} MB over PCIe per batch today)", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
