#!/usr/bin/env python3
"""What the one-vs-rest AUCs cost on one device in one process: the score store and the pair count (`ops.ovr_append`,
`ops.ovr_rank_counts`) against what `evaluate.evaluate_model` does today and sklearn on the host.

Per batch: B = 1024 rows of C in {36, 1000, 10 000} logits (`synth.randn * 3`, the target raised by 2), resident on the device.
  append    `softmax_argmax` with probabilities + one `ovr_append` into a resident store of 8 batches (`first` rotates over it);
            nothing leaves the device
  today     `softmax_argmax` with probabilities, then the device-to-host copies `evaluate_model` makes per batch: the [B, C]
            probabilities, the [B, C] logits (for the loss) and the [B] predictions, into pageable host memory as `.cpu()` does
At the end: the count at (N, C) in {(1764, 36), (100 000, 36), (100 000, 10 000)} on a store of probability rows (uniform
draws divided by their row sums, made on the device, every class present in the labels).
  count     one `ovr_rank_counts` call (the zeroing kernel and the count); N^2 / time is the pair rate
  finish    host clock around `OvrScores.metrics()`: the count, the one copy of labels and counts, `ovr_metrics` in float64
  sklearn   host clock around `roc_auc_score(multi_class='ovr')` + `average_precision_score` on the same scores, copied to the
            host first (not timed).  Where `--sklearn-budget` seconds would be exceeded (estimated from the first classes), the two
            binary calls are timed on `--sklearn-classes` columns and the figure is that time x C / columns: reported as
            "extrapolated", never as measured.  The device's figures are reported beside sklearn's (worst difference).
Timing: HIP events around `--iters` back-to-back calls of one path (the copies of `today` synchronise by themselves), every shape
warmed up first, the two per-batch paths alternating inside each repeat; per path the median over `--reps` repeats of the
repeat's mean time per call, and the spread (max - min) of those.  The counts of the timed store are checked for repeatability
(two calls, identical words).  No pass / fail gate on time."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from frmap_amd import evaluate, ops, synth

ap = argparse.ArgumentParser()
ap.add_argument("--classes", type=int, nargs="+", default=[36, 1000, 10000])
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--counts", type=str, nargs="+", default=["1764x36", "100000x36", "100000x10000"], help="N x C of the final count")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=50, help="timed calls per repeat of the per-batch paths")
ap.add_argument("--count-iters", type=int, default=3, help="timed calls per repeat of the count")
ap.add_argument("--sklearn-budget", type=float, default=60.0)
ap.add_argument("--sklearn-classes", type=int, default=8)
ap.add_argument("--out", default=None, help="write the results as JSON here")
args = ap.parse_args()
assert torch.cuda.is_available(), "ovr_bench needs a GPU"
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


def summary(samples):
    return {"median_ms": statistics.median(samples), "spread_ms": max(samples) - min(samples)}


results = {"per_batch": [], "count": []}
for C in args.classes:
    y = torch.from_numpy(np.random.default_rng([41, C]).integers(0, C, B).astype(np.int32))
    z = synth.randn(4100 + C, (B, C), "ovr-bench") * 3
    z[torch.arange(B), y.long()] += 2.0
    zd, yd = z.to(DEV), y.to(DEV)
    store = torch.empty((C, 8 * B), dtype=torch.float32, device=DEV)
    labels = torch.empty((8 * B,), dtype=torch.int32, device=DEV)
    turn = [0]

    def append():
        probs, _ = ops.softmax_argmax(zd)
        ops.ovr_append(probs, yd, store, labels, (turn[0] % 8) * B)
        turn[0] += 1

    def today():
        probs, pred = ops.softmax_argmax(zd)
        return probs.cpu(), zd.cpu(), pred.cpu()

    run = {"append": append, "today": today}
    for _ in range(8):                                          # warm-up: code objects, allocator pools, the host buffers, the whole store
        for fn in run.values():
            fn()
    torch.cuda.synchronize()
    per_rep = {p: [] for p in run}
    for rep in range(args.reps):
        for p in (("append", "today"), ("today", "append"))[rep % 2]:
            per_rep[p].append(timed(run[p], args.iters))
    probs, _ = ops.softmax_argmax(zd)
    assert torch.equal(store[:, :B].t().contiguous().view(torch.int32), probs.view(torch.int32)), "the store is not the transpose of the probabilities"
    row = {"B": B, "C": C, "pcie_bytes_today": 2 * B * C * 4 + B * 4}
    for p in run:
        row[p] = summary(per_rep[p])
    row["today_over_append"] = row["today"]["median_ms"] / row["append"]["median_ms"]
    results["per_batch"].append(row)
    print(f"B={B} C={C:6d}  " + "  ".join(f"{p}: {1e3 * row[p]['median_ms']:9.1f} us (spread {1e3 * row[p]['spread_ms']:7.1f})" for p in run)
          + f"  today / append = {row['today_over_append']:.1f}x  ({row['pcie_bytes_today'] / 1e6:.1f} MB over PCIe per batch today)", flush=True)
    del store, labels, zd

for spec in args.counts:
    N, C = (int(v) for v in spec.split("x"))
    acc = evaluate.OvrScores(C, N, device=DEV)
    acc.store.uniform_()
    acc.store.div_(acc.store.sum(dim=0, keepdim=True))          # probability rows, made in place: no second copy of the scores
    y = torch.from_numpy(np.random.default_rng([43, N, C]).permutation(np.arange(N) % C).astype(np.int32))
    acc.labels.copy_(y.to(DEV))
    acc.rows = N
    first = ops.ovr_rank_counts(acc.store, acc.labels, N)       # (warm-up as well)
    again = ops.ovr_rank_counts(acc.store, acc.labels, N)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two counts of one store differ"
    del first, again
    count = [timed(lambda: ops.ovr_rank_counts(acc.store, acc.labels, N), args.count_iters) for _ in range(args.reps)]
    finish = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = acc.metrics()
        finish.append(1e3 * (time.perf_counter() - t0))
    row = {"N": N, "C": C, "count": summary(count), "finish_host_ms": summary(finish), "store_bytes": 4 * N * C}
    row["pairs_per_s"] = N * N / (1e-3 * row["count"]["median_ms"])
    # sklearn on the host, on the same scores
    from sklearn.metrics import average_precision_score, roc_auc_score
    yh = y.numpy()
    k = min(C, args.sklearn_classes)
    cols = acc.store[:k].cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    some = [(roc_auc_score(yh == c, cols[c]), average_precision_score(yh == c, cols[c])) for c in range(k)]
    per_class_s = (time.perf_counter() - t0) / k
    # the device's figures beside sklearn's, class by class (reported, not gated: the tests hold the 1e-12 bar at their sizes)
    row["max_difference_per_class"] = max(max(abs(m["per_class"][str(c)]["roc_auc"] - some[c][0]),
                                              abs(m["per_class"][str(c)]["average_precision"] - some[c][1])) for c in range(k))
    if per_class_s * C <= args.sklearn_budget:
        scores = acc.store[:, :N].t().contiguous().cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        roc = roc_auc_score(yh, scores, multi_class="ovr")
        pr = average_precision_score(yh, scores)
        row["sklearn_s"], row["sklearn"] = time.perf_counter() - t0, "measured"
        row["max_difference"] = max(abs(roc - m["roc_auc"]), abs(pr - m["pr_auc"]))
        del scores
    else:
        row["sklearn_s"], row["sklearn"] = per_class_s * C, f"extrapolated from {k} classes ({per_class_s:.3f} s each) x {C} / {k}"
    results["count"].append(row)
    print(f"N={N:7d} C={C:6d}  count: {row['count']['median_ms']:9.3f} ms (spread {row['count']['spread_ms']:.3f})  "
          f"{row['pairs_per_s'] / 1e9:8.1f} G pairs/s  finish (count + copy + float64 on the host): {row['finish_host_ms']['median_ms']:9.1f} ms  "
          f"sklearn: {row['sklearn_s']:9.2f} s ({row['sklearn']})  store {row['store_bytes'] / 1e6:.0f} MB  "
          f"worst difference from sklearn: {max(row['max_difference_per_class'], row.get('max_difference', 0.0)):.2g}", flush=True)
    del acc, cols
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
