#!/usr/bin/env python3
"""Time the head-fitting step (`frmap_head_fit_step`) against the same step in torch eager on the same card.

For (B, D, C) = (32, 512, 18), (256, 512, 1000) and (1024, 512, 10 000):
  * one step: a mini-batch as ``rows`` into a cache of 10 000 rows, a fresh dropout mask, Adam with coupled weight decay;
  * one epoch: the 10 000 cached rows once, ``ceil(10 000 / B)`` steps with a device permutation and per-step masks.
The torch side is ``nn.Linear`` + ``nn.Dropout`` + ``F.cross_entropy`` + ``torch.optim.Adam`` on a gathered copy ``x[rows]``, what
the reference's frozen phase runs per step.  Both sides start from the same weights; the loss of the last timed step is printed for
each as a sanity check (different dropout masks: they agree to a few percent, not to the bit).

Timing: a host clock around a window that ends in a device synchronise, after warm-up steps at the same shape; the two sides
alternate, ``--repeats`` windows each, and the median and the spread (min .. max) are reported.  ``--features``: also time
`head_fit.cache_features` on a synthetic ``cnn`` model (images already on the device), the rate next to which a step's cost stands.
A machine without a GPU is refused: there is no CPU timing.

Prints one JSON line per shape and writes them all to ``--out`` when given.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = ((32, 512, 18), (256, 512, 1000), (1024, 512, 10000))
CACHE_ROWS = 10000
HYPER = dict(lr=1e-3, weight_decay=1e-4)
DROPOUT = 0.1


def _window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def bench_shape(B, D, C, steps, warmup, repeats, dev):
    from frmap_amd import head_fit as hf
    g = torch.Generator(device=dev).manual_seed(B + C)
    x = torch.randn((CACHE_ROWS, D), device=dev, generator=g)
    labels = torch.randint(0, C, (CACHE_ROWS,), device=dev, generator=g, dtype=torch.int32)
    labels64 = labels.long()
    head = hf.LinearHead(D, C, dev, generator=torch.Generator().manual_seed(1))
    lin = torch.nn.Linear(D, C).to(dev)
    with torch.no_grad():
        lin.weight.copy_(head.weight)
        lin.bias.copy_(head.bias)
    drop = torch.nn.Dropout(DROPOUT)
    opt = torch.optim.Adam(lin.parameters(), **HYPER)
    last = {}

    def ours_step(rows):
        keep = (torch.rand((rows.shape[0], D), device=dev, generator=g) >= DROPOUT).to(torch.uint8)
        head.step(x, labels, rows, keep, dropout=DROPOUT, **HYPER)

    def torch_step(rows):
        opt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(lin(drop(x[rows.long()])), labels64[rows.long()])
        loss.backward()
        opt.step()
        last["torch"] = loss

    def epoch(step):
        perm = torch.randperm(CACHE_ROWS, device=dev, generator=g).to(torch.int32)
        for lo in range(0, CACHE_ROWS, B):
            step(perm[lo: lo + B])

    rows0 = torch.randperm(CACHE_ROWS, device=dev, generator=g)[:B].to(torch.int32)
    out = {"B": B, "D": D, "C": C, "cache_rows": CACHE_ROWS, "steps_per_window": steps, "repeats": repeats}
    for name, step in (("ours", ours_step), ("torch", torch_step)):
        for _ in range(warmup):
            step(rows0)
    per = {"ours": [], "torch": [], "ours_epoch": [], "torch_epoch": []}
    for _ in range(repeats):                                   # the two sides alternate inside one process
        per["ours"].append(_window(lambda: ours_step(rows0), steps))
        per["torch"].append(_window(lambda: torch_step(rows0), steps))
    for _ in range(max(2, repeats // 2)):
        per["ours_epoch"].append(_window(lambda: epoch(ours_step), 1))
        per["torch_epoch"].append(_window(lambda: epoch(torch_step), 1))
    for k, v in per.items():
        scale = 1e6 if "epoch" not in k else 1e3
        out[k + ("_us" if "epoch" not in k else "_ms")] = {"median": statistics.median(v) * scale, "min": min(v) * scale, "max": max(v) * scale}
    head.new_epoch().step(x, labels, rows0, None, **HYPER)
    out["loss_ours_last_step"] = head.epoch_figures()["loss"]
    out["loss_torch_last_step"] = float(last["torch"].detach())
    out["steps_per_epoch"] = math.ceil(CACHE_ROWS / B)
    out["speedup_step"] = out["torch_us"]["median"] / out["ours_us"]["median"]
    out["speedup_epoch"] = out["torch_epoch_ms"]["median"] / out["ours_epoch_ms"]["median"]
    return out


def bench_features(dev, batch=256, batches=8, repeats=3):
    """faces/s of `head_fit.cache_features` on a synthetic cnn model, normalised images already on the device."""
    import frmap_amd
    from frmap_amd import head_fit as hf, synth
    from oracle import weights
    model = frmap_amd.get_model("cnn", 36)
    model.load_state_dict(weights.calibrated_state_dict("cnn", synth.shapes_of(model), weights.SEEDS["cnn"][0], n_calib=8))
    model = model.to(dev).eval().set_compute_dtype(torch.float16)
    g = torch.Generator(device=dev).manual_seed(2)
    data = [(torch.randn((batch, 3, 224, 224), device=dev, generator=g), torch.zeros((batch,), dtype=torch.int64)) for _ in range(batches)]
    hf.cache_features(model, "cnn", data, device=dev)           # warm-up: plans, code objects
    times = [_window(lambda: hf.cache_features(model, "cnn", data, device=dev), 1) for _ in range(repeats)]
    return {"what": "cache_features cnn fp16", "batch": batch, "faces": batch * batches, "faces_per_s": batch * batches / statistics.median(times),
            "min_faces_per_s": batch * batches / max(times), "max_faces_per_s": batch * batches / min(times)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=200, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--features", action="store_true", help="also time cache_features on a synthetic cnn model")
    ap.add_argument("--out", default=None, help="write the JSON lines to this file as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("head_fit_bench: no GPU; a timing on the CPU says nothing about the device (not measured)")
    dev = torch.device("cuda:0")
    lines = [bench_shape(B, D, C, args.steps, args.warmup, args.repeats, dev) for B, D, C in SHAPES]
    if args.features:
        lines.append(bench_features(dev))
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
