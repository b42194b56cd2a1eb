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
import math
import statistics

import head_fit_bench_common as common
import torch
import torch.nn.functional as F

SHAPES = ((32, 512, 18), (256, 512, 1000), (1024, 512, 10000))
CACHE_ROWS = 10000
HYPER = dict(lr=1e-3, weight_decay=1e-4)
DROPOUT = 0.1


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
    common.time_steps(out, lambda: ours_step(rows0), lambda: torch_step(rows0), steps, warmup, repeats)
    epochs = common.alternate({"ours_epoch": lambda: epoch(ours_step), "torch_epoch": lambda: epoch(torch_step)}, 1, max(2, repeats // 2))
    for k, v in epochs.items():
        out[k + "_ms"] = common.record(v, 1e3)
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
    times = [common.window(lambda: hf.cache_features(model, "cnn", data, device=dev), 1) for _ in range(repeats)]
    return {"what": "cache_features cnn fp16", "batch": batch, "faces": batch * batches, "faces_per_s": batch * batches / statistics.median(times),
            "min_faces_per_s": batch * batches / max(times), "max_faces_per_s": batch * batches / min(times)}


def lines_of(args, shapes, dev):
    for B, D, C in shapes:
        yield bench_shape(B, D, C, args.steps, args.warmup, args.repeats, dev)
    if args.features:
        yield bench_features(dev)


def _features(ap):
    ap.add_argument("--features", action="store_true", help="also time cache_features on a synthetic cnn model")


if __name__ == "__main__":
    common.main("head_fit_bench", __doc__, SHAPES, lines_of, steps=200, steps_help="steps per timed window", more=_features)
