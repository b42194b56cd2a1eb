#!/usr/bin/env python3
"""Time the grouped head-fitting step (`frmap_head_fit_group_step`) against H single steps (`frmap_head_fit_step`) on one card.

For H in {1, 5, 16, 64} at (B, D, C) = (32, 512, 18) and (256, 512, 1000):
  * grouped: one `HeadGroup.step` - H heads, their rows ``[H, B]`` and masks ``[H, B, D]`` already on the device;
  * single: H `LinearHead.step` calls over the same rows and masks, one after the other on the same stream.
Both sides read the same 10 000-row cache, resident on the device, and the same pre-drawn masks, so that what is timed is the steps.
Then a 5-fold x 15-epoch `cross_validate` on the 10 000 cached rows against five `fit_head`-style loops (a `LinearHead` per fold:
a device permutation an epoch, a fresh mask a step, the validation rows through `logits` + `ClassificationTally`).

Timing: a host clock around back-to-back steps that ends in one device synchronise, after warm-up steps at the same shape; the two
sides alternate inside each repeat, ``--repeats`` windows each, and the median and the spread (min .. max) are reported.  A machine
without a GPU is refused: there is no CPU timing.

Prints one JSON line per (shape, H) and one for the cross-validation, and writes them all to ``--out`` when given.
"""
import head_fit_bench_common as common
import torch

SHAPES = ((32, 512, 18), (256, 512, 1000))
HEADS = (1, 5, 16, 64)
CACHE_ROWS = 10000
HYPER = dict(lr=1e-3, weight_decay=1e-4)
DROPOUT = 0.1


def bench_step(H, B, D, C, x, labels, steps, warmup, repeats, dev):
    from frmap_amd import head_fit as hf
    g = torch.Generator(device=dev).manual_seed(H * 1000 + B)
    rows = torch.stack([torch.randperm(CACHE_ROWS, device=dev, generator=g)[:B] for _ in range(H)]).to(torch.int32).contiguous()
    keep = (torch.rand((H, B, D), device=dev, generator=g) >= DROPOUT).to(torch.uint8)
    group = hf.HeadGroup(H, D, C, dev, generator=torch.Generator().manual_seed(1))
    heads = [hf.LinearHead(D, C, dev, generator=torch.Generator().manual_seed(1 + h)) for h in range(H)]
    row_h, keep_h = [rows[h].contiguous() for h in range(H)], [keep[h].contiguous() for h in range(H)]

    def grouped():
        group.step(x, labels, rows, keep, dropout=DROPOUT, **HYPER)

    def singles():
        for h in range(H):
            heads[h].step(x, labels, row_h[h], keep_h[h], dropout=DROPOUT, **HYPER)

    per = common.alternate({"grouped": grouped, "singles": singles}, {"grouped": steps, "singles": max(1, steps // H)}, repeats, warmup)
    out = {"what": "step", "H": H, "B": B, "D": D, "C": C, "steps_per_window": steps, "repeats": repeats,
           "grouped_us": common.record(per["grouped"]), "singles_us": common.record(per["singles"])}
    out["speedup"] = out["singles_us"]["median"] / out["grouped_us"]["median"]
    # beyond the run-to-run spread of the two sides: the slowest grouped window still beats the fastest window of H single steps
    out["beyond_spread"] = out["grouped_us"]["max"] < out["singles_us"]["min"]
    return out


def bench_cv(x, labels, C, repeats, dev, folds=5, epochs=15, B=32):
    from frmap_amd import evaluate, head_fit as hf
    D = int(x.shape[1])

    def grouped():
        hf.cross_validate(x, labels, n_folds=folds, epochs=epochs, batch_size=B, dropout=DROPOUT, num_classes=C,
                          generator=torch.Generator().manual_seed(3), **HYPER)

    def loops():
        g = torch.Generator(device=dev).manual_seed(3)
        for tr, va in hf.kfold_rows(CACHE_ROWS, folds, 42):
            tr, va = torch.from_numpy(tr).to(dev), torch.from_numpy(va).to(dev).long()
            head = hf.LinearHead(D, C, dev, generator=torch.Generator().manual_seed(3))
            vx, vy = x[va].contiguous(), labels[va].contiguous()
            for _ in range(epochs):
                perm = tr[torch.randperm(tr.shape[0], device=dev, generator=g)]
                head.new_epoch()
                for lo in range(0, perm.shape[0], B):
                    r = perm[lo: lo + B]
                    keep = (torch.rand((r.shape[0], D), device=dev, generator=g) >= DROPOUT).to(torch.uint8)
                    head.step(x, labels, r, keep, dropout=DROPOUT, **HYPER)
                head.epoch_figures()
                tally = evaluate.ClassificationTally(C, device=dev)
                tally.update(head.logits(vx), vy)
                tally.metrics()

    per = common.alternate({"grouped": grouped, "loops": loops}, 1, repeats, warmup=1)
    out = {"what": "cross_validate", "folds": folds, "epochs": epochs, "B": B, "D": D, "C": C, "cache_rows": CACHE_ROWS, "repeats": repeats,
           "grouped_ms": common.record(per["grouped"], 1e3), "loops_ms": common.record(per["loops"], 1e3)}
    out["speedup"] = out["loops_ms"]["median"] / out["grouped_ms"]["median"]
    out["beyond_spread"] = out["grouped_ms"]["max"] < out["loops_ms"]["min"]
    return out


def lines_of(args, shapes, dev):
    for B, D, C in shapes:
        g = torch.Generator(device=dev).manual_seed(B + C)
        x = torch.randn((CACHE_ROWS, D), device=dev, generator=g)
        labels = torch.randint(0, C, (CACHE_ROWS,), device=dev, generator=g, dtype=torch.int32)
        for H in HEADS:
            yield bench_step(H, B, D, C, x, labels, args.steps, args.warmup, args.repeats, dev)
        if not args.no_cv and (B, D, C) == SHAPES[0]:
            yield bench_cv(x, labels, C, max(2, args.repeats // 2), dev)


def _no_cv(ap):
    ap.add_argument("--no-cv", action="store_true", help="skip the cross-validation timing")


if __name__ == "__main__":
    common.main("head_fit_group_bench", __doc__, SHAPES, lines_of, steps=200, more=_no_cv,
                steps_help="grouped steps per timed window (the single side runs steps / H rounds of H)")
