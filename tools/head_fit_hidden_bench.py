#!/usr/bin/env python3
"""Time the hidden-layer head-fitting step (`frmap_head_fit_hidden_step`) against the same step in torch eager on the same card.

For (B, D, Hd, C) = (32, 128, 512, 18) - the baseline's own fc1 / fc2 -, (32, 512, 256, 18) - a projection of ResNet features - and
(256, 512, 256, 1000): one step is a mini-batch as ``rows`` into a cache of 10 000 rows, fresh dropout masks on the input (p = 0.1)
and on the hidden layer (p = 0.5), Adam with coupled weight decay.  The torch side is ``Dropout -> Linear -> ReLU -> Dropout ->
Linear`` + ``F.cross_entropy`` + one ``torch.optim.Adam`` over the four parameters on a gathered copy ``x[rows]``.  Both sides
start from the same weights; the loss of the last timed step is printed for each as a sanity check (different dropout masks: they
agree to a few percent, not to the bit).

Timing is `tools/head_fit_bench.py`'s: a host clock around a window of ``--steps`` back-to-back steps that ends in a device
synchronise, after warm-up steps at the same shape; the two sides alternate inside ``--repeats`` repeats, and the median and the
spread (min .. max) are reported.  ``--only ours`` runs our side alone (``--steps`` steps per shape after the warm-up, nothing
timed) and ``--shape I`` one shape of the table: the run a kernel trace is taken of.  A machine without a GPU is refused: there
is no CPU timing.

Prints one JSON line per shape and writes them all to ``--out`` when given.
"""
import head_fit_bench_common as common
import torch
import torch.nn.functional as F

SHAPES = ((32, 128, 512, 18), (32, 512, 256, 18), (256, 512, 256, 1000))
CACHE_ROWS = 10000
HYPER = dict(lr=1e-3, weight_decay=1e-4)
DROPOUT1, DROPOUT2 = 0.1, 0.5


def bench_shape(B, D, Hd, C, steps, warmup, repeats, dev, only_ours=False):
    from frmap_amd import head_fit as hf
    g = torch.Generator(device=dev).manual_seed(B + Hd + C)
    x = torch.randn((CACHE_ROWS, D), device=dev, generator=g)
    labels = torch.randint(0, C, (CACHE_ROWS,), device=dev, generator=g, dtype=torch.int32)
    labels64 = labels.long()
    head = hf.HiddenHead(D, Hd, C, dev, generator=torch.Generator().manual_seed(1))
    net = torch.nn.Sequential(torch.nn.Dropout(DROPOUT1), torch.nn.Linear(D, Hd), torch.nn.ReLU(), torch.nn.Dropout(DROPOUT2),
                              torch.nn.Linear(Hd, C)).to(dev)
    with torch.no_grad():
        net[1].weight.copy_(head.w1)
        net[1].bias.copy_(head.b1)
        net[4].weight.copy_(head.w2)
        net[4].bias.copy_(head.b2)
    opt = torch.optim.Adam(net.parameters(), **HYPER)
    last = {}

    def ours_step(rows):
        keep1 = (torch.rand((rows.shape[0], D), device=dev, generator=g) >= DROPOUT1).to(torch.uint8)
        keep2 = (torch.rand((rows.shape[0], Hd), device=dev, generator=g) >= DROPOUT2).to(torch.uint8)
        head.step(x, labels, rows, keep1, keep2, dropout1=DROPOUT1, dropout2=DROPOUT2, **HYPER)

    def torch_step(rows):
        opt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(net(x[rows.long()]), labels64[rows.long()])
        loss.backward()
        opt.step()
        last["torch"] = loss

    rows0 = torch.randperm(CACHE_ROWS, device=dev, generator=g)[:B].to(torch.int32)
    out = {"B": B, "D": D, "Hd": Hd, "C": C, "cache_rows": CACHE_ROWS, "steps_per_window": steps, "repeats": repeats}
    if not common.time_steps(out, lambda: ours_step(rows0), lambda: torch_step(rows0), steps, warmup, repeats, only_ours):
        return out
    head.new_epoch().step(x, labels, rows0, None, None, **HYPER)
    out["loss_ours_last_step"] = head.epoch_figures()["loss"]
    out["loss_torch_last_step"] = float(last["torch"].detach())
    out["speedup_step"] = out["torch_us"]["median"] / out["ours_us"]["median"]
    return out


def lines_of(args, shapes, dev):
    for B, D, Hd, C in shapes:
        yield bench_shape(B, D, Hd, C, args.steps, args.warmup, args.repeats, dev, args.only == "ours")


if __name__ == "__main__":
    common.main("head_fit_hidden_bench", __doc__, SHAPES, lines_of, steps=500, more=common.only_option)
