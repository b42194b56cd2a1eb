#!/usr/bin/env python3
"""Time the pair head-fitting step (`frmap_head_fit_pair_step`) against the same step in torch eager with autograd on the same card.

For (P, D, E) = (32, 512, 256) - the reference's batch on a SiameseNet's fc.8 -, (256, 512, 256) and (1024, 512, 128): one step is
``P`` pairs as ``left`` / ``right`` into a cache of 10 000 rows, no dropout mask (the reference has none in front of fc.8), Adam with
coupled weight decay.  The torch side is ``F.linear`` on the gathered copy ``x[left ++ right]`` -> ``F.normalize`` ->
``F.pairwise_distance`` -> the clamp and the two weighted terms (margin 2.0, 0.8 / 1.2) -> one ``torch.optim.Adam`` over the two
parameters.  Both sides start from the same weights and step on the same fixed pair lists; the mean loss of a last step is printed
for each as a sanity check that neither diverged (after thousands of steps on one fixed list both are near zero, not equal).

Timing is `tools/head_fit_bench.py`'s: a host clock around a window of ``--steps`` back-to-back steps that ends in a device
synchronise, after warm-up steps at the same shape; the two sides alternate inside ``--repeats`` repeats, and the median and the
spread (min .. max) are reported.  ``--only ours`` runs our side alone (``--steps`` steps per shape after the warm-up, nothing
timed) and ``--shape I`` one shape of the table: the run a kernel trace is taken of, whose per-kernel totals are the split of the
step (forward, gate, pair, update).  A machine without a GPU is refused: there is no CPU timing.

Prints one JSON line per shape and writes them all to ``--out`` when given.
"""
import head_fit_bench_common as common
import torch
import torch.nn.functional as F

SHAPES = ((32, 512, 256), (256, 512, 256), (1024, 512, 128))
CACHE_ROWS = 10000
HYPER = dict(lr=1e-3, weight_decay=1e-4)
MARGIN, W_SAME, W_DIFF = 2.0, 0.8, 1.2


def bench_shape(P, D, E, steps, warmup, repeats, dev, only_ours=False):
    from frmap_amd import head_fit as hf
    g = torch.Generator(device=dev).manual_seed(P + D + E)
    x = torch.randn((CACHE_ROWS, D), device=dev, generator=g)
    labels = torch.randint(0, 100, (CACHE_ROWS,), device=dev, generator=g, dtype=torch.int32)
    left, right, differ = hf.draw_pairs(labels, P, g)
    idx = torch.cat([left, right]).long()
    y = differ.float()
    head = hf.PairHead(D, E, dev, generator=torch.Generator().manual_seed(1))
    lin = torch.nn.Linear(D, E).to(dev)
    with torch.no_grad():
        lin.weight.copy_(head.weight)
        lin.bias.copy_(head.bias)
    opt = torch.optim.Adam(lin.parameters(), **HYPER)
    last = {}

    def ours_step():
        head.step(x, left, right, differ, margin=MARGIN, w_same=W_SAME, w_diff=W_DIFF, **HYPER)

    def torch_step():
        opt.zero_grad(set_to_none=True)
        u = F.normalize(lin(x[idx]), p=2, dim=1)
        d = torch.clamp(F.pairwise_distance(u[:P], u[P:]), min=1e-8)
        loss = ((1 - y) * d.pow(2) * W_SAME + y * torch.clamp(MARGIN - d, min=0.0).pow(2) * W_DIFF).mean()
        loss.backward()
        opt.step()
        last["torch"] = loss

    out = {"P": P, "D": D, "E": E, "cache_rows": CACHE_ROWS, "steps_per_window": steps, "repeats": repeats}
    if not common.time_steps(out, ours_step, torch_step, steps, warmup, repeats, only_ours):
        return out
    head.new_epoch()
    ours_step()
    out["loss_ours_last_step"] = head.epoch_figures()["loss"]
    out["loss_torch_last_step"] = float(last["torch"].detach())
    out["speedup_step"] = out["torch_us"]["median"] / out["ours_us"]["median"]
    return out


def lines_of(args, shapes, dev):
    for P, D, E in shapes:
        yield bench_shape(P, D, E, args.steps, args.warmup, args.repeats, dev, args.only == "ours")


if __name__ == "__main__":
    common.main("head_fit_pair_bench", __doc__, SHAPES, lines_of, steps=500, more=common.only_option)
