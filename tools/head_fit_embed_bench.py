#!/usr/bin/env python3
"""Time the embedding head-fitting step (`frmap_head_fit_embed_step`) against the same step in torch eager with autograd on the same card.

For (B, D, E, C) = (32, 512, 512, 18) - the reference's batch and class count on an ArcFaceNet's pooled features - and
(256, 512, 512, 1000): one step is ``B`` rows as ``rows`` into a cache of 10 000 rows, a dropout mask of p = 0.2 behind the BatchNorm
(a fixed one, the same on both sides: drawing it is not part of either step), AdamW with AMSGrad and label smoothing 0.05 (the
reference's ArcFace settings), at the schedule's values after the warm-up (s = 24 x 0.8 x 0.35, m = 0.45).  The torch side is the
reference's own sequence of calls on the gathered copy ``x[rows]``: ``F.linear`` -> ``nn.BatchNorm1d`` in training mode -> the mask ->
``F.normalize`` of both -> ``F.linear`` -> ``clamp`` -> ``acos`` -> ``minimum`` -> ``cos`` -> ``where`` on a one-hot ->
``cross_entropy(label_smoothing=)`` -> one ``torch.optim.AdamW`` over the four tensors.  Both sides start from the same parameters and
step on the same fixed rows; the mean loss of a last step is printed for each as a sanity check that neither diverged.

Timing is `tools/head_fit_bench.py`'s: a host clock around a window of ``--steps`` back-to-back steps that ends in a device
synchronise, after warm-up steps at the same shape; the two sides alternate inside ``--repeats`` repeats, and the median and the
spread (min .. max) are reported.  A machine without a GPU is refused: there is no CPU timing.

Prints one JSON line per shape and writes them all to ``--out`` when given.
"""
import math

import head_fit_bench_common as common
import torch
import torch.nn.functional as F

SHAPES = ((32, 512, 512, 18), (256, 512, 512, 1000))
CACHE_ROWS = 10000
HYPER = dict(lr=1e-3, weight_decay=1e-4)
SMOOTHING, DROPOUT = 0.05, 0.2


def bench_shape(B, D, E, C, steps, warmup, repeats, dev):
    from frmap_amd import head_fit as hf
    m_eff, s_eff = hf.margin_schedule(10)
    g = torch.Generator(device=dev).manual_seed(B + D + E + C)
    x = torch.randn((CACHE_ROWS, D), device=dev, generator=g).abs()             # pooled features follow a ReLU
    labels = torch.randint(0, C, (CACHE_ROWS,), device=dev, generator=g, dtype=torch.int32)
    rows = torch.randperm(CACHE_ROWS, device=dev, generator=g)[:B].to(torch.int32)
    keep = (torch.rand((B, E), device=dev, generator=g) >= DROPOUT).to(torch.uint8)
    idx, y = rows.long(), labels[rows.long()].long()
    head = hf.EmbedHead(D, E, C, dev, amsgrad=True, generator=torch.Generator().manual_seed(1))
    lin = torch.nn.Linear(D, E, bias=False, device=dev)
    bn = torch.nn.BatchNorm1d(E, eps=head.bn_eps, momentum=head.bn_momentum, device=dev).train()
    with torch.no_grad():
        lin.weight.copy_(head.w1)
    centres = torch.nn.Parameter(head.wc.clone())
    opt = torch.optim.AdamW([lin.weight, bn.weight, bn.bias, centres], amsgrad=True, **HYPER)
    cap = torch.tensor(math.pi - 1e-4, device=dev)
    mask = keep.float() / (1.0 - DROPOUT)
    last = {}

    def ours_step():
        head.step(x, labels, rows, keep, s=s_eff, m=m_eff, label_smoothing=SMOOTHING, dropout=DROPOUT, decoupled=True, **HYPER)

    def torch_step():
        opt.zero_grad(set_to_none=True)
        emb = bn(lin(x[idx])) * mask
        cs = torch.clamp(F.linear(F.normalize(emb, p=2, dim=1, eps=1e-12), F.normalize(centres, p=2, dim=1, eps=1e-12)), min=-1.0 + 1e-7,
                         max=1.0 - 1e-7)
        phi = torch.cos(torch.minimum(cap, torch.acos(cs) + m_eff))
        one_hot = torch.zeros_like(cs)
        one_hot.scatter_(1, y.view(-1, 1), 1)
        loss = F.cross_entropy(torch.where(one_hot.bool(), phi, cs) * s_eff, y, label_smoothing=SMOOTHING)
        loss.backward()
        opt.step()
        last["torch"] = loss

    out = {"B": B, "D": D, "E": E, "C": C, "cache_rows": CACHE_ROWS, "steps_per_window": steps, "repeats": repeats, "s": s_eff, "m": m_eff}
    common.time_steps(out, ours_step, torch_step, steps, warmup, repeats)
    head.new_epoch()
    ours_step()
    out["loss_ours_last_step"] = head.epoch_figures()["loss"]
    out["loss_torch_last_step"] = float(last["torch"].detach())
    out["speedup_step"] = out["torch_us"]["median"] / out["ours_us"]["median"]
    return out


def lines_of(args, shapes, dev):
    for B, D, E, C in shapes:
        yield bench_shape(B, D, E, C, args.steps, args.warmup, args.repeats, dev)


if __name__ == "__main__":
    common.main("head_fit_embed_bench", __doc__, SHAPES, lines_of, steps=300)
