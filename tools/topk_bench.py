#!/usr/bin/env python3
"""Micro-benchmark of the exact top-k search against the top-1 match on prepared galleries (HIP events, one process):
1024 probes x {10 000, 100 000} rows x 512, match_top1_packed vs match_topk_packed for k in {1, 5, 16, 64}, entry mode on random
rows and identity mode on a gallery of 5 near-duplicate enrolments per identity (shuffled)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from frmap_amd import ops
def t(fn, n=20):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
torch.manual_seed(0)
B, D = 1024, 512
for G in (10000, 100000):
    e = torch.nn.functional.normalize(torch.randn(B, D, device="cuda"), dim=1)
    g = torch.nn.functional.normalize(torch.randn(G, D, device="cuda"), dim=1)
    # identity gallery: G / 5 identities x 5 enrolments at separations 1e-6 .. 1e-3, shuffled; probes near enrolled identities
    N = G // 5
    base = torch.nn.functional.normalize(torch.randn(N, D, device="cuda"), dim=1)
    seps = (0.0, 1e-6, 1e-5, 1e-4, 1e-3)
    gi = torch.cat([base + s * torch.randn(N, D, device="cuda") for s in seps])
    li = torch.arange(N, device="cuda", dtype=torch.int32).repeat(5)
    perm = torch.randperm(G, device="cuda")
    gi, li = gi[perm].contiguous(), li[perm].contiguous()
    ei = (base[torch.randint(0, N, (B,), device="cuda")] + 1e-4 * torch.randn(B, D, device="cuda")).contiguous()
    prep, prep_i = ops.match_prepare(g), ops.match_prepare(gi)
    t1 = t(lambda: ops.match_top1(e, g, prepared=prep))
    t1i = t(lambda: ops.match_top1(ei, gi, prepared=prep_i))
    print(f"G={G}: match_top1_packed {t1:7.1f} us (random rows), {t1i:7.1f} us (5-enrolment gallery)", flush=True)
    for k in (1, 5, 16, 64):
        te = t(lambda: ops.match_topk(e, g, k, prepared=prep))
        tn = t(lambda: ops.match_topk(ei, gi, k, labels=li, prepared=prep_i))
        print(f"  k={k:2d}: entry {te:7.1f} us ({te / t1:4.2f}x top-1)   identity {tn:7.1f} us ({tn / t1i:4.2f}x top-1)", flush=True)
