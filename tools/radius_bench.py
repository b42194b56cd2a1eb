#!/usr/bin/env python3
"""Micro-benchmark of the exact threshold search (frmap_match_radius_packed on a prepared set) beside frmap_match_top1_packed and
frmap_verify_counts_packed at T = 1 on the same inputs (HIP events, one device, one process).  Synthetic clustered identities as
tools/verify_bench.py: unit-norm centres (synth.unit_rows), 8 noisy enrolments each, D = 512.  Shapes: 1024 probes x 10 000 gallery
rows (cross mode), N = 16 384 and N = 32 768 (self mode, N (N - 1) / 2 pairs).  Per shape three thresholds, the 0.01 %, 0.1 % and
1 % quantiles of the pair distances (estimated once with torch on a sample of the counted pairs), so the list holds about that share
of the pairs.  Every call goes straight to its C entry point with buffers allocated once; the list's capacity is the exact total
of a count-only call.  Prints ms, pairs/s, the listed and re-scored share of the pairs and the ratios to the two yardsticks."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from frmap_amd import _lib, ops, synth
def t(fn, n=0):
    """ms per call between two HIP events; n = 0: two passes, the second long enough to fill ~60 ms (5 .. 200 calls)"""
    for _ in range(2): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n or 3): fn()
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / (n or 3)
    return ms if n else t(fn, max(5, min(200, int(60 / max(ms, 1e-3)))))
lib = _lib.load()
st = lambda: torch.cuda.current_stream().cuda_stream


def radius_fn(a, b, prep, thresh, row0, capacity):
    """a launch-only closure over frmap_match_radius_packed (no labels, every pair); returns (pairs, dists, counts, total, rescored)"""
    (P, D), Q, dev = a.shape, b.shape[0], a.device
    counts = torch.empty((P,), dtype=torch.int32, device=dev)
    total, resc = torch.empty((1,), dtype=torch.int64, device=dev), torch.empty((1,), dtype=torch.int64, device=dev)
    pairs = torch.empty((capacity, 2), dtype=torch.int32, device=dev)
    dists = torch.empty((capacity,), dtype=torch.float32, device=dev)
    ws = torch.empty((lib.frmap_match_radius_workspace_bytes(P, Q, D),), dtype=torch.uint8, device=dev)
    args = (a.data_ptr(), 0, P, b.data_ptr(), prep.packed.data_ptr(), prep.stat_w.data_ptr(), 0, Q, D, row0, float(thresh), 0,
            counts.data_ptr(), total.data_ptr(), pairs.data_ptr() if capacity else 0, dists.data_ptr() if capacity else 0, capacity,
            resc.data_ptr(), ws.data_ptr())

    def run():
        _lib.check(lib.frmap_match_radius_packed(*args, st()), "match_radius_packed")
        return pairs, dists, counts, total, resc
    return run


def verify_fn(a, la, b, lb, prep, thresh, row0):
    """frmap_verify_counts_packed at T = 1 (the threshold checked here, once)"""
    (P, D), Q, dev = a.shape, b.shape[0], a.device
    td = ops.verify_thresholds([float(thresh)], dev)
    out = torch.empty((2, 1), dtype=torch.int64, device=dev)
    ws = torch.empty((lib.frmap_verify_workspace_bytes(P, Q, D, 1),), dtype=torch.uint8, device=dev)
    args = (a.data_ptr(), la.data_ptr(), P, b.data_ptr(), prep.packed.data_ptr(), prep.stat_w.data_ptr(), lb.data_ptr(), Q, D, row0,
            td.data_ptr(), 1, out.data_ptr(), 0, ws.data_ptr())

    def run():
        _lib.check(lib.frmap_verify_counts_packed(*args, st()), "verify_counts_packed")
        return out
    return run


def top1_fn(a, b, prep):
    (P, D), Q, dev = a.shape, b.shape[0], a.device
    idx = torch.empty((P,), dtype=torch.int32, device=dev)
    dist = torch.empty((P,), dtype=torch.float32, device=dev)
    ws = torch.empty((lib.frmap_match_workspace_bytes(P, Q),), dtype=torch.uint8, device=dev)
    split = torch.empty((P, 3 * D), dtype=torch.float16, device=dev)
    args = (a.data_ptr(), b.data_ptr(), prep.packed.data_ptr(), prep.stat_w.data_ptr(), idx.data_ptr(), dist.data_ptr(), 0, 0,
            float("inf"), ws.data_ptr(), split.data_ptr(), P, Q, D)
    return lambda: _lib.check(lib.frmap_match_top1_packed(*args, st()), "match_top1_packed")


def clustered(ids, n, seed, D=512, per=8):
    c = synth.unit_rows(7, ids, D, "radius_bench").cuda()
    lab = (torch.arange(n, device="cuda") % ids).to(torch.int32) if n != ids * per else \
        torch.arange(ids, device="cuda", dtype=torch.int32).repeat_interleave(per)
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (c[lab.long()] + 0.5 / D ** 0.5 * torch.randn(n, D, device="cuda", generator=g)).contiguous(), lab


def quantile_thresholds(a, b, self_mode, shares, samples=1 << 23):
    """the `shares` quantiles of the counted pairs' distances, from a sample of pairs (plain torch; an estimate is all that is needed)"""
    g = torch.Generator(device="cuda").manual_seed(1)
    i = torch.randint(0, a.shape[0], (samples,), device="cuda", generator=g)
    j = torch.randint(0, b.shape[0], (samples,), device="cuda", generator=g)
    if self_mode:
        keep = i < j
        i, j = i[keep], j[keep]
    d = torch.cat([((a[i[k:k + (1 << 18)]] - b[j[k:k + (1 << 18)]]) + 1e-6).double().pow(2).sum(1).sqrt() for k in range(0, i.shape[0], 1 << 18)])
    d = d.sort().values
    return [float(d[max(int(s * d.shape[0]) - 1, 0)].float()) for s in shares]


SHARES = (1e-4, 1e-3, 1e-2)
for what, P, Q in (("cross", 1024, 10000), ("self", 16384, 16384), ("self", 32768, 32768)):
    self_mode = what == "self"
    b, lb = clustered(Q // 8, Q, Q)
    a, la = (b, lb) if self_mode else clustered(Q // 8, P, Q + 1)
    prep = ops.match_prepare(b)
    row0 = 0 if self_mode else -1
    pairs = P * (P - 1) // 2 if self_mode else P * Q
    t1 = t(top1_fn(a, b, prep))
    print(f"{what} {P} x {Q}, D = 512 ({pairs:.3e} pairs): match_top1_packed {t1:8.3f} ms", flush=True)
    for share, thr in zip(SHARES, quantile_thresholds(a, b, self_mode, SHARES)):
        tv = t(verify_fn(a, la, b, lb, prep, thr, row0))
        total = int(radius_fn(a, b, prep, thr, row0, 0)()[3].item())             # count-only: the list's exact size
        tc = t(radius_fn(a, b, prep, thr, row0, 0))
        fn = radius_fn(a, b, prep, thr, row0, total)
        ms = t(fn)
        _, _, counts, tot, resc = fn()
        assert int(tot.item()) == total == int(counts.sum().item())
        print(f"  t={thr:8.5f} (target {100 * share:5.2f} %): listed {100 * total / pairs:7.4f} %  re-scored {100 * int(resc.item()) / pairs:7.4f} %  "
              f"radius {ms:8.3f} ms ({pairs / ms * 1e3:9.3e} pairs/s)  count-only {tc:8.3f} ms  verify T=1 {tv:8.3f} ms  "
              f"-> {ms / tv:5.2f}x verify, {ms / t1:5.2f}x top-1", flush=True)
