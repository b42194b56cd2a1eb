#!/usr/bin/env python3
"""Micro-benchmark of the exact verification counts (frmap_verify_counts_packed on a prepared set) against the top-1 match on the same
N x N square (HIP events, one process).  Synthetic clustered identities: N / 8 unit-norm centres (synth.unit_rows), 8 noisy
enrolments each, D = 512.  N in {4096, 16384, 32768}, T in {1, 64, 256, 1024} evenly spaced thresholds over the distance range
(T = 1 at t = 0: nothing straddles, the GEMM + binning floor), self mode (N (N - 1) / 2 pairs) and cross mode (N x N pairs).
Prints ms, pairs/s and the share of pairs re-scored exactly.  The verify calls are timed at the C entry point with device thresholds
checked once up front and buffers allocated once: `ops.verify_counts` checks thresholds through a host copy, which synchronises."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from frmap_amd import _lib, evaluate, ops, synth
def t(fn, n=5):
    for _ in range(2): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
lib = _lib.load()


def verify_fn(a, la, thr, b=None, lb=None, prep=None):
    """a launch-only closure over frmap_verify_counts[_packed] (self mode over `a` when b is None); returns (counts, rescored)"""
    P, D = a.shape
    b, lb, row0 = (a, la, 0) if b is None else (b, lb, -1)
    Q = b.shape[0]
    td = ops.verify_thresholds(thr, a.device)         # checked once, here
    T = td.shape[0]
    out = torch.empty((2, T), dtype=torch.int64, device=a.device)
    resc = torch.empty((1,), dtype=torch.int64, device=a.device)
    ws = torch.empty((lib.frmap_verify_workspace_bytes(P, Q, D, T),), dtype=torch.uint8, device=a.device)
    st = torch.cuda.current_stream().cuda_stream
    if prep is not None:
        args = (a.data_ptr(), la.data_ptr(), P, b.data_ptr(), prep.packed.data_ptr(), prep.stat_w.data_ptr(), lb.data_ptr(), Q, D, row0,
                td.data_ptr(), T, out.data_ptr(), resc.data_ptr(), ws.data_ptr(), st)
        call = lambda: _lib.check(lib.frmap_verify_counts_packed(*args), "verify_counts_packed")
    else:
        args = (a.data_ptr(), la.data_ptr(), P, b.data_ptr(), lb.data_ptr(), Q, D, row0, td.data_ptr(), T, out.data_ptr(), resc.data_ptr(),
                ws.data_ptr(), st)
        call = lambda: _lib.check(lib.frmap_verify_counts(*args), "verify_counts")

    def run():
        call()
        return out, resc
    return run


D, PER = 512, 8
for N in (4096, 16384, 32768):
    ids = N // PER
    c = synth.unit_rows(7, ids, D, "verify_bench").cuda()
    lab = torch.arange(ids, device="cuda", dtype=torch.int32).repeat_interleave(PER)
    g = torch.Generator(device="cuda").manual_seed(N)
    x = (c[lab.long()] + 0.5 / D ** 0.5 * torch.randn(N, D, device="cuda", generator=g)).contiguous()
    y = (c[lab.long()] + 0.5 / D ** 0.5 * torch.randn(N, D, device="cuda", generator=g)).contiguous()
    px, py = ops.match_prepare(x), ops.match_prepare(y)
    t1 = t(lambda: ops.match_top1(x, y, prepared=py))
    print(f"N={N}: match_top1_packed (B = G = {N}) {t1:8.3f} ms", flush=True)
    for T in (1, 64, 256, 1024):
        thr = np.zeros(1, np.float32) if T == 1 else evaluate.default_thresholds(x, y, T)
        for mode in ("self", "cross"):
            if mode == "self":
                fn = verify_fn(x, lab, thr, prep=px)
                pairs = N * (N - 1) // 2
            else:
                fn = verify_fn(x, lab, thr, y, lab, prep=py)
                pairs = N * N
            ms = t(fn)
            _, resc = fn()
            frac = int(resc.item()) / pairs
            print(f"  T={T:4d} {mode:5s}: {ms:8.3f} ms  {pairs / ms * 1e3:9.3e} pairs/s  ({ms / t1:4.2f}x top-1)  "
                  f"re-scored {100 * frac:6.3f} %", flush=True)
    if N == 4096:
        thr = evaluate.default_thresholds(x, y, 256)
        ms = t(verify_fn(x, lab, thr), n=2)
        print(f"  exact scan, T= 256 self: {ms:8.3f} ms  {N * (N - 1) // 2 / ms * 1e3:9.3e} pairs/s", flush=True)
