"""Shared code of the classification-tally tests (`test_tally_cpu.py`, `test_tally_gpu.py`).  A plain helper module like
`conv_cases.py` and `guard.py` (no fixture, no setting).

* `SWEEP_*`: the grid of tools/classify_tally_check.cpp (C x R x n_bins, the confusion matrix kept and not).
* `host_rows`: rows for the CPU sweep - labels out of range, non-finite logits, many ties, confidences at both ends and on
  the bin edges, losses at and above the clamp.  conf and loss are plain fp32 inputs there: the twin and the numpy rule are fed
  the same arrays, so no libm enters the comparison.
* `gpu_rows(C)`: the 259 rows of width C the GPU tests share (a case of B rows takes the first B), built once per C with
  their float64 reference: `synth.randn * 3` with the target raised by 2; row 1 alternates +-80, row 2 has a tie inside one lane
  (columns 0 and 64), row 3 a tie across lanes (columns 63 and 65), row 4 a target tied with the maximum at a higher index
  (rank 1, not 0).  A row whose float64 confidence comes within `EDGE_CLEAR` of a bin edge is rescaled (x 1.03, which keeps ties
  and the arg-max) until it is clear, so the bins cannot hinge on the last bits of a softmax.
* `kernel_order_rows`: a numpy float32 restatement of the kernel's summation order - lane-strided partial sums, then the xor
  butterfly - with numpy's fp32 exp / log: the CPU measurement the loss gate is a multiple of.
"""
import functools

import numpy as np
import torch

from frmap_amd import evaluate, synth

SWEEP_C = (1, 2, 63, 64, 65, 1000)
SWEEP_R = (1, 6, 1024)
SWEEP_BINS = (1, 2, 10, 1024)
SPLIT = (1, 101)                    # 1 + 100 + 158 rows
B_FULL = 259
EDGE_CLEAR = 1e-4                   # the builders clear this much; the tests assert `EDGE_ASSERT`
EDGE_ASSERT = 1e-5
RANKS, N_BINS = 6, 10               # the defaults of `ops.classify_tally`
F32 = np.float32


def host_rows(seed, B, C, n_bins):
    rng = np.random.default_rng([seed, B, C, n_bins])
    z = ((rng.integers(0, 13, (B, C)) - 6) * 0.5).astype(F32)               # few values: many ties
    y = rng.integers(0, C, B).astype(np.int32)
    i = np.arange(B)
    y[i % 11 == 3] = -1
    y[i % 11 == 5] = C
    y[i % 11 == 6] = 2 ** 31 - 1
    for k, v in ((7, np.nan), (8, np.inf), (9, -np.inf)):
        rows = np.nonzero(i % 11 == k)[0]
        z[rows, rng.integers(0, C, len(rows))] = v
    both = i % 22 == 14                                                       # out of range AND non-finite: ignored
    y[both] = -5
    z[both, 0] = np.nan
    conf = rng.random(B).astype(F32)
    conf[i % 7 == 0] = 1.0
    conf[i % 7 == 1] = 0.0
    on_edge = np.nonzero(i % 7 == 2)[0]
    conf[on_edge] = evaluate.tally_edges(n_bins)[rng.integers(0, n_bins, len(on_edge))].astype(F32)
    loss = (rng.random(B) * 20).astype(F32)
    loss[i % 5 == 0] = 0.0
    loss[i % 5 == 1] = 65536.0
    loss[i % 5 == 2] = 3.0e9
    return z, y, conf, loss


def edge_distance(conf64, n_bins=N_BINS):
    """Per row: the distance of a float64 confidence to the nearest bin edge."""
    return np.abs(np.asarray(conf64, np.float64)[:, None] - evaluate.tally_edges(n_bins)[None, :]).min(axis=1)


def clear_of_edges(z, y, n_bins=N_BINS):
    """Rescale (x 1.03: ties and the arg-max survive) every row whose float64 confidence lies within EDGE_CLEAR of a bin edge,
    unless that confidence is exactly 1.0 (see `assert_no_knife_edge`)."""
    for _ in range(50):
        _, _, conf, _ = evaluate.tally_rows_reference(z, y)
        near = np.nonzero((edge_distance(conf, n_bins) < EDGE_CLEAR) & (conf != 1.0))[0]
        if near.size == 0:
            return z
        z[near] = (z[near] * F32(1.03)).astype(F32)
    raise AssertionError("rows %s stay within %g of a bin edge" % (near.tolist(), EDGE_CLEAR))


def assert_no_knife_edge(conf64, n_bins=N_BINS):
    """From the float64 reference, for EVERY counted row: the confidence is at least EDGE_ASSERT from every bin edge - or it is
    exactly 1.0 in float64.  The second arm is not a row left out: a row of one class (C = 1 is a shape the tests must cover) or
    the +-80 row of C = 2 has sum_c exp(z[c] - max) == 1 exactly in float64, so every other term is below 2^-53; the same
    terms in fp32 are then below 2^-24 / 1000 each, the fp32 sum of at most 1000 of them onto 1.0f is 1.0f, and conf is 1.0f on
    any machine: it sits ON the last edge by the rule's own quirk, not next to it."""
    c = np.asarray(conf64, np.float64)
    c = c[~np.isnan(c)]
    d = edge_distance(c, n_bins)
    bad = np.nonzero((d < EDGE_ASSERT) & (c != 1.0))[0]
    assert bad.size == 0, (bad.tolist(), c[bad].tolist())
    return float(d[c != 1.0].min()) if (c != 1.0).any() else float("inf")


@functools.lru_cache(maxsize=None)
def gpu_rows(C):
    """(logits fp32 [259, C], labels int32 [259], float64 reference (pred, rank, conf, loss)) - built once, never modified."""
    B = B_FULL
    z = (synth.randn(2600 + C, (B, C), "tally") * 3).numpy().astype(F32)
    y = np.random.default_rng([2600, C]).integers(0, C, B).astype(np.int32)
    z[np.arange(B), y] += F32(2.0)
    z[1] = np.where(np.arange(C) % 2 == 0, 80.0, -80.0).astype(F32)           # exp(-160) underflows, exp(0) does not overflow
    y[1] = 0
    if C > 64:                                                                # a tie inside one lane: the first index wins
        z[2, 0] = z[2, 64] = z[2].max() + F32(1.0)
        y[2] = 64
    if C > 65:                                                                # a tie across lanes 63 and 1
        z[3, 63] = z[3, 65] = z[3].max() + F32(1.0)
        y[3] = 65
    if C >= 2:                                                                # the target ties the maximum at a higher index
        z[4, 0] = z[4, C - 1] = z[4].max() + F32(1.0)
        y[4] = C - 1
    z = clear_of_edges(z, y)
    ref = evaluate.tally_rows_reference(z, y)
    if C >= 2:
        assert ref[0][4] == 0 and ref[1][4] == 1 and ref[0][1] == 0 and ref[1][1] == 0
    if C > 65:
        assert ref[0][2] == 0 and ref[1][2] == 1 and ref[0][3] == 63 and ref[1][3] == 1
    z.setflags(write=False)
    y.setflags(write=False)
    return z, y, ref


def kernel_order_rows(z, y):
    """(conf, loss) in float32 in the kernel's own summation order, for rows that are all counted: per lane l the terms
    exp(z[c] - max) of c = l, l + 64, ... added in turn, then the butterfly s[l] += s[l ^ o] for o = 32, 16, ... 1; conf = 1 / s,
    loss = max(0, log(s) + (max - z[y])).  numpy's fp32 exp and log."""
    z = np.asarray(z, F32)
    B, C = z.shape
    mx = z.max(axis=1)
    e = np.exp((z - mx[:, None]).astype(F32)).astype(F32)
    chunks = -(-C // 64)
    pad = np.zeros((B, chunks * 64), F32)
    pad[:, :C] = e
    pad = pad.reshape(B, chunks, 64)
    s = np.zeros((B, 64), F32)
    for k in range(chunks):
        s = (s + pad[:, k, :]).astype(F32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, lanes ^ o]).astype(F32)
    assert (s == s[:, :1]).all()                                              # every lane ends with the same bits
    s = s[:, 0]
    zy = z[np.arange(B), np.asarray(y, np.int64)]
    conf = (F32(1.0) / s).astype(F32)
    loss = np.maximum(F32(0.0), (np.log(s).astype(F32) + (mx - zy).astype(F32)).astype(F32)).astype(F32)
    return conf, loss


GPU_C = (1, 2, 36, 63, 64, 65, 129, 1000)
GPU_B = (1, 5, 259)
LOSS_FLOOR = 2.0 ** -22



def t(a, dtype=None):
    """A numpy array as a (writable) CPU tensor."""
    out = torch.from_numpy(np.array(a))
    return out if dtype is None else out.to(dtype)
