"""Cases of the head-fitting tests (`test_head_fit_cpu.py`, `test_head_fit_gpu.py`): a plain helper module like `tally_cases.py`
(no fixture, no setting).

SHAPES.  `SWEEP_B` x `SWEEP_D` x `SWEEP_C` are the issue's: one row and one class, one short of / exactly / one past the 32-wide
tile of both GEMMs, more than one tile, D = 1 and 3 (a chain shorter than one MFMA step), 64 / 65 (one past a staging step) and
512 (four whole chains).  Every shape runs three steps; the VARIATION of a shape - with or without ``rows``, ``keep``, AMSGrad,
decoupled decay, label smoothing - is taken from its index, so that the sweep covers every variation on every kind of edge
without multiplying the cases (`variation`).

DATA.  `problem(seed, B, D, C)`: a cache of N = B + 5 rows of small multiples of 2^-6 (so products are exact in few bits and ties
happen), labels in range, and - where the batch has room - one row of each declined kind: a ``rows`` entry out of range, a label
out of range, a NaN feature, an infinite feature.
"""
import numpy as np

SWEEP_B = (1, 31, 32, 33, 65)
SWEEP_D = (1, 3, 64, 65, 512)
SWEEP_C = (1, 2, 18, 33, 65)
STEPS = 3
TILE_EDGES = ((1024, 512, 1000), (64, 512, 10000))        # (B, D, C), one step each
F32 = np.float32


def shapes():
    return [(B, D, C) for B in SWEEP_B for D in SWEEP_D for C in SWEEP_C]


def variation(index: int) -> dict:
    """The optional operands and optimiser flags of case ``index``: five independent bits, all 32 combinations within 32 cases."""
    return {"rows": bool(index & 1), "keep": bool(index & 2), "amsgrad": bool(index & 4), "decoupled": bool(index & 8),
            "label_smoothing": 0.05 if index & 16 else 0.0}


HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)


def problem(seed: int, B: int, D: int, C: int, declined: bool = True, rows: bool = True, keep: bool = True):
    """``(x [N, D] f32, labels [N] i32, w [C, D] f32, b [C] f32, rows [B] i32 or None, keep [B, D] u8 or None)``."""
    rng = np.random.default_rng(seed)
    N = B + 5
    x = (rng.integers(-64, 65, (N, D)) / 64.0).astype(F32)
    labels = rng.integers(0, C, N).astype(np.int32)
    w = (rng.integers(-32, 33, (C, D)) / 256.0).astype(F32)
    b = (rng.integers(-32, 33, (C,)) / 256.0).astype(F32)
    r = rng.permutation(N)[:B].astype(np.int32) if rows else None
    k = (rng.random((B, D)) >= 0.25).astype(np.uint8) if keep else None
    if declined and B >= 6:
        src = r if r is not None else np.arange(B, dtype=np.int32)
        labels[src[1]] = C                        # a label out of range
        x[src[2], rng.integers(0, D)] = np.nan    # a NaN feature
        x[src[3], D - 1] = np.inf                 # an infinity in the last feature
        labels[src[4]] = -1
        if r is not None:
            r[0], r[5] = -1, N                    # rows entries out of range on both sides
    return x, labels, w, b, r, k


def ulp32(v64):
    """One float32 unit in the last place at the magnitude of float64 values (2^-149 below the normal range)."""
    v = np.abs(np.asarray(v64, np.float64))
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -126)))
    return 2.0 ** (e - 23)


def softmax64(z, labels_of_rows, n, ls, C):
    """g and the row loss of float32 logits ``z`` [B, C] in float64 (the formulas of the rule): ``(g, loss)``.  ``ls`` is the
    float32 the step receives by value."""
    ls = float(F32(ls))
    z = z.astype(np.float64)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    nl = np.log(s) + (m - z)
    y = np.full(z.shape, ls / C)
    y[np.arange(len(z)), labels_of_rows] += 1.0 - ls
    return (e / s - y) / float(n), (y * nl).sum(axis=1)


def softmax32(z, labels_of_rows, n, ls, C):
    """The same in float32 the way a wavefront sums: lane-strided partial sums over 64 lanes, then the xor butterfly - a numpy
    restatement whose deviation from `softmax64` sets the gate of the device's (4 x, the tally's convention)."""
    z = z.astype(F32)
    Bn = len(z)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m).astype(F32)

    def wave_sum(v):
        lanes = np.zeros((Bn, 64), F32)
        for c in range(v.shape[1]):
            lanes[:, c % 64] = lanes[:, c % 64] + v[:, c]
        o = 32
        while o:
            lanes = lanes + lanes[:, np.arange(64) ^ o]
            o >>= 1
        return lanes[:, :1]
    s = wave_sum(e)
    lse = np.log(s).astype(F32)
    nl = (lse + (m - z)).astype(F32)
    nll = nl[np.arange(Bn), labels_of_rows]
    lsf = F32(ls)
    y_off = lsf / F32(C) if ls > 0 else F32(0)
    y_on = (F32(1) - lsf) + y_off
    loss = nll if ls == 0 else (y_off * wave_sum(nl)[:, 0] + (F32(1) - lsf) * nll).astype(F32)
    y = np.full(z.shape, y_off, F32)
    y[np.arange(Bn), labels_of_rows] = y_on
    return (((e / s).astype(F32) - y) / F32(n)).astype(F32), np.maximum(loss, 0).astype(F32)
