"""Cases of the grouped head-fitting tests (`test_head_fit_group_cpu.py`, `test_head_fit_group_gpu.py`): a plain helper module like
`fit_cases.py` (no fixture, no setting).

SHAPES.  `HEADS` x `SHAPES`: one, two and five heads; (B, D, C) from one row, one feature, one class over one short of / exactly /
one past the 32-wide tile to more than one tile and four whole 128-chains.  (5, 2, 1) runs with AMSGrad: C D + C = 3 is odd, so the
state's content (64 + 12 x 3 = 100 bytes) is no multiple of 8 and the bytes up to the stride are padding.  Every case runs three
steps; whether it has masks, decoupled decay or AMSGrad comes from its index (`cases`), the hyper-parameters differ in every column
from head to head (`hyper`), head h's rows end in min(h, B - 1) entries of -1, and in `DEAD` cases one head's rows are ALL -1.

DATA.  `problem`: a cache of N = B + 5 + H rows of small multiples of 2^-6 shared by the heads (so products are exact in few bits
and ties happen), per-head weights, and - where the batch has room - rows of every declined kind.

`slices` cuts the group's operands into the single-head operands of head h, which is what the contract is stated on: head h of a
grouped step has exactly the bits of the single step on these.
"""
import numpy as np

from frmap_amd import head_fit as hf

HEADS = (1, 2, 5)
SHAPES = ((1, 1, 1), (5, 2, 1), (31, 3, 2), (32, 64, 18), (33, 65, 33), (65, 512, 65))
STEPS = 3
DEAD = {(5, (33, 65, 33)): 2, (2, (5, 2, 1)): 0}            # (H, shape) -> the head whose rows are all declined
F32 = np.float32


def cases():
    """[(H, B, D, C, variation)]: every shape with every head count; the variation bits from the index."""
    out = []
    for s, (B, D, C) in enumerate(SHAPES):
        for k, H in enumerate(HEADS):
            i = 3 * s + k
            out.append((H, B, D, C, {"keep": bool(i & 1), "decoupled": bool(i & 2), "amsgrad": bool(i & 4) or (B, D, C) == (5, 2, 1),
                                     "dead": DEAD.get((H, (B, D, C)))}))
    return out


def case_id(case):
    H, B, D, C, var = case
    return "H%d-B%d-D%d-C%d%s%s%s%s" % (H, B, D, C, "-keep" if var["keep"] else "", "-adamw" if var["decoupled"] else "",
                                        "-ams" if var["amsgrad"] else "", "" if var["dead"] is None else "-dead%d" % var["dead"])


def hyper(H: int, keep: bool, step: int = 0) -> np.ndarray:
    """The [H, 8] table of step `step`: every column differs from head to head, head 0 has no smoothing, and the learning rate
    changes from step to step (the table is what a caller rewrites between steps)."""
    h = np.arange(H, dtype=np.float64)
    return hf.hyper_table(H, lr=1e-2 * (1 + h / 4) * (1 + step / 2), beta1=0.9 - 0.01 * h, beta2=0.999 - 0.001 * h, eps=1e-8 * (1 + h),
                          weight_decay=5e-3 * (h + 1), label_smoothing=0.05 * h / max(H, 1), keep_scale=(1.0 / (0.75 - 0.05 * (h % 5))) if keep else 1.0)


def problem(seed: int, H: int, B: int, D: int, C: int, keep: bool = True, dead=None, declined: bool = True):
    """``(x [N, D] f32, labels [N] i32, w [H, C, D] f32, b [H, C] f32, rows [H, B] i32, keep [H, B, D] u8 or None)``."""
    rng = np.random.default_rng(seed)
    N = B + 5 + H
    x = (rng.integers(-64, 65, (N, D)) / 64.0).astype(F32)
    labels = rng.integers(0, C, N).astype(np.int32)
    w = (rng.integers(-32, 33, (H, C, D)) / 256.0).astype(F32)
    b = (rng.integers(-32, 33, (H, C)) / 256.0).astype(F32)
    rows = np.stack([rng.permutation(N)[:B] for _ in range(H)]).astype(np.int32)
    k = (rng.random((H, B, D)) >= 0.25).astype(np.uint8) if keep else None
    if declined and B >= 6:
        r0 = rows[0]
        labels[r0[1]] = C                         # a label out of range
        x[r0[2], rng.integers(0, D)] = np.nan     # a NaN feature
        x[r0[3], D - 1] = np.inf                  # an infinity in the last feature
        labels[r0[4]] = -1
        rows[:, 0] = N                            # a rows entry past the cache in every head
    for h in range(H):                            # head h is padded with min(h, B - 1) entries of -1
        pad = min(h, B - 1)
        if pad:
            rows[h, B - pad:] = -1
    if dead is not None:
        rows[dead, :] = -1
    return x, labels, w, b, rows, k


def content_bytes(D, C, amsgrad):
    """Bytes of a state that hold something: the header and the moments (the stride may add padding behind them)."""
    return 64 + 4 * (C * D + C) * (3 if amsgrad else 2)


def fresh_states(H, D, C, amsgrad, fill=0):
    """H fresh states `group_state_stride` apart: zeroed contents, the padding bytes between them at `fill`."""
    stride, content = hf.group_state_stride(D, C, amsgrad), content_bytes(D, C, amsgrad)
    st = np.full((H * stride,), fill, np.uint8)
    for h in range(H):
        st[h * stride: h * stride + content] = 0
    return st


def slices(h, H, B, D, C, amsgrad, w, b, rows, keep, state, workspace=None):
    """Head h's single-head operands, cut from the group's (numpy arrays; views): ``(w, b, rows, keep, state, workspace)``."""
    stride, single = hf.group_state_stride(D, C, amsgrad), hf.state_bytes(D, C, amsgrad)
    work = hf.workspace_bytes(B, D, C)
    return (w[h], b[h], rows[h], None if keep is None else keep[h], state[h * stride: h * stride + single],
            None if workspace is None else workspace[h * work: (h + 1) * work])


def single_kw(table, h, var, clear=False):
    """The keyword arguments of `head_fit.step` / `step_host` that row h of a hyper table stands for."""
    r = table[h]
    return dict(lr=float(r[0]), beta1=float(r[1]), beta2=float(r[2]), eps=float(r[3]), weight_decay=float(r[4]), label_smoothing=float(r[5]),
                decoupled=var["decoupled"], amsgrad=var["amsgrad"], clear=clear)
