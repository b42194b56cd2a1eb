"""The shape tables and the inputs of the hidden-layer head-fitting tests (`test_head_fit_hidden_cpu.py`, `test_head_fit_hidden_gpu.py`)
and of tools/head_fit_hidden_check.cpp, which carries the same CPU table.

Shapes are (B, D, Hd, C).  Every K of every GEMM crosses a 32-tile edge somewhere in the CPU table, and D, Hd, C and B each cross
the 128 chain cut; the hidden width Hd is both a K (layer 2 forward) and an N (back).  The two GPU-only shapes are the baseline's
head with full MFMA tiles everywhere but C, and a wide one.

Every case runs `STEPS` steps with `lr` changing per step, in two variations: both masks with coupled decay, and `keep2` only
with decoupled decay, AMSGrad and label smoothing.  Where the batch has room (B >= 4) one row has ``rows = -1``, one a label of C
and one a NaN feature.

Weights and features are zero-mean, so that about half of the pre-activations are negative: a wrong ReLU mask cannot hide.  The
builder asserts 0.3 <= share(h > 0) <= 0.7 wherever the counted rows hold at least `SHARE_MIN` hidden values; below that the share
of a zero-mean draw leaves that interval by chance alone (15 values: one draw in eight), so those cases only require both signs to
occur where there are two values or more."""
import numpy as np

F32 = np.float32
CPU_SHAPES = ((1, 1, 1, 1), (5, 2, 3, 1), (31, 3, 33, 2), (32, 64, 32, 18), (33, 65, 65, 33), (65, 129, 129, 129))
GPU_SHAPES = CPU_SHAPES + ((64, 128, 512, 36), (256, 512, 256, 1000))
STEPS = 3
LRS = (1e-2, 5e-3, 2e-2)
KEEP1_P, KEEP2_P = 0.25, 0.5
SHARE_MIN = 32
VARIATIONS = (
    {"name": "both-masks", "keep1": True, "keep2": True, "decoupled": False, "amsgrad": False, "label_smoothing": 0.0, "weight_decay": 1e-2},
    {"name": "keep2-adamw-ams-ls", "keep1": False, "keep2": True, "decoupled": True, "amsgrad": True, "label_smoothing": 0.1, "weight_decay": 1e-2},
)


def cases(shapes=CPU_SHAPES):
    return [(shape, var) for shape in shapes for var in VARIATIONS]


NO_MASKS = {"name": "no-masks", "keep1": False, "keep2": False, "decoupled": False, "amsgrad": False, "label_smoothing": 0.0, "weight_decay": 0.0}


def case_id(case):
    return "B%d-D%d-Hd%d-C%d-%s" % (*case[0], case[1]["name"])


def step_kw(var, s, clear=None):
    """The keyword arguments of step `s` of a variation, for `hidden_step`, `hidden_step_host` and `hidden_step_rule` alike."""
    return dict(lr=LRS[s % len(LRS)], weight_decay=var["weight_decay"], label_smoothing=var["label_smoothing"], decoupled=var["decoupled"],
                amsgrad=var["amsgrad"], clear=(s == 0) if clear is None else clear)


def keep_scales(var):
    return (1.0 / (1.0 - KEEP1_P) if var["keep1"] else 1.0), (1.0 / (1.0 - KEEP2_P) if var["keep2"] else 1.0)


def share_positive(p):
    """The share of positive pre-activations over the counted rows of a problem (float64, no mask), and how many values that is."""
    ok = np.array([0 <= r < len(p["x"]) and 0 <= p["labels"][r] < p["C"] and np.isfinite(p["x"][r]).all() for r in p["rows"]])
    if not ok.any():
        return float("nan"), 0
    a = p["x"][p["rows"][ok]].astype(np.float64) @ p["w1"].astype(np.float64).T + p["b1"].astype(np.float64)
    return float((a > 0).mean()), int(a.size)


def problem(seed, B, D, Hd, C, var, declined=True):
    """A dict of host arrays: x [N, D], labels [N], rows [B], w1 [Hd, D], b1 [Hd], w2 [C, Hd], b2 [C], keep1 [B, D] or None,
    keep2 [B, Hd] or None.  Features are multiples of 1/64 in [-1, 1], weights zero-mean normal draws of nn.Linear's scale; with
    `declined` and B >= 4 three batch rows are bad (the docstring of the module)."""
    rng = np.random.default_rng(seed)
    N = B + 5
    x = (rng.integers(-64, 65, (N, D)) / 64.0).astype(F32)
    labels = rng.integers(0, C, N).astype(np.int32)
    rows = rng.permutation(N)[:B].astype(np.int32)
    w1 = (rng.standard_normal((Hd, D)) / np.sqrt(D)).astype(F32)
    b1 = (rng.standard_normal(Hd) * 0.05).astype(F32)
    w2 = (rng.standard_normal((C, Hd)) / np.sqrt(Hd)).astype(F32)
    b2 = (rng.standard_normal(C) * 0.05).astype(F32)
    keep1 = (rng.random((B, D)) >= KEEP1_P).astype(np.uint8) if var["keep1"] else None
    keep2 = (rng.random((B, Hd)) >= KEEP2_P).astype(np.uint8) if var["keep2"] else None
    bad = []
    if declined and B >= 4:
        rows[1] = -1
        labels[rows[2]] = C
        x[rows[3], D // 2] = np.nan
        bad = [1, 2, 3]
    p = {"x": x, "labels": labels, "rows": rows, "w1": w1, "b1": b1, "w2": w2, "b2": b2, "keep1": keep1, "keep2": keep2, "bad": bad,
         "B": B, "D": D, "Hd": Hd, "C": C, "N": N}
    share, count = share_positive(p)
    if count >= SHARE_MIN:
        assert 0.3 <= share <= 0.7, ("share of positive pre-activations", share, (B, D, Hd, C))
    elif count >= 2:
        assert 0.0 < share < 1.0, ("both signs of the pre-activations", share, (B, D, Hd, C), seed)
    return p


def without_bad_rows(p):
    """The same problem with the bad batch rows removed and B smaller: the counted rows, in their order, with their mask rows."""
    good = [i for i in range(p["B"]) if i not in p["bad"]]
    q = dict(p)
    q["rows"] = p["rows"][good].copy()
    q["keep1"] = None if p["keep1"] is None else p["keep1"][good].copy()
    q["keep2"] = None if p["keep2"] is None else p["keep2"][good].copy()
    q["B"], q["bad"] = len(good), []
    return q
