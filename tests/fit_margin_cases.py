"""The shape tables and the inputs of the margin head-fitting tests (`test_head_fit_margin_cpu.py`, `test_head_fit_margin_gpu.py`) and of
tools/head_fit_margin_check.cpp, which walks a part of the same table.

Shapes are (B, D, C): B and C cross the 32-row tile and the wavefront, D the tile and the 128 chain.  Every case runs `STEPS` steps with
`lr`, the effective scale and margin, the easy margin and the label smoothing changing per step (`step_kw`), in a variation chosen by
the shape's index, so that the table covers Adam / AdamW, AMSGrad and a step with and without a dropout mask.

KNIFE EDGES.  The rule has four comparisons that a last bit can flip: the two clamp bounds, the cap, easy margin's ``cs > 0`` and the
arg-max.  `assert_no_knife_edge` holds every table to, in float64: every element has ``|cos| <= 1 - 1e-5`` or saturates at ``|cos| >= 1 -
1e-9`` by construction; every target has ``|theta + m - cap| > 1e-4``; under easy margin every target has ``|cos| > 1e-4`` or is an exact
0.  A case that violates one gets another seed (`RESEED`), never another condition.  What saturates by construction: D = 1 (features
are then signed powers of two, so that ``1 / |x'|`` is exact in fp32 and the fp32 cosine is off 1 by one rounding, inside the
saturated side of the fp32 bound; the mask scale is 2 for the same reason), and the hand-built rows of `branch_problem`."""
import numpy as np

F32 = np.float32
BS, DS, CS = (1, 31, 32, 33, 65), (1, 3, 64, 65, 512), (1, 2, 18, 33, 65)
CPU_SHAPES = tuple((B, D, C) for B in BS for D in DS for C in CS)
GPU_SHAPES = CPU_SHAPES + ((1024, 512, 1000), (64, 512, 10000))
STEPS = 3
LRS = (1e-2, 5e-3, 2e-2)
SCALES = (7.2, 9.6, 5.28)                # effective scales within the reference's schedule (at most 19.2)
MARGINS = (0.0, 0.27, 0.45)              # effective margins: epoch 0, a warm-up epoch, 0.5 x 0.9
KEEP_P = 0.5                             # (keep_scale = 2: exact)
EDGE_COS, SATURATED, EDGE_CAP, EDGE_EASY = 1e-5, 1e-9, 1e-4, 1e-4
CAP = float(F32(np.pi - 1e-4))
VARIATIONS = (
    {"name": "adam-mask", "keep": True, "decoupled": False, "amsgrad": False, "weight_decay": 1e-2},
    {"name": "adamw-ams", "keep": False, "decoupled": True, "amsgrad": True, "weight_decay": 1e-2},
)
# shape -> the seed's offset (see KNIFE EDGES): in three dimensions, dozens of rows against dozens of centres come within 1e-5 of parallel
RESEED = {(33, 3, 18): 1000, (65, 3, 65): 1000}


def variation(shape):
    return VARIATIONS[GPU_SHAPES.index(shape) % 2]


def case_seed(shape):
    """The seed of a shape of the contract tests: the same problem on the CPU and on the GPU."""
    return 3000 + GPU_SHAPES.index(shape) + RESEED.get(shape, 0)


def case_id(shape):
    return "B%d-D%d-C%d" % shape


def step_kw(var, k, clear=None):
    """The keyword arguments of step `k` of a variation, for `margin_step`, `margin_step_host` and `margin_step_rule` alike: easy margin
    on the odd steps, label smoothing on the steps after the first."""
    return dict(lr=LRS[k % 3], s=SCALES[k % 3], m=MARGINS[k % 3], easy_margin=bool(k & 1), label_smoothing=0.05 if k else 0.0,
                weight_decay=var["weight_decay"], decoupled=var["decoupled"], amsgrad=var["amsgrad"], clear=(k == 0) if clear is None else clear)


def keep_scale(var):
    return 1.0 / (1.0 - KEEP_P) if var["keep"] else 1.0


def problem(seed, B, D, C, var):
    """A dict of host arrays: x [N, D], labels [N], rows [B] (a draw without repeats from the N = B + 3 cached rows), w [C, D], keep
    [B, D] or None.  Features are multiples of 1/64 in [-1, 1] (D = 1: signed powers of two) with a non-zero feature 0, which a mask
    keeps; weights are normal draws of the reference's initial scale."""
    rng = np.random.default_rng(seed)
    N = B + 3
    x = (rng.integers(-64, 65, (N, D)) / 64.0).astype(F32)
    x[x[:, 0] == 0, 0] = 0.5
    if D == 1:
        x = (np.sign(x) * np.exp2(rng.integers(-3, 2, (N, 1)))).astype(F32)
    labels = rng.integers(0, C, N).astype(np.int32)
    rows = rng.permutation(N)[:B].astype(np.int32)
    w = (rng.standard_normal((C, D)) * np.sqrt(4.0 / (C + D))).astype(F32)
    if B >= 256:
        # (a thousand targets with chance cosines would put one within 1e-4 of 0 for certain: a row leans towards its class centre)
        lean = w[labels] / np.sqrt((w[labels].astype(np.float64) ** 2).sum(axis=1, keepdims=True))
        x = (np.round((x + 0.6 * np.sqrt(D / 3.0) * lean) * 64.0) / 64.0).astype(F32)
    keep = (rng.random((B, D)) >= KEEP_P).astype(np.uint8) if var["keep"] else None
    if keep is not None:
        keep[:, 0] = 1
    return {"x": x, "labels": labels, "rows": rows, "w": w, "keep": keep, "B": B, "D": D, "C": C, "N": N}


def assert_no_knife_edge(rule_out, easy, what=""):
    """The three conditions of KNIFE EDGES on the float64 intermediates of a `margin_step_rule` result (its ``detail``), counted rows
    only.  Returns ``(the largest unsaturated |cos|, the smallest |theta + m - cap|)``."""
    det, ok, y = rule_out["detail"], rule_out["ok"], rule_out["y"]
    if not ok.any():
        return 0.0, float("inf")
    a = np.abs(det["cos"][ok])
    free = a < 1.0 - SATURATED
    worst = float(a[free].max()) if free.any() else 0.0
    assert worst <= 1.0 - EDGE_COS, (what, "an element's |cos| is within 1e-5 of the clamp without saturating", worst)
    rows = np.flatnonzero(ok)
    tm = det["theta_m"][rows]
    cy = det["cs"][rows, y[rows]]
    gap = float(np.abs(tm - CAP).min())
    if not easy:
        assert gap > EDGE_CAP, (what, "a target's theta + m is within 1e-4 of the cap", gap)
    else:
        assert ((np.abs(cy) > EDGE_EASY) | (cy == 0)).all(), (what, "an easy-margin target's cos is within 1e-4 of 0", float(np.abs(cy).min()))
    return worst, gap


# Hand-built rows, one per branch: D = 4, C = 4, the class centres small integers.  Centre 0 is (1, 1, 1, 1): its norm 2 and the norms
# of its exact multiples are exact in fp32, so row 1's cosine is exactly 1 on every side.
BRANCH_ROWS = ("capped target", "clamped element", "zero-norm row", "target on the zero centre", "ordinary", "ordinary, wrong class near")


def branch_problem():
    """x [6, 4], labels [6], w [4, 4]: row 0 is ``-1.5 w_0`` nudged off the axis (|cos| = 1 - 4.4e-5: a capped target that the clamp
    passes), row 1 is ``2 w_0`` (cos exactly 1: clamped), row 2 is zeros (rx = 1e12, every cos an exact 0), row 3's target is class 3,
    whose centre is zeros (rw = 1e12, no projection term), rows 4 and 5 are ordinary."""
    w = np.array([[1, 1, 1, 1], [1, -1, 0.5, 0], [-0.5, 0.25, 1, -1], [0, 0, 0, 0]], F32)
    x = np.array([[-1.48, -1.52, -1.5, -1.5], [2, 2, 2, 2], [0, 0, 0, 0], [0.5, -0.25, 0.75, 1], [1, -0.5, 0.25, 0.125], [-0.25, 0.5, 1, -0.5]], F32)
    labels = np.array([0, 0, 1, 3, 1, 0], np.int32)
    return {"x": x, "labels": labels, "rows": None, "w": w, "keep": None, "B": 6, "D": 4, "C": 4, "N": 6}


BRANCH_KW = dict(lr=1e-2, s=9.6, m=0.45, label_smoothing=0.05, weight_decay=1e-2, decoupled=True, amsgrad=True)

BAD_KINDS = ("row -1", "row N", "label -1", "label C", "nan feature", "inf feature")


def with_bad_row(p, kind, at):
    """The problem with one more batch row INSERTED before row `at`, declined in the way `kind` says; its mask row is ones.  The cache
    gains a row for it, so that no other batch row reads what was spoiled."""
    q = dict(p)
    x = np.concatenate([p["x"], p["x"][:1]])
    labels = np.concatenate([p["labels"], p["labels"][:1]])
    N = len(x)
    r = N - 1
    if kind == "row -1":
        r = -1
    elif kind == "row N":
        r = N
    elif kind == "label -1":
        labels[N - 1] = -1
    elif kind == "label C":
        labels[N - 1] = p["C"]
    elif kind == "nan feature":
        x[N - 1, p["D"] // 2] = np.nan
    elif kind == "inf feature":
        x[N - 1, 0] = -np.inf
    else:
        raise KeyError(kind)
    rows = p["rows"] if p["rows"] is not None else np.arange(p["B"], dtype=np.int32)
    q["x"], q["labels"], q["N"], q["B"] = x, labels, N, p["B"] + 1
    q["rows"] = np.insert(rows, at, r).astype(np.int32)
    if p["keep"] is not None:
        q["keep"] = np.concatenate([p["keep"][:at], np.ones((1, p["D"]), np.uint8), p["keep"][at:]])
    return q


# The synthetic fit: 8 classes of clustered unit vectors in 16 dimensions (noise 0.35 around unit centres), 256 rows to fit on and 256 to
# validate on, 60 steps of 64 rows through the reference's schedule (an "epoch" every 4 steps, so that the warm-up is crossed).
FIT = dict(classes=8, D=16, train=256, val=256, noise=0.35, steps=60, batch=64, lr=2e-2, seed=5, steps_per_epoch=4)


def unit(x):
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), 1e-12)


def fit_data():
    """(train x, train labels, val x, val labels, initial w, [rows] per step): host arrays, all fixed by the seed."""
    f = FIT
    rng = np.random.default_rng(f["seed"])
    centres = unit(rng.standard_normal((f["classes"], f["D"])))

    def draw(n):
        y = rng.integers(0, f["classes"], n)
        return unit(centres[y] + rng.standard_normal((n, f["D"])) * f["noise"]).astype(F32), y.astype(np.int32)
    xt, yt = draw(f["train"])
    xv, yv = draw(f["val"])
    w0 = (rng.standard_normal((f["classes"], f["D"])) * np.sqrt(4.0 / (f["classes"] + f["D"]))).astype(F32)
    steps = [rng.permutation(f["train"])[:f["batch"]].astype(np.int32) for _ in range(f["steps"])]
    return xt, yt, xv, yv, w0, steps


def cosine_accuracy(w, x, y):
    """The share of rows of `x` whose largest cosine with a row of `w` is their label's (float64, host)."""
    return float((np.argmax(unit(x) @ unit(w).T, axis=1) == np.asarray(y)).mean())
