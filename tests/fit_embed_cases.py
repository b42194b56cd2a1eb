"""The shape table and the inputs of the embedding head-fitting tests (`test_head_fit_embed_cpu.py`, `test_head_fit_embed_gpu.py`) and of
tools/head_fit_embed_check.cpp, which walks a part of the same table.

Shapes are (B, D, E, C): the smallest that cross every boundary - the 32-wide tile and the 128-long chain - in each of the four
extents; each extent takes 2 or 3, 31, 32, 33 and 129 somewhere, and C = 1 and E = 1 are in.  Every case runs `STEPS` steps with `lr`,
the effective scale and margin, the easy margin and the label smoothing changing per step (`step_kw`), in a variation chosen by the
shape's index, so that the table covers Adam / AdamW, AMSGrad and a step with and without a dropout mask behind the BatchNorm.

KNIFE EDGES.  The margin stage has the comparisons `fit_margin_cases` lists; `assert_no_knife_edge` there is applied to the margin
stage of every step of every table, in float64, and `assert_norms` holds every counted row's ``|y'|`` above `MIN_NORM`, far from the
1e-12 clamp of the normalisation.  E = 1 saturates by construction (a one-dimensional row is parallel to every centre); E = 2 appears only with few rows or few centres -
in the plane dozens of rows against dozens of centres come within 1e-5 of parallel."""
import numpy as np

import fit_margin_cases as mc

F32 = np.float32
SHAPES = (
    (3, 3, 3, 3), (2, 31, 33, 2), (31, 32, 31, 32), (32, 33, 32, 31), (33, 31, 1, 33), (33, 3, 33, 1), (129, 3, 3, 3), (3, 129, 3, 2),
    (2, 3, 129, 3), (3, 2, 3, 129), (31, 33, 32, 18), (32, 31, 33, 33), (33, 32, 31, 31), (65, 5, 31, 32), (5, 65, 32, 33), (31, 4, 33, 31),
    (129, 33, 31, 2), (33, 129, 3, 31), (32, 2, 129, 32), (31, 3, 32, 129), (130, 5, 5, 5), (257, 3, 4, 3),
)
BIG_SHAPES = ((32, 512, 512, 18), (256, 512, 512, 1000))          # one step each, on the GPU
ALL_SHAPES = SHAPES + BIG_SHAPES
STEPS = 3
LRS, SCALES, MARGINS, KEEP_P = mc.LRS, mc.SCALES, mc.MARGINS, mc.KEEP_P
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
MIN_NORM = 1e-3
VARIATIONS = mc.VARIATIONS
RESEED = {}


def variation(shape):
    return VARIATIONS[ALL_SHAPES.index(shape) % 2]


def case_seed(shape):
    return 7000 + ALL_SHAPES.index(shape) + RESEED.get(shape, 0)


def case_id(shape):
    return "B%d-D%d-E%d-C%d" % shape


def step_kw(var, k, clear=None):
    """The keyword arguments of step `k` of a variation, for `embed_step`, `embed_step_host` and `embed_step_rule` alike."""
    kw = mc.step_kw(var, k, clear)
    kw.update(bn_eps=BN_EPS, bn_momentum=BN_MOMENTUM)
    return kw


def keep_scale(var):
    return mc.keep_scale(var)


PARAMS = ("w1", "gamma", "beta", "running_mean", "running_var", "wc")


def problem(seed, B, D, E, C, var):
    """A dict of host arrays: x [N, D], labels [N], rows [B] (a draw without repeats from the N = B + 3 cached rows), w1 [E, D], gamma,
    beta, running_mean, running_var [E], wc [C, E], keep [B, E] or None (column 0 is kept, so that no row of y' is all zeros).  Features
    are multiples of 1/64 in [-1, 1]; large batches lean towards their class (as `fit_margin_cases.problem` explains)."""
    rng = np.random.default_rng(seed)
    N = B + 3
    x = (rng.integers(-64, 65, (N, D)) / 64.0).astype(F32)
    labels = rng.integers(0, C, N).astype(np.int32)
    rows = rng.permutation(N)[:B].astype(np.int32)
    w1 = (rng.standard_normal((E, D)) / np.sqrt(D)).astype(F32)
    gamma = (1.0 + 0.1 * rng.standard_normal(E)).astype(F32)
    beta = (0.1 * rng.standard_normal(E)).astype(F32)
    running_mean = (0.1 * rng.standard_normal(E)).astype(F32)
    running_var = (1.0 + 0.1 * np.abs(rng.standard_normal(E))).astype(F32)
    wc = (rng.standard_normal((C, E)) * np.sqrt(4.0 / (C + E))).astype(F32)
    if B >= 256:
        # lean the features so that the embedding of a row leans towards its class centre: x += c (wc[label] w1^+), roughly
        pinv = np.linalg.pinv(w1.astype(np.float64))                   # [D, E]
        lean = wc[labels].astype(np.float64) @ pinv.T
        lean /= np.maximum(np.sqrt((lean ** 2).sum(axis=1, keepdims=True)), 1e-9)
        x = (np.round((x + 0.6 * np.sqrt(D / 3.0) * lean) * 64.0) / 64.0).astype(F32)
    keep = (rng.random((B, E)) >= KEEP_P).astype(np.uint8) if var["keep"] else None
    if keep is not None:
        keep[:, 0] = 1
    return {"x": x, "labels": labels, "rows": rows, "w1": w1, "gamma": gamma, "beta": beta, "running_mean": running_mean,
            "running_var": running_var, "wc": wc, "keep": keep, "B": B, "D": D, "E": E, "C": C, "N": N}


def params_of(p, dtype=F32):
    return {k: np.array(p[k], dtype) for k in PARAMS}


def assert_norms(rule_out, what=""):
    """Every row the margin stage counts has ``|y'|`` well above the 1e-12 clamp of the normalisation.  Returns the smallest."""
    ok = rule_out["margin"]["ok"]
    if not ok.any():
        return float("inf")
    nrm = np.sqrt((np.asarray(rule_out["yp"], np.float64)[ok] ** 2).sum(axis=1))
    assert nrm.min() > MIN_NORM, (what, "a row of y' has a norm near the clamp of the normalisation", float(nrm.min()))
    return float(nrm.min())


def with_bad_row(p, kind, at):
    """`fit_margin_cases.with_bad_row` for an embedding problem: the inserted mask row is [1, E] ones."""
    q = mc.with_bad_row({**p, "keep": None}, kind, at)
    q["keep"] = None if p["keep"] is None else np.concatenate([p["keep"][:at], np.ones((1, p["E"]), np.uint8), p["keep"][at:]])
    return q


# The synthetic fit: 8 classes of clustered vectors in 12 pooled dimensions behind a random 12 -> 16 embedding; 256 rows to fit on and
# 256 to validate on, 60 steps of 64 rows through the reference's schedule (an "epoch" every 4 steps).
FIT = dict(classes=8, D=12, E=16, train=256, val=256, noise=0.25, steps=60, batch=64, lr=2e-2, seed=11, steps_per_epoch=4)


def fit_data():
    """(train x, train labels, val x, val labels, initial parameters, [rows] per step): host arrays, all fixed by the seed."""
    f = FIT
    rng = np.random.default_rng(f["seed"])
    centres = mc.unit(rng.standard_normal((f["classes"], f["D"])))

    def draw(n):
        y = rng.integers(0, f["classes"], n)
        return (centres[y] + rng.standard_normal((n, f["D"])) * f["noise"]).astype(F32), y.astype(np.int32)
    xt, yt = draw(f["train"])
    xv, yv = draw(f["val"])
    E, D, C = f["E"], f["D"], f["classes"]
    p0 = {"w1": (rng.standard_normal((E, D)) / np.sqrt(D)).astype(F32), "gamma": np.ones(E, F32), "beta": np.zeros(E, F32),
          "running_mean": np.zeros(E, F32), "running_var": np.ones(E, F32),
          "wc": (rng.standard_normal((C, E)) * np.sqrt(4.0 / (C + E))).astype(F32)}
    steps = [rng.permutation(f["train"])[:f["batch"]].astype(np.int32) for _ in range(f["steps"])]
    return xt, yt, xv, yv, p0, steps


def deployed_embedding(p, x, eps=BN_EPS):
    """``normalize(bn_eval(x w1^T))`` with the running statistics, float64 on the host."""
    p = {k: np.asarray(v, np.float64) for k, v in p.items()}
    a = np.asarray(x, np.float64) @ p["w1"].T
    return mc.unit((a - p["running_mean"]) / np.sqrt(p["running_var"] + eps) * p["gamma"] + p["beta"])


def deployed_accuracy(p, x, y):
    return float((np.argmax(deployed_embedding(p, x) @ mc.unit(p["wc"]).T, axis=1) == np.asarray(y)).mean())
