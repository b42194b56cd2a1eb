"""The shape tables and the inputs of the pair head-fitting tests (`test_head_fit_pair_cpu.py`, `test_head_fit_pair_gpu.py`) and of
tools/head_fit_pair_check.cpp, which carries the same CPU table.

Shapes are (P, D, E).  The batch has 2P rows: it crosses the 32-row tile between P = 16 and 17; E crosses the tile at 32 / 33 and the
wavefront at 64 / 65; D crosses the tile and the 128 chain.  The GPU table adds a many-workgroup step, and E at the pair kernel's
register limit (`REG_E`, HF_PAIR_REG_E of csrc/head_fit_pair.hip) and one above it.

Every case runs `STEPS` steps with `lr` changing per step, in two variations that between them cover Adam / AdamW, AMSGrad, and a step
with and without a dropout mask.  A case with P >= 4 contains a pair with ``left == right`` (pair 2; `differ` 1, so that the loss
pushes a pair of distance ~0), a cache row used by several pairs (pairs 0 and 1 share their left row) and both values of `differ`;
a case with P = 1 is one ordinary pair, `differ` = 0 in the first variation and 1 in the second - one pair cannot hold all three.

MARGIN and ACCEPT are chosen away from the distances small shapes can only take (E = 1: u, v = +-1, so d is 1e-6 or 2 + 1e-6 - the
reference's margin 2.0 would sit on it): `assert_no_knife_edge` refuses a pair whose float64 distance is within 1e-4 of either."""
import numpy as np

F32 = np.float32
CPU_SHAPES = ((1, 1, 1), (1, 3, 2), (16, 64, 32), (17, 65, 33), (31, 128, 63), (32, 129, 64), (33, 512, 65), (64, 512, 256))
REG_E = 512
GPU_SHAPES = CPU_SHAPES + ((512, 512, 256), (9, 40, REG_E), (9, 40, REG_E + 1))
STEPS = 3
LRS = (1e-2, 5e-3, 2e-2)
KEEP_P = 0.25
MARGIN, ACCEPT, W_SAME, W_DIFF = 1.2, 0.9, 0.8, 1.2
EDGE = 1e-4
LOSS_F32 = tuple(float(F32(v)) for v in (MARGIN, W_SAME, W_DIFF))        # what the library computes with: it takes them as fp32
VARIATIONS = (
    {"name": "adam-mask", "keep": True, "decoupled": False, "amsgrad": False, "weight_decay": 1e-2},
    {"name": "adamw-ams", "keep": False, "decoupled": True, "amsgrad": True, "weight_decay": 1e-2},
)
BAD_KINDS = ("left -1", "right N", "nan feature", "inf feature", "differ 2", "differ -1")


def cases(shapes=CPU_SHAPES):
    return [(shape, var) for shape in shapes for var in VARIATIONS]


# A seed whose problem puts a pair within EDGE of ACCEPT or MARGIN at one of its three steps is moved on by 100 (`assert_no_knife_edge`
# finds them; `test_head_fit_pair_cpu.py` walks every CPU and GPU case with the twin): (shape, variation name) -> the seed's offset.
RESEED = {((64, 512, 256), "adamw-ams"): 100}


def case_seed(case):
    """The seed of a case of the contract tests: the same problem on the CPU and on the GPU."""
    shape, var = case
    return 1000 + 2 * GPU_SHAPES.index(shape) + VARIATIONS.index(var) + RESEED.get((shape, var["name"]), 0)


def case_id(case):
    return "P%d-D%d-E%d-%s" % (*case[0], case[1]["name"])


def step_kw(var, s, clear=None):
    """The keyword arguments of step `s` of a variation, for `pair_step`, `pair_step_host` and `pair_step_rule` alike."""
    return dict(lr=LRS[s % len(LRS)], weight_decay=var["weight_decay"], decoupled=var["decoupled"], amsgrad=var["amsgrad"],
                margin=MARGIN, accept=ACCEPT, w_same=W_SAME, w_diff=W_DIFF, clear=(s == 0) if clear is None else clear)


def keep_scale(var):
    return 1.0 / (1.0 - KEEP_P) if var["keep"] else 1.0


def assert_no_knife_edge(dist, what=""):
    """No counted pair's distance (float64) within `EDGE` of ACCEPT or MARGIN: the figures and the clamp must not hang on a last bit."""
    d = np.asarray(dist, np.float64)
    d = d[np.isfinite(d)]
    gap = float(np.minimum(np.abs(d - ACCEPT), np.abs(d - MARGIN)).min()) if d.size else float("inf")
    assert gap >= EDGE, (what, "a pair's distance is within %g of accept or margin" % EDGE, gap)
    return gap


def problem(seed, P, D, E, var):
    """A dict of host arrays: x [N, D], left, right, differ [P], w [E, D], b [E], keep [2P, D] or None.  Features are multiples of 1/64
    in [-1, 1], weights zero-mean normal draws of nn.Linear's scale (the module docstring says what every case contains)."""
    rng = np.random.default_rng(seed)
    N = P + 5
    x = (rng.integers(-64, 65, (N, D)) / 64.0).astype(F32)
    x[np.abs(x).sum(axis=1) == 0, 0] = 0.5                        # (no all-zero row by chance: the zero-norm branch has its own test)
    left = rng.integers(0, N, P).astype(np.int32)
    right = ((left + 1 + rng.integers(0, N - 1, P)) % N).astype(np.int32)        # (never the left row)
    differ = rng.integers(0, 2, P).astype(np.int32)
    if P >= 4:
        left[1] = left[0]
        right[2] = left[2]
        differ[:4] = (0, 1, 1, 0)
    else:
        differ[0] = VARIATIONS.index(var) if var in VARIATIONS else 0
    w = (rng.standard_normal((E, D)) / np.sqrt(D)).astype(F32)
    b = (rng.standard_normal(E) * 0.05).astype(F32)
    keep = (rng.random((2 * P, D)) >= KEEP_P).astype(np.uint8) if var["keep"] else None
    if keep is not None:
        keep[:, 0] = 1                                            # (a masked row keeps at least one feature)
    return {"x": x, "left": left, "right": right, "differ": differ, "w": w, "b": b, "keep": keep, "P": P, "D": D, "E": E, "N": N}


def with_bad_pair(p, kind, at):
    """The problem with one more pair INSERTED before pair `at`, bad in the way `kind` says (`BAD_KINDS`); its mask rows are ones.
    The cache gains a row for the non-finite kinds, so that no other pair reads the spoiled row."""
    q = dict(p)
    x = np.concatenate([p["x"], p["x"][:1]])
    N = len(x)
    l, r, d = int(p["left"][0]), int(p["right"][0]), 0
    if kind == "left -1":
        l = -1
    elif kind == "right N":
        r = N
    elif kind == "nan feature":
        x[N - 1, p["D"] // 2] = np.nan
        l = N - 1
    elif kind == "inf feature":
        x[N - 1, 0] = -np.inf
        r = N - 1
    elif kind == "differ 2":
        d = 2
    elif kind == "differ -1":
        d = -1
    else:
        raise KeyError(kind)
    P = p["P"]
    q["x"], q["N"], q["P"] = x, N, P + 1
    q["left"] = np.insert(p["left"], at, l).astype(np.int32)
    q["right"] = np.insert(p["right"], at, r).astype(np.int32)
    q["differ"] = np.insert(p["differ"], at, d).astype(np.int32)
    if p["keep"] is not None:
        one = np.ones((1, p["D"]), np.uint8)
        q["keep"] = np.concatenate([p["keep"][:at], one, p["keep"][at:P], p["keep"][P:P + at], one, p["keep"][P + at:]])
    return q


# The synthetic fit: 8 classes whose signal lives in 4 of 32 dimensions under noise 0.3; the other 28 are unrelated noise of amplitude 3,
# so raw distances say little and a learned projection has to find the 4.
FIT = dict(classes=8, D=32, E=8, train=256, val=256, signal=4, noise=0.3, clutter=3.0, steps=300, pairs=64, lr=1e-2, seed=3)


def fit_data(seed=None):
    """(train x, train labels, val x, val labels, [(left, right, differ)] per step): host arrays, pair lists fixed by the seed."""
    f = FIT
    rng = np.random.default_rng(f["seed"] if seed is None else seed)
    centres = rng.standard_normal((f["classes"], f["signal"]))

    def draw(n):
        y = rng.integers(0, f["classes"], n)
        x = rng.standard_normal((n, f["D"])) * f["clutter"]
        x[:, :f["signal"]] = centres[y] + rng.standard_normal((n, f["signal"])) * f["noise"]
        return x.astype(F32), y.astype(np.int32)
    xt, yt = draw(f["train"])
    xv, yv = draw(f["val"])
    by_class = [np.flatnonzero(yt == c) for c in range(f["classes"])]
    steps = []
    for _ in range(f["steps"]):
        left = rng.integers(0, f["train"], f["pairs"])
        right = np.empty_like(left)
        for k, a in enumerate(left):
            same = by_class[yt[a]]
            same = same[same != a]
            if rng.random() < 0.5 and len(same):
                right[k] = rng.choice(same)
            else:
                right[k] = rng.choice(np.flatnonzero(yt != yt[a]))
        steps.append((left.astype(np.int32), right.astype(np.int32), (yt[left] != yt[right]).astype(np.int32)))
    return xt, yt, xv, yv, steps


def eer(emb, labels):
    """The equal error rate of all unordered pairs of rows of `emb` by Euclidean distance (float64, host)."""
    e = np.asarray(emb, np.float64)
    iu = np.triu_indices(len(e), 1)
    d = np.sqrt(((e[iu[0]] - e[iu[1]]) ** 2).sum(axis=1))
    genuine = np.asarray(labels)[iu[0]] == np.asarray(labels)[iu[1]]
    order = np.argsort(d, kind="stable")
    g = genuine[order]
    far = np.cumsum(~g) / max(int((~g).sum()), 1)                 # impostors accepted at each threshold
    frr = 1.0 - np.cumsum(g) / max(int(g.sum()), 1)               # genuines rejected
    k = int(np.argmin(np.abs(far - frr)))
    return float((far[k] + frr[k]) / 2)


def unit(x):
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), 1e-12)
