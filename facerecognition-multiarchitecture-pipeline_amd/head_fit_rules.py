"""The specification of head fitting: every step of `head_fit` in numpy, in float64 (the formulas as torch evaluates them, which the
tests check against torch) and in float32 in the order of csrc/head_fit_rule.h (what the kernels and the host twin compute, word for
word).  Every test measures the kernels and the twin against these functions, so they touch neither torch nor the library: this module
imports `math` and `numpy` and nothing else.  `head_fit` re-exports every name; its docstring says what each step is.  `fma32`, `dot32`,
`adam_scalars32` and `adam32` are the float32 arithmetic; `_rule_batch` (declined rows, the masked input) and `_adam_rule` are shared
by the rules, one step of a family each; `margin_schedule` is the host arithmetic of the ArcFace warm-up."""
from __future__ import annotations

import math

import numpy as np

CHAIN = 128                       # FRMAP_HEAD_FIT_CHAIN: where the dot products are cut
LOSS_CLAMP, LOSS_SCALE = 65536.0, 16777216.0         # the tally's fixed point (csrc/tally_rule.h)
F32 = np.float32
NORM_EPS, DIST_EPS, DIST_MIN = 1e-12, 1e-6, 1e-8      # F.normalize, F.pairwise_distance, the loss's clamp
MARGIN_HI = float(F32(1.0 - 1e-7))                 # the clamp bound of the cosine as the library holds it (fp32)
MARGIN_CAP = float(F32(math.pi - 1e-4))            # the reference's torch.tensor(math.pi - 1e-4): a float32 in every dtype
MARGIN_RMAX = F32(1.0 / 1e-12)                     # the fp32 reciprocal of a clamped norm


def fma32(a, b, c):
    """fmaf on float32 arrays, correctly rounded: the product of two float32 is exact in float64; the float64 sum is rounded TO ODD
    (the error of the addition, exact by TwoSum, decides the last bit), and a round-to-odd value of 53 bits rounds to the right 24."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = s.view(np.int64).copy()
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((bits & 1) == 0)
        away = (err > 0) == (s > 0)                     # the exact sum lies further from zero than s
        bits = np.where(fix, bits + np.where(away, 1, -1), bits)
        return bits.view(np.float64).astype(F32)


def dot32(a, b):
    """The rule's dot product over the LAST axis of float32 arrays ``a`` and ``b`` (broadcast against each other): chains of `fma32`
    from +0 cut at the multiples of `CHAIN`, the chains added in ascending order from +0."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    K = a.shape[-1]
    shape = np.broadcast_shapes(a.shape[:-1], b.shape[:-1])
    s = np.zeros(shape, F32)
    for k0 in range(0, K, CHAIN):
        c = np.zeros(shape, F32)
        for k in range(k0, min(k0 + CHAIN, K)):
            c = fma32(a[..., k], b[..., k], c)
        s = s + c
    return s


def _powi(base: float, t: int) -> float:
    r, p = 1.0, float(base)
    while t:
        if t & 1:
            r = r * p
        p = p * p
        t >>= 1
    return r


def adam_scalars32(t: int, lr, beta1, beta2, eps, weight_decay) -> dict:
    """The per-step scalars of `frmap_head_fit_adam_scalars`: beta^t by squarings in float64, everything else float32."""
    lr, beta1, beta2, eps, wd = (F32(v) for v in (lr, beta1, beta2, eps, weight_decay))
    bc1 = F32(1.0 - _powi(float(beta1), t))
    bc2 = F32(1.0 - _powi(float(beta2), t))
    return {"step_size": F32(lr / bc1), "bc2_sqrt": np.sqrt(bc2), "omb1": F32(F32(1) - beta1), "omb2": F32(F32(1) - beta2), "beta2": beta2,
            "eps": eps, "wd": wd, "decay": F32(F32(1) - F32(lr * wd))}


def adam32(a: dict, grad, p, m, v, vmax, decoupled: bool, amsgrad: bool):
    """`frmap_head_fit_adam` on float32 arrays; returns ``(p, m, v, vmax)``."""
    grad, p, m, v = (np.asarray(t, F32) for t in (grad, p, m, v))
    with np.errstate(all="ignore"):
        if decoupled:
            p = p * a["decay"]
        elif a["wd"] != 0:
            grad = fma32(a["wd"], p, grad)
        m = fma32(a["omb1"], grad - m, m)
        v = fma32(a["omb2"], grad * grad, v * a["beta2"])
        vhat = v
        if amsgrad:
            vmax = np.where(vmax > v, vmax, v).astype(F32)
            vhat = vmax
        u = m / (np.sqrt(vhat) / a["bc2_sqrt"] + a["eps"])
        p = fma32(-a["step_size"], u, p)
    return p.astype(F32), m.astype(F32), v.astype(F32), vmax


def fresh_state(D: int, C: int, amsgrad: bool = False, dtype=np.float64) -> dict:
    """An optimiser state of the rule: the header integers and zero moments of ``dtype``."""
    st = {"t": 0, "n": 0, "rows": 0, "correct": 0, "loss_q": 0, "m_w": np.zeros((C, D), dtype), "v_w": np.zeros((C, D), dtype),
          "m_b": np.zeros((C,), dtype), "v_b": np.zeros((C,), dtype)}
    if amsgrad:
        st["vmax_w"], st["vmax_b"] = np.zeros((C, D), dtype), np.zeros((C,), dtype)
    return st


def loss_q(row_loss) -> int:
    """The tally's fixed point of float32 row losses, summed: llrint(min(loss, 65536) * 2^24), a NaN taken at the clamp."""
    l = np.asarray(row_loss, F32).astype(np.float64)
    l = np.where(l < LOSS_CLAMP, l, LOSS_CLAMP)
    return int(np.rint(l * LOSS_SCALE).astype(np.uint64).sum(dtype=np.uint64))


def _copy_state(st: dict, dtype) -> dict:
    """A rule state with its moments copied as ``dtype`` and its header words as ints."""
    return {k: (np.array(v, dtype) if isinstance(v, np.ndarray) else int(v)) for k, v in st.items()}


def _adam_rule(p, grad, st: dict, which: str, t: int, lr, beta1, beta2, eps, weight_decay, decoupled, amsgrad, f32):
    """The update of the rule on one tensor (``which``: "w" or "b", the suffix of its moments in ``st``): `adam32` in float32 mode,
    the formulas as torch evaluates them in float64.  Returns the new parameter; ``st`` is updated in place."""
    km, kv, kx = "m_" + which, "v_" + which, "vmax_" + which
    if f32:
        a = adam_scalars32(t, lr, beta1, beta2, eps, weight_decay)
        p, st[km], st[kv], vm = adam32(a, grad, p, st[km], st[kv], st.get(kx), decoupled, amsgrad)
        if amsgrad:
            st[kx] = vm
        return p
    p = np.array(p, np.float64)
    if decoupled:
        p *= 1.0 - lr * weight_decay
    elif weight_decay != 0:
        grad = grad + weight_decay * p
    st[km] = st[km] + (1.0 - beta1) * (grad - st[km])
    st[kv] = st[kv] * beta2 + (1.0 - beta2) * grad * grad
    vhat = st[kv]
    if amsgrad:
        st[kx] = np.maximum(st[kx], st[kv])
        vhat = st[kx]
    denom = np.sqrt(vhat) / math.sqrt(1.0 - beta2 ** t) + eps
    p += -(lr / (1.0 - beta1 ** t)) * (st[km] / denom)
    return p


def _rule_batch(x, labels, C: int, rows, B: int, keep, keep_scale, f32: bool):
    """``(row_src, ok, x')`` of a batch of the rule: ``rows`` (``None``: rows ``0 .. B-1``) with -1 where a row is declined - outside
    the cache, a label outside ``[0, C)``, a non-finite feature -, that as a mask, and the ``[B, D]`` input with ``keep`` applied and
    scaled (a declined row is zeros)."""
    N, D = x.shape
    rows = np.arange(B, dtype=np.int64) if rows is None else np.asarray(rows).astype(np.int64)
    row_src = np.full((len(rows),), -1, np.int32)
    for i, r in enumerate(rows):
        if 0 <= r < N and 0 <= labels[r] < C and np.isfinite(x[r]).all():
            row_src[i] = r
    ok = row_src >= 0
    xp = np.zeros((len(rows), D), x.dtype)
    xp[ok] = x[row_src[ok]]
    if keep is not None:
        kept = np.asarray(keep).astype(bool)
        scaled = (xp * F32(keep_scale)).astype(F32) if f32 else xp * float(keep_scale)
        xp = np.where(kept, scaled, 0).astype(x.dtype)
        xp[~ok] = 0
    return row_src, ok, xp


def step_rule(x, labels, w, b, state: dict | None = None, rows=None, keep=None, keep_scale: float = 1.0, *, lr: float = 1e-3,
              beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0, label_smoothing: float = 0.0,
              decoupled: bool = False, amsgrad: bool = False, clear: bool = False, dtype=np.float64, given: dict | None = None,
              batch: int | None = None) -> dict:
    """One training step, the specification (module docstring; the formulas are those of include/frmap_hip.h, "Head fitting").

    ``dtype=np.float64``: the formulas in float64, as torch evaluates them (``nn.Linear`` + ``F.cross_entropy`` + ``optim.Adam`` /
    ``AdamW``).  ``dtype=np.float32``: every operation float32 in the order of csrc/head_fit_rule.h - `dot32` for both GEMMs, `adam32` for the
    update; the softmax, the row loss and g in float64 from the float32 logits and rounded once - which is what the host twin
    computes bit for bit (up to a rare last bit of g and the loss where the C library's exp / log and numpy's differ).  ``given``: ``{"z", "g", "row_loss"}`` to take as they are (float32 mode: the device's or the twin's own)
    instead of computing them, the way `frmap_head_fit_step_host` takes them with ``given_g``.

    ``batch``: the number of batch rows B when neither ``rows`` nor ``keep`` gives it (default: the whole cache).

    Nothing is modified: returns ``{"w", "b", "state", "z", "g", "row_loss", "row_src", "dw", "db", "n", "loss"}`` with new arrays;
    ``loss`` is the mean row loss of the counted rows (NaN when all are declined)."""
    f32 = np.dtype(dtype) == np.dtype(np.float32)
    x = np.asarray(x, F32 if f32 else np.float64)
    w, b = np.array(w, dtype), np.array(b, dtype)
    labels = np.asarray(labels).astype(np.int64)
    N, D = x.shape
    C = w.shape[0]
    st = _copy_state(state or fresh_state(D, C, amsgrad, dtype), dtype)
    if clear:
        st["rows"] = st["correct"] = st["loss_q"] = 0
    # rows 0 .. B-1 without `rows`: B is the mask's, else `batch`, else the whole cache
    row_src, ok, xp = _rule_batch(x, labels, C, rows, len(keep) if keep is not None else (N if batch is None else int(batch)), keep,
                                  keep_scale, f32)
    B = len(row_src)
    n = int(ok.sum())
    st["n"] = n
    y = np.where(ok, labels[np.clip(row_src, 0, N - 1)], 0)
    ls = F32(label_smoothing) if f32 else float(label_smoothing)
    with np.errstate(all="ignore"):
        if given is not None:
            z, g, row_loss = (np.array(given[k], dtype) for k in ("z", "g", "row_loss"))
        else:
            z = (dot32(xp[:, None, :], w[None, :, :]) + b[None, :]).astype(F32) if f32 else xp @ w.T + b[None, :]
            z[~ok] = 0
            # the softmax half is float64 in both modes (csrc/head_fit_rule.h): the float32 mode rounds g and the loss once
            z64 = z.astype(np.float64)
            m = z64.max(axis=1, keepdims=True)
            e = np.exp(z64 - m)
            s = e.sum(axis=1, keepdims=True)
            nl = np.log(s) - (z64 - m)                               # -log p, per class
            nll = nl[np.arange(B), y]
            ls64, off64 = float(ls), (float(ls) / C if ls > 0 else 0.0)
            row_loss = (1.0 - ls64) * nll + off64 * nl.sum(axis=1) if ls > 0 else nll
            row_loss = np.where(row_loss > 0, row_loss, np.where(np.isnan(row_loss), row_loss, 0)).astype(dtype)
            t64 = np.full((B, C), off64)
            t64[np.arange(B), y] = (1.0 - ls64) + off64
            g = (((e / s) - t64) / float(max(n, 1))).astype(dtype)
            g[~ok] = 0
            row_loss[~ok] = np.nan
    pred = z.argmax(axis=1)
    st["rows"] += n
    st["correct"] += int((ok & (pred == y)).sum())
    st["loss_q"] += loss_q(row_loss[ok])
    out = {"z": z, "g": g, "row_loss": row_loss, "row_src": row_src, "n": n,
           "loss": float(row_loss[ok].astype(np.float64).mean()) if n else float("nan")}
    gz = np.where(ok[:, None], g, 0).astype(dtype)
    if f32:
        dw = dot32(gz.T[:, None, :], xp.T[None, :, :])
        db = dot32(gz.T, np.ones((1, B), F32))
    else:
        dw, db = gz.T @ xp, gz.sum(axis=0)
    out["dw"], out["db"] = dw, db
    if n:
        st["t"] += 1
        kw = dict(t=st["t"], lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, decoupled=decoupled, amsgrad=amsgrad,
                  f32=f32)
        w, b = _adam_rule(w, dw, st, "w", **kw), _adam_rule(b, db, st, "b", **kw)
    out["w"], out["b"], out["state"] = w, b, st
    return out


def group_step_rule(x, labels, w, b, states, rows, keep=None, *, hyper, decoupled: bool = False, amsgrad: bool = False, clear: bool = False,
                    evaluate: bool = False, dtype=np.float64, given=None) -> list:
    """The grouped step in numpy: ``H`` calls of `step_rule`, head ``h`` on ``w[h]``, ``b[h]``, ``states[h]`` (a rule state or
    ``None``), ``rows[h]``, ``keep[h]`` and row ``h`` of ``hyper`` (`hyper_table`).  ``evaluate``: the weights, the moments and ``t``
    of the returned dicts are the inputs'; only ``n`` and the figures are the step's.  Returns the list of `step_rule` results."""
    hyper = np.asarray(hyper, np.float32)
    H = len(w)
    if hyper.shape != (H, 8) or len(rows) != H:
        raise ValueError(f"head_fit.group_step_rule: hyper [{H}, 8] and rows [{H}, B] expected")
    out = []
    for h in range(H):
        hy = hyper[h]
        st = None if states is None else states[h]
        r = step_rule(x, labels, w[h], b[h], st, rows[h], None if keep is None else keep[h], float(hy[6]), lr=float(hy[0]),
                      beta1=float(hy[1]), beta2=float(hy[2]), eps=float(hy[3]), weight_decay=float(hy[4]), label_smoothing=float(hy[5]),
                      decoupled=decoupled, amsgrad=amsgrad, clear=clear, dtype=dtype, given=None if given is None else given[h])
        if evaluate:
            D, C = np.asarray(w[h]).shape[1], np.asarray(w[h]).shape[0]
            old = _copy_state(st or fresh_state(D, C, amsgrad, dtype), dtype)
            for k in ("n", "rows", "correct", "loss_q"):
                old[k] = r["state"][k]
            r["w"], r["b"], r["state"] = np.array(w[h], dtype), np.array(b[h], dtype), old
        out.append(r)
    return out


def hidden_step_rule(x, labels, w1, b1, w2, b2, state: dict | None = None, rows=None, keep1=None, keep1_scale: float = 1.0, keep2=None,
                     keep2_scale: float = 1.0, *, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                     weight_decay: float = 0.0, label_smoothing: float = 0.0, decoupled: bool = False, amsgrad: bool = False,
                     clear: bool = False, dtype=np.float64, given: dict | None = None, batch: int | None = None) -> dict:
    """One training step of Linear(D, Hd) -> ReLU -> dropout -> Linear(Hd, C), the specification (csrc/head_fit_rule.h, HIDDEN LAYER).

    Layer 1's forward and its declined rows are computed here; all of layer 2 is `step_rule` on ``(h, lab, keep2)``; ``da`` is formed
    against the ``w2`` from BEFORE that update, and layer 1's update uses layer 2's ``t`` and ``n``.  ``dtype`` and ``given`` as in
    `step_rule` (``given`` holds layer 2's ``z``, ``g`` and ``row_loss``).  ``state``: ``{"layer1": ..., "layer2": ...}`` of
    `fresh_state` dicts for (D, Hd) and (Hd, C), or ``None``.

    Nothing is modified: returns ``{"w1", "b1", "w2", "b2", "state", "h", "lab", "row_src1", "da", "z", "g", "row_loss", "row_src",
    "dw1", "db1", "dw2", "db2", "n", "loss"}`` with new arrays."""
    f32 = np.dtype(dtype) == np.dtype(np.float32)
    x = np.asarray(x, F32 if f32 else np.float64)
    w1, b1 = np.array(w1, dtype), np.array(b1, dtype)
    w2_old = np.array(w2, dtype)
    labels = np.asarray(labels).astype(np.int64)
    N, D = x.shape
    Hd, C = w1.shape[0], w2_old.shape[0]
    state = state or {"layer1": fresh_state(D, Hd, amsgrad, dtype), "layer2": fresh_state(Hd, C, amsgrad, dtype)}
    st1 = _copy_state(state["layer1"], dtype)
    masks = [len(k) for k in (keep1, keep2) if k is not None]
    row_src1, ok1, xp = _rule_batch(x, labels, C, rows, masks[0] if masks else (N if batch is None else int(batch)), keep1, keep1_scale, f32)
    B = len(row_src1)
    lab = np.where(ok1, labels[np.clip(row_src1, 0, N - 1)], -1).astype(np.int32)
    with np.errstate(all="ignore"):
        a = (dot32(xp[:, None, :], w1[None, :, :]) + b1[None, :]).astype(F32) if f32 else xp @ w1.T + b1[None, :]
        h = np.where(a > 0, a, np.where(np.isnan(a), a, 0)).astype(dtype)
    h[~ok1] = 0
    r2 = step_rule(h, lab, w2_old, b2, state["layer2"], None, keep2, keep2_scale, lr=lr, beta1=beta1, beta2=beta2, eps=eps,
                   weight_decay=weight_decay, label_smoothing=label_smoothing, decoupled=decoupled, amsgrad=amsgrad, clear=clear,
                   dtype=dtype, given=given, batch=B)
    ok2 = r2["row_src"] >= 0
    g = np.where(ok2[:, None], r2["g"], 0).astype(dtype)
    with np.errstate(all="ignore"):
        s = dot32(g[:, None, :], w2_old.T[None, :, :]) if f32 else g @ w2_old
        live = ok2[:, None] & (h > 0)
        if keep2 is not None:
            live = live & np.asarray(keep2).astype(bool)
            s = (s * F32(keep2_scale)).astype(F32) if f32 else s * float(keep2_scale)
        da = np.where(live, s, 0).astype(dtype)
        dz = np.where(ok1[:, None], da, 0).astype(dtype)
        if f32:
            dw1 = dot32(dz.T[:, None, :], xp.T[None, :, :])
            db1 = dot32(dz.T, np.ones((1, B), F32))
        else:
            dw1, db1 = dz.T @ xp, dz.sum(axis=0)
    n = r2["n"]
    st1["t"], st1["n"] = r2["state"]["t"], n
    if n:
        kw = dict(t=st1["t"], lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, decoupled=decoupled, amsgrad=amsgrad,
                  f32=f32)
        w1, b1 = _adam_rule(w1, dw1, st1, "w", **kw), _adam_rule(b1, db1, st1, "b", **kw)
    out = {"w1": w1, "b1": b1, "w2": r2["w"], "b2": r2["b"], "state": {"layer1": st1, "layer2": r2["state"]}, "h": h, "lab": lab,
           "row_src1": row_src1, "da": da, "dw1": dw1, "db1": db1, "dw2": r2["dw"], "db2": r2["db"]}
    for k in ("z", "g", "row_loss", "row_src", "n", "loss"):
        out[k] = r2[k]
    return out


def pair_loss_rule(al, ar, differ, n: int, margin: float = 2.0, w_same: float = 0.8, w_diff: float = 1.2):
    """The float64 half of the pair rule (csrc/head_fit_rule.h, PAIR) on rows ``al``, ``ar`` ``[P, E]`` with ``differ`` ``[P]`` in
    {0, 1}: ``(pair_loss [P], dist [P], ga_l [P, E], ga_r [P, E])`` in float64, the gradients those of ``sum(pair_loss) / n``."""
    al, ar = np.asarray(al, np.float64), np.asarray(ar, np.float64)
    dif = np.asarray(differ).astype(bool)
    with np.errstate(all="ignore"):
        nl, nr = np.sqrt((al * al).sum(axis=1)), np.sqrt((ar * ar).sum(axis=1))
        sl, sr = np.maximum(nl, NORM_EPS)[:, None], np.maximum(nr, NORM_EPS)[:, None]
        u, v = al / sl, ar / sr
        delta = (u - v) + DIST_EPS
        d0 = np.sqrt((delta * delta).sum(axis=1))
        d = np.maximum(d0, DIST_MIN)
        gap = np.maximum(float(margin) - d, 0.0)
        loss = np.where(dif, float(w_diff) * gap * gap, float(w_same) * d * d)
        q = np.where(dif, -2.0 * float(w_diff) * gap, 2.0 * float(w_same) * d) / float(max(n, 1))
        c = np.where(d0 < DIST_MIN, 0.0, q / np.where(d0 > 0, d0, 1.0))[:, None]
        ud, vd = (u * delta).sum(axis=1, keepdims=True), (v * delta).sum(axis=1, keepdims=True)
        gl = (c / sl) * np.where((nl > NORM_EPS)[:, None], delta - u * ud, delta)
        gr = (-c / sr) * np.where((nr > NORM_EPS)[:, None], delta - v * vd, delta)
    return loss, d, gl, gr


def pair_step_rule(x, left, right, differ, w, b, state: dict | None = None, keep=None, keep_scale: float = 1.0, *, margin: float = 2.0,
                   w_same: float = 0.8, w_diff: float = 1.2, accept: float = 0.5, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999,
                   eps: float = 1e-8, weight_decay: float = 0.0, decoupled: bool = False, amsgrad: bool = False, clear: bool = False,
                   dtype=np.float64, given: dict | None = None) -> dict:
    """One training step of the pair head, the specification (csrc/head_fit_rule.h, PAIR; include/frmap_hip.h, "Head fitting on pairs").

    ``dtype=np.float64``: the formulas in float64, as torch evaluates ``F.linear`` -> ``F.normalize`` -> ``F.pairwise_distance`` -> the
    clamp and the two weighted terms -> ``optim.Adam`` / ``AdamW``.  ``dtype=np.float32``: the projection and both update GEMMs by
    `dot32`, the update by `adam32`, and the loss half in float64 from the float32 ``a`` (and the float32 values of ``margin``,
    ``w_same``, ``w_diff`` and ``accept``: the library takes them as fp32), rounded once - what the host twin computes,
    word for word but for a rare last bit of ``ga``, ``pair_loss`` and ``dist`` (the order of the float64 sums).  ``given``: ``{"a",
    "ga", "pair_loss", "dist"}`` to take as they are.

    Nothing is modified: returns ``{"w", "b", "state", "a", "ga", "pair_loss", "dist", "row_src", "dw", "db", "n", "loss"}``."""
    f32 = np.dtype(dtype) == np.dtype(np.float32)
    x = np.asarray(x, F32 if f32 else np.float64)
    w, b = np.array(w, dtype), np.array(b, dtype)
    N, D = x.shape
    E = w.shape[0]
    left, right, differ = (np.asarray(t).astype(np.int64).reshape(-1) for t in (left, right, differ))
    P = len(left)
    st = _copy_state(state or fresh_state(D, E, amsgrad, dtype), dtype)
    if clear:
        st["rows"] = st["correct"] = st["loss_q"] = 0
    if f32:                                                           # (the library takes them as fp32 and widens those values)
        margin, w_same, w_diff = (float(F32(v)) for v in (margin, w_same, w_diff))
    idx = np.concatenate([left, right])
    row_ok = np.array([0 <= r < N and bool(np.isfinite(x[r]).all()) for r in idx])
    src = np.where(row_ok, idx, -1).astype(np.int32)

    def masked(ok):
        xp = np.zeros((2 * P, D), x.dtype)
        xp[ok] = x[src[ok]]
        if keep is not None:
            scaled = (xp * F32(keep_scale)).astype(F32) if f32 else xp * float(keep_scale)
            xp = np.where(np.asarray(keep).astype(bool), scaled, 0).astype(x.dtype)
            xp[~ok] = 0
        return xp
    with np.errstate(all="ignore"):
        if given is not None:
            a = np.array(given["a"], dtype)
        else:
            xr = masked(row_ok)
            a = (dot32(xr[:, None, :], w[None, :, :]) + b[None, :]).astype(F32) if f32 else xr @ w.T + b[None, :]
            a[~row_ok] = 0
    pair_ok = row_ok[:P] & row_ok[P:] & ((differ == 0) | (differ == 1))
    ok = np.concatenate([pair_ok, pair_ok])
    row_src = np.where(ok, src, -1).astype(np.int32)
    n = int(pair_ok.sum())
    st["n"] = n
    if given is not None:
        ga, pair_loss, dist = (np.array(given[k], dtype) for k in ("ga", "pair_loss", "dist"))
    else:
        loss64, d64, gl, gr = pair_loss_rule(a[:P], a[P:], differ == 1, n, margin, w_same, w_diff)
        ga = np.concatenate([gl, gr]).astype(dtype)
        ga[~ok] = 0
        pair_loss, dist = loss64.astype(dtype), d64.astype(dtype)
        pair_loss[~pair_ok] = np.nan
        dist[~pair_ok] = np.nan
    acc = F32(accept) if f32 else float(accept)
    st["rows"] += n
    st["correct"] += int((pair_ok & ((dist < acc) == (differ == 0))).sum())
    st["loss_q"] += loss_q(pair_loss[pair_ok])
    xp = masked(ok)
    gz = np.where(ok[:, None], ga, 0).astype(dtype)
    with np.errstate(all="ignore"):
        if f32:
            dw = dot32(gz.T[:, None, :], xp.T[None, :, :])
            db = dot32(gz.T, np.ones((1, 2 * P), F32))
        else:
            dw, db = gz.T @ xp, gz.sum(axis=0)
    out = {"a": a, "ga": ga, "pair_loss": pair_loss, "dist": dist, "row_src": row_src, "dw": dw, "db": db, "n": n,
           "loss": float(pair_loss[pair_ok].astype(np.float64).mean()) if n else float("nan")}
    if n:
        st["t"] += 1
        kw = dict(t=st["t"], lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, decoupled=decoupled, amsgrad=amsgrad,
                  f32=f32)
        w, b = _adam_rule(w, dw, st, "w", **kw), _adam_rule(b, db, st, "b", **kw)
    out["w"], out["b"], out["state"] = w, b, st
    return out


def margin_schedule(epoch: int, s: float = 32.0, m: float = 0.5, warm_up_epochs: int = 10, warm_up: bool = True):
    """``(m_eff, s_eff)`` of training epoch ``epoch``: the arithmetic of the reference's ``ArcMarginProduct`` in training mode
    (`src/face_models.py:336-348, 369, 401-409`).  ``margin_factor = min(0.9, (epoch / warm_up_epochs)^2)`` and ``scale_factor =
    min(0.8, 0.3 + 0.5 epoch / warm_up_epochs)`` inside the warm-up, 0.9 and 0.8 after it; ``m_eff = m margin_factor``; ``s_eff =
    min(s, 24) min(0.8, scale_factor)``, times ``(0.8 - 0.5 margin_factor)`` when ``m > 0.4``.  ``warm_up=False`` leaves the factors at
    the module's initial 0.0 and 0.3, as ``use_warm_up=False`` does.  The reference's randomly printed "hard cap" (`:415-418`) multiplies
    the output by 1, and no schedule reaches its threshold of 20 (``s_eff <= 24 x 0.8 = 19.2``): it is not restated."""
    margin_factor, scale_factor = 0.0, 0.3
    if warm_up:
        if epoch < warm_up_epochs:
            progress = epoch / warm_up_epochs
            margin_factor = min(0.9, progress * progress)
            scale_factor = min(0.8, 0.3 + 0.5 * progress)
        else:
            margin_factor, scale_factor = 0.9, 0.8
    m_eff = m * margin_factor
    s_eff = min(s, 24.0) * min(0.8, scale_factor)
    if m > 0.4:
        s_eff = s_eff * (0.8 - 0.5 * margin_factor)
    return m_eff, s_eff


def margin_logits_rule(z, rx, rw, y, s: float, m: float, easy_margin: bool = False, f32: bool = False):
    """The float64 half of the margin rule up to the logits (csrc/head_fit_rule.h, MARGIN) on ``z [B, C]``, ``rx [B]``, ``rw [C]`` and the
    targets ``y [B]``: ``{"cos", "cs", "inside", "theta_m", "out", "l", "dfac"}`` in float64 (``theta_m``: theta + m of every target).
    ``f32``: the clamp bounds are the fp32 roundings, as in the library; else the doubles ``1 - 1e-7``."""
    z, rx, rw = (np.asarray(t).astype(np.float64) for t in (z, rx, rw))
    B, C = z.shape
    hi = MARGIN_HI if f32 else 1.0 - 1e-7
    rows = np.arange(B)
    with np.errstate(all="ignore"):
        cos = (z * rx[:, None]) * rw[None, :]
        inside = (cos >= -hi) & (cos <= hi)
        cs = np.where(cos < -hi, -hi, np.where(cos > hi, hi, cos))
        out, dfac = cs.copy(), inside.astype(np.float64)
        cy, iy = cs[rows, y], inside[rows, y].astype(np.float64)
        theta = np.arccos(cy)
        tm = theta + float(m)
        ratio = np.sin(tm) / np.sin(theta)
        if easy_margin:
            take = cy > 0
            out[rows, y] = np.where(take, np.cos(tm), cy)
            dfac[rows, y] = np.where(take, iy * ratio, iy)
        else:
            capped = tm >= MARGIN_CAP                                    # (a NaN is not capped: it stays one, as torch.minimum keeps it)
            out[rows, y] = np.where(capped, math.cos(MARGIN_CAP), np.cos(tm))
            dfac[rows, y] = np.where(capped, 0.0, iy * ratio)
        return {"cos": cos, "cs": cs, "inside": inside, "theta_m": tm, "out": out, "l": float(s) * out, "dfac": dfac}


def margin_step_rule(x, labels, w, state: dict | None = None, rows=None, keep=None, keep_scale: float = 1.0, *, s: float, m: float,
                     easy_margin: bool = False, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                     weight_decay: float = 0.0, label_smoothing: float = 0.0, decoupled: bool = False, amsgrad: bool = False,
                     clear: bool = False, dtype=np.float64, given: dict | None = None, batch: int | None = None) -> dict:
    """One training step of the margin head, the specification (csrc/head_fit_rule.h, MARGIN; include/frmap_hip.h, "Head fitting with a
    margin").

    ``dtype=np.float64``: the formulas in float64 as torch evaluates the reference's ``F.normalize`` -> ``F.linear`` -> ``clamp`` ->
    ``acos`` -> ``minimum`` / ``where`` -> ``cross_entropy(label_smoothing=)`` -> ``optim.Adam`` / ``AdamW`` (the cosine is
    ``z / (|x'| |w|)`` on raw dot products: the same value).  ``dtype=np.float32``: z and both chains over B by `dot32`, rx and rw
    rounded to float32 once, the margin softmax in float64 from those float32 values (and the float32 values of ``s``, ``m`` and the
    bounds) with cosv, g, h and the row loss rounded once, the combination of dw in float32 products, `adam32` - what the host twin
    computes, word for word but for a rare last bit of rx, rw, cosv, g, h and the row loss.  ``given``: ``{"z", "rx", "rw", "cosv", "g",
    "h", "row_loss"}`` to take as they are.

    Nothing is modified: returns ``{"w", "state", "z", "rx", "rw", "cosv", "g", "h", "row_loss", "row_src", "pred", "dw", "n", "loss"}``
    and the float64 intermediates of `margin_logits_rule` under ``"detail"``."""
    f32 = np.dtype(dtype) == np.dtype(np.float32)
    x = np.asarray(x, F32 if f32 else np.float64)
    w = np.array(w, dtype)
    labels = np.asarray(labels).astype(np.int64)
    N, D = x.shape
    C = w.shape[0]
    st = _copy_state(state or fresh_state(D, C, amsgrad, dtype), dtype)
    if clear:
        st["rows"] = st["correct"] = st["loss_q"] = 0
    row_src, ok, xp = _rule_batch(x, labels, C, rows, len(keep) if keep is not None else (N if batch is None else int(batch)), keep,
                                  keep_scale, f32)
    B = len(row_src)
    n = int(ok.sum())
    st["n"] = n
    y = np.where(ok, labels[np.clip(row_src, 0, N - 1)], 0)
    if f32:
        s, m, ls = float(F32(s)), float(F32(m)), float(F32(label_smoothing))
    else:
        s, m, ls = float(s), float(m), float(label_smoothing)
    with np.errstate(all="ignore"):
        if given is not None:
            z, rx, rw = (np.array(given[k], dtype) for k in ("z", "rx", "rw"))
        else:
            z = dot32(xp[:, None, :], w[None, :, :]).astype(F32) if f32 else xp @ w.T
            z[~ok] = 0
            nx = np.sqrt((xp.astype(np.float64) ** 2).sum(axis=1))
            nw = np.sqrt((w.astype(np.float64) ** 2).sum(axis=1))
            rx = (1.0 / np.maximum(nx, NORM_EPS)).astype(dtype)
            rw = (1.0 / np.maximum(nw, NORM_EPS)).astype(dtype)
            rx[~ok] = 0
        det = margin_logits_rule(z, rx, rw, y, s, m, easy_margin, f32)
        l = det["l"]
        pred = np.where(np.isnan(l).all(axis=1), -1, np.argmax(np.where(np.isnan(l), -np.inf, l), axis=1))
        if given is not None:
            cosv, g, h, row_loss = (np.array(given[k], dtype) for k in ("cosv", "g", "h", "row_loss"))
        else:
            mx = l.max(axis=1, keepdims=True)
            e = np.exp(l - mx)
            sm = e.sum(axis=1, keepdims=True)
            nl = np.log(sm) - (l - mx)
            nll = nl[np.arange(B), y]
            off = ls / C if ls > 0 else 0.0
            row_loss = (1.0 - ls) * nll + off * nl.sum(axis=1) if ls > 0 else nll
            row_loss = np.where(row_loss > 0, row_loss, np.where(np.isnan(row_loss), row_loss, 0)).astype(dtype)
            t64 = np.full((B, C), off)
            t64[np.arange(B), y] = (1.0 - ls) + off
            gcos = ((s * ((e / sm) - t64)) / float(max(n, 1))) * det["dfac"]
            g = (gcos * rx.astype(np.float64)[:, None]).astype(dtype)
            h = (gcos * det["cos"]).astype(dtype)
            cosv = det["cs"].astype(dtype)
            for a in (g, h, cosv):
                a[~ok] = 0
            row_loss[~ok] = np.nan
    st["rows"] += n
    st["correct"] += int((ok & (pred == y)).sum())
    st["loss_q"] += loss_q(row_loss[ok])
    gz, hz = np.where(ok[:, None], g, 0).astype(dtype), np.where(ok[:, None], h, 0).astype(dtype)
    with np.errstate(all="ignore"):
        if f32:
            A = dot32(gz.T[:, None, :], xp.T[None, :, :])
            k = dot32(hz.T, np.ones((1, B), F32))
            rw32 = rw.astype(F32)
            free = rw32 < MARGIN_RMAX
            t1 = (rw32[:, None] * A).astype(F32)
            t3 = (((rw32 * rw32).astype(F32) * k).astype(F32)[:, None] * w).astype(F32)
            dw = np.where(free[:, None], (t1 - t3).astype(F32), t1)
        else:
            nw = np.sqrt((w * w).sum(axis=1))
            free = nw > NORM_EPS
            dw = rw[:, None] * (gz.T @ xp) - np.where(free, rw * rw * hz.sum(axis=0), 0.0)[:, None] * w
    out = {"z": z, "rx": rx, "rw": rw, "cosv": cosv, "g": g, "h": h, "row_loss": row_loss, "row_src": row_src, "pred": pred, "dw": dw,
           "n": n, "detail": det, "ok": ok, "y": y, "loss": float(row_loss[ok].astype(np.float64).mean()) if n else float("nan")}
    if n:
        st["t"] += 1
        w = _adam_rule(w, dw, st, "w", t=st["t"], lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay,
                       decoupled=decoupled, amsgrad=amsgrad, f32=f32)
    out["w"], out["state"] = w, st
    return out


def embed_fresh_state(D: int, E: int, C: int, amsgrad: bool = False, dtype=np.float64) -> dict:
    """A state of `embed_step_rule`: ``{"linear", "bn", "margin"}`` of `fresh_state` dicts for (D, E), (1, E) and (E, C)."""
    return {"linear": fresh_state(D, E, amsgrad, dtype), "bn": fresh_state(1, E, amsgrad, dtype), "margin": fresh_state(E, C, amsgrad, dtype)}


def embed_step_rule(x, labels, w1, gamma, beta, running_mean, running_var, wc, state: dict | None = None, rows=None, keep=None,
                    keep_scale: float = 1.0, *, bn_eps: float = 1e-5, bn_momentum: float = 0.1, s: float, m: float,
                    easy_margin: bool = False, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                    weight_decay: float = 0.0, label_smoothing: float = 0.0, decoupled: bool = False, amsgrad: bool = False,
                    clear: bool = False, dtype=np.float64, given: dict | None = None, batch: int | None = None) -> dict:
    """One training step of the embedding head, the specification (csrc/head_fit_rule.h, EMBED; include/frmap_hip.h, "Head fitting of an
    embedding layer").

    ``dtype=np.float64``: the formulas in float64 as torch evaluates ``F.linear`` -> ``nn.BatchNorm1d`` in training mode -> the mask ->
    `margin_step_rule`'s chain -> one ``optim.Adam`` / ``AdamW`` over the four tensors.  ``dtype=np.float32``: a, S, k and the chains
    over B by `dot32`; the batch statistics, ah and da in float64 from float32 values and rounded once; the margin stage is
    `margin_step_rule` in float32 on ``(y', lab)``; `adam32` - what the host twin computes, word for word but for a rare last bit of the
    float64 stages.  ``given``: any of ``{"mean32", "rstd", "uvar", "ah"}`` (together), ``"margin"`` (`margin_step_rule`'s ``given``)
    and ``"da"`` to take as they are.  ``state``: `embed_fresh_state`'s shape, or ``None``.

    Nothing is modified: returns the new ``w1, gamma, beta, running_mean, running_var, wc, state`` and ``a, lab, row_src1, n1, n2, taken,
    mean32, rstd, uvar, ah, yp, gy, dbeta, dgamma, da, dw1, loss`` with the margin stage's own result under ``"margin"``."""
    f32 = np.dtype(dtype) == np.dtype(np.float32)
    given = given or {}
    x = np.asarray(x, F32 if f32 else np.float64)
    w1, gamma, beta, rm, rv = (np.array(t, dtype) for t in (w1, gamma, beta, running_mean, running_var))
    wc_old = np.array(wc, dtype)
    labels = np.asarray(labels).astype(np.int64)
    N, D = x.shape
    E, C = w1.shape[0], wc_old.shape[0]
    state = state or embed_fresh_state(D, E, C, amsgrad, dtype)
    row_src1, ok1, xz = _rule_batch(x, labels, C, rows, len(keep) if keep is not None else (N if batch is None else int(batch)), None, 1.0, f32)
    B = len(row_src1)
    n1 = int(ok1.sum())
    live = n1 >= 2
    lab = np.where(ok1, labels[np.clip(row_src1, 0, N - 1)], -1).astype(np.int32)
    kept = np.asarray(keep).astype(bool) if keep is not None else None
    with np.errstate(all="ignore"):
        a = dot32(xz[:, None, :], w1[None, :, :]).astype(F32) if f32 else xz @ w1.T
        a[~ok1] = 0
        a64 = a.astype(np.float64)
        if "ah" in given:
            mean32, rstd, uvar, ah = (np.array(given[k], dtype) for k in ("mean32", "rstd", "uvar", "ah"))
        elif not live:
            mean32, rstd, uvar, ah = np.zeros(E, dtype), np.zeros(E, dtype), np.zeros(E, dtype), np.zeros((B, E), dtype)
        else:
            mean = a64[ok1].sum(axis=0) / n1
            var = ((a64[ok1] - mean) ** 2).sum(axis=0) / n1
            mean32 = mean.astype(dtype)
            rstd = (1.0 / np.sqrt(var + float(F32(bn_eps) if f32 else bn_eps))).astype(dtype)
            uvar = ((var * n1) / (n1 - 1)).astype(dtype)
            ah = ((a64 - (mean32.astype(np.float64) if f32 else mean)) * rstd.astype(np.float64)).astype(dtype)
            ah[~ok1] = 0
        y = (gamma[None, :] * ah).astype(dtype) + beta[None, :]
        yp = y.astype(dtype)
        if kept is not None:
            yp = np.where(kept, (y * (F32(keep_scale) if f32 else float(keep_scale))).astype(dtype), 0).astype(dtype)
        yp[~ok1] = 0
        if not live:
            yp[:] = 0
    r2 = margin_step_rule(yp, lab, wc_old, state["margin"], None, None, 1.0, s=s, m=m, easy_margin=easy_margin, lr=lr, beta1=beta1,
                          beta2=beta2, eps=eps, weight_decay=weight_decay, label_smoothing=label_smoothing, decoupled=decoupled,
                          amsgrad=amsgrad, clear=clear, dtype=dtype, given=given.get("margin"), batch=B)
    n2, ok2 = r2["n"], r2["ok"]
    taken = live and n2 == n1
    n = n1 if taken else 0
    gz, hz = np.where(ok2[:, None], r2["g"], 0).astype(dtype), np.where(ok2[:, None], r2["h"], 0).astype(dtype)
    rx, rw = np.asarray(r2["rx"], dtype), np.asarray(r2["rw"], dtype)
    with np.errstate(all="ignore"):
        if f32:
            gw = (gz * rw[None, :]).astype(F32)
            S = dot32(gw[:, None, :], wc_old.T[None, :, :])
            k = dot32(hz, np.ones((1, C), F32))
            t3 = (((rx * rx).astype(F32) * k).astype(F32)[:, None] * yp).astype(F32)
            gyp = np.where((rx < MARGIN_RMAX)[:, None], (S - t3).astype(F32), S)
            gy = gyp if kept is None else np.where(kept, (gyp * F32(keep_scale)).astype(F32), 0)
        else:
            free = rx < 1.0 / NORM_EPS
            gyp = (gz * rw[None, :]) @ wc_old - np.where(free, rx * rx * hz.sum(axis=1), 0.0)[:, None] * yp
            gy = gyp if kept is None else np.where(kept, gyp * float(keep_scale), 0)
        gy = np.where(ok2[:, None], gy, 0).astype(dtype)
        gyz, ahz = np.where(ok1[:, None], gy, 0).astype(dtype), np.where(ok1[:, None], ah, 0).astype(dtype)
        if f32:
            dbeta = dot32(gyz.T, np.ones((1, B), F32))
            dgamma = dot32(gyz.T, ahz.T)
        else:
            dbeta, dgamma = gyz.sum(axis=0), (gyz * ahz).sum(axis=0)
        if "da" in given:
            da = np.array(given["da"], dtype)
        elif not taken:
            da = np.zeros((B, E), dtype)
        else:
            g64, r64, b64, d64 = (t.astype(np.float64) for t in (gamma, rstd, dbeta, dgamma))
            da = ((g64 * r64)[None, :] * ((gy.astype(np.float64) - (b64 / n1)[None, :]) - ah.astype(np.float64) * (d64 / n1)[None, :])).astype(dtype)
            da[~ok1] = 0
        daz = np.where(ok1[:, None], da, 0).astype(dtype)
        dw1 = dot32(daz.T[:, None, :], xz.T[None, :, :]) if f32 else daz.T @ xz
    st1, st2 = _copy_state(state["linear"], dtype), _copy_state(state["bn"], dtype)
    if taken:
        st3, wc_new = r2["state"], r2["w"]
        kw = dict(t=st3["t"], lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, decoupled=decoupled, amsgrad=amsgrad, f32=f32)
        w1 = _adam_rule(w1, dw1, st1, "w", **kw)
        gamma = _adam_rule(gamma[:, None], dgamma[:, None], st2, "w", **kw)[:, 0]
        beta = _adam_rule(beta, dbeta, st2, "b", **kw)
        if f32:
            mom = F32(bn_momentum)
            omm = F32(F32(1) - mom)
            rm = (omm * rm).astype(F32) + (mom * mean32).astype(F32)
            rv = (omm * rv).astype(F32) + (mom * uvar).astype(F32)
        else:
            rm = (1.0 - bn_momentum) * rm + bn_momentum * mean32
            rv = (1.0 - bn_momentum) * rv + bn_momentum * uvar
    else:
        st3, wc_new = _copy_state(state["margin"], dtype), wc_old
        if clear:
            st3["rows"] = st3["correct"] = st3["loss_q"] = 0
        st3["n"] = 0
    for st in (st1, st2):
        st["t"], st["n"] = st3["t"], n
    return {"w1": w1, "gamma": gamma, "beta": beta, "running_mean": rm, "running_var": rv, "wc": wc_new,
            "state": {"linear": st1, "bn": st2, "margin": st3}, "a": a, "lab": lab, "row_src1": row_src1, "n1": n1, "n2": n2, "taken": taken,
            "mean32": mean32, "rstd": rstd, "uvar": uvar, "ah": ah, "yp": yp, "gy": gy, "dbeta": dbeta, "dgamma": dgamma, "da": da, "dw1": dw1,
            "loss": r2["loss"], "margin": r2}
