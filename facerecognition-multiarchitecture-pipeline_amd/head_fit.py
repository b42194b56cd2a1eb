"""Fit a classifier head on the device over cached trunk features.

With the trunk frozen its output for an image never changes, so the training set is embedded ONCE on the inference path
(`cache_features`) and what remains per step is softmax regression on a ``[B, D]`` view of the cached matrix: two small fp32
GEMMs, a row softmax and an Adam update (`frmap_head_fit_step`, csrc/head_fit.hip).  This is the training the reference does with
``ResNetTransfer(freeze_backbone=True)`` (`src/face_models.py:64-86`), in the frozen phase of two-phase ArcFace training
(`src/training.py:375-377`) and what the ``nn.Linear(512, num_classes)`` of `src/testing.py:134-136` lacks.  No backward pass
through a convolution exists here, and none is planned.

* `step_rule` - the specification of one step in numpy: float64 (checked against torch) or float32 in the order of
  csrc/head_fit_rule.h (what the kernels and the host twin compute, word for word).
* `step` / `step_host` - the step on device tensors / on numpy arrays through the host twin.
* `LinearHead` - weight, bias, optimiser state and workspace on the device.
* `cache_features`, `fit_head` - from a folder of images to a fitted head.
* `group_step` / `group_step_host` / `group_step_rule`, `HeadGroup` - ``H`` independent heads over one cache advanced by one call
  (`frmap_head_fit_group_step`): head ``h`` has the bits of `step` on its slices; the hyper-parameters are a table on the device.
* `kfold_rows`, `cross_validate`, `sweep_heads` - the reference's cross-validation (`src/cross_validation.py`) and the frozen-trunk
  part of its parameter search (`src/hyperparameter_tuning.py`) on one cache, every fold / trial a head of one group.

* `hidden_step_rule` / `hidden_step_host` / `hidden_step`, `HiddenHead` - one step of ``Linear(D, Hd) -> ReLU -> dropout ->
  Linear(Hd, C)`` (`frmap_head_fit_hidden_step`): layer 2 is `step` on the hidden activations, layer 1 plain backpropagation through
  the ReLU, one Adam over the four tensors.  `HiddenHead.embed` is a new embedding layer on a frozen trunk; for ``BaselineNet`` it
  is the model's own ``fc1`` (`cache_features(layer="pooled")`, `fit_head(hidden=512)`, `HiddenHead.load_into`).

Out of scope: groups of hidden heads, ``BatchNorm1d`` in a head, more than one hidden layer, gradient clipping, learning-rate schedulers (the caller passes ``lr`` per step), the margin schedule of
``ArcMarginProduct``, anything that trains a convolution, Optuna's sampler, pruner and schedulers (the caller supplies the trials).
"""
from __future__ import annotations

import math
import os
from typing import Optional

import numpy as np
import torch

from . import _lib, ops
from .ops import _dev, _sized, _stream

CHAIN = 128                       # FRMAP_HEAD_FIT_CHAIN: where the dot products are cut
MAX_C = MAX_D = 65536
MAX_B = 1 << 20
DECOUPLED, AMSGRAD, CLEAR = 1, 2, 4
EVAL = 8                          # grouped step only: figures, no update
MAX_H = 4096                      # heads of one group
HYPER_COLUMNS = ("lr", "beta1", "beta2", "eps", "weight_decay", "label_smoothing", "keep_scale")     # of the [H, 8] table; column 7 is 0
HEADER = ("t", "n", "rows", "correct", "loss_q")     # words 0 .. 4 of the 8-word header
LOSS_CLAMP, LOSS_SCALE = 65536.0, 16777216.0         # the tally's fixed point (csrc/tally_rule.h)
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------------------
# sizes and layouts
# ---------------------------------------------------------------------------------------------------------------------------------
def state_bytes(D: int, C: int, amsgrad: bool = False) -> int:
    """Bytes of an optimiser state (`frmap_head_fit_state_bytes`); ``ValueError`` for a shape the launcher refuses."""
    n = int(_lib.load().frmap_head_fit_state_bytes(int(D), int(C), int(bool(amsgrad))))
    if n == 0:
        raise ValueError(f"head_fit: unsupported D = {D}, C = {C} (D in 1 ... {MAX_D}, C in 1 ... {MAX_C})")
    return n


def workspace_bytes(B: int, D: int, C: int) -> int:
    """Bytes of the workspace of a step of ``B`` rows (`frmap_head_fit_workspace_bytes`)."""
    n = int(_lib.load().frmap_head_fit_workspace_bytes(int(B), int(D), int(C)))
    if n == 0:
        raise ValueError(f"head_fit: unsupported B = {B}, D = {D}, C = {C} (B in 1 ... {MAX_B}, D in 1 ... {MAX_D}, C in 1 ... {MAX_C})")
    return n


def state_layout(D: int, C: int, amsgrad: bool = False) -> dict:
    """name -> (byte offset, dtype, shape) of the state: the uint64 header words by name, then the fp32 moments."""
    out = {name: (8 * k, np.uint64, ()) for k, name in enumerate(HEADER)}
    at = 64
    for name, shape in (("m_w", (C, D)), ("v_w", (C, D)), ("m_b", (C,)), ("v_b", (C,))) + (
            (("vmax_w", (C, D)), ("vmax_b", (C,))) if amsgrad else ()):
        out[name] = (at, np.float32, shape)
        at += 4 * int(np.prod(shape))
    assert (at + 7) // 8 * 8 == state_bytes(D, C, amsgrad), (at, state_bytes(D, C, amsgrad))
    return out


def state_views(state: np.ndarray, D: int, C: int, amsgrad: bool = False) -> dict:
    """name -> numpy view into a host copy of a state (header words as 0-d views)."""
    raw = np.ascontiguousarray(state).view(np.uint8).reshape(-1)
    out = {}
    for name, (at, dtype, shape) in state_layout(D, C, amsgrad).items():
        n = int(np.prod(shape)) if shape else 1
        out[name] = raw[at: at + n * np.dtype(dtype).itemsize].view(dtype).reshape(shape)
    return out


def workspace_views(workspace: np.ndarray, B: int, C: int) -> dict:
    """z [B, C], g [B, C], row_loss [B] (float32) and row_src [B] (int32) of a host copy of a workspace."""
    raw = np.ascontiguousarray(workspace).view(np.uint8).reshape(-1)
    f = raw[: 4 * (2 * B * C + B)].view(np.float32)
    return {"z": f[: B * C].reshape(B, C), "g": f[B * C: 2 * B * C].reshape(B, C), "row_loss": f[2 * B * C:],
            "row_src": raw[4 * (2 * B * C + B): 4 * (2 * B * C + 2 * B)].view(np.int32)}


def figures_of(head_words) -> dict:
    """rows, accuracy and mean loss of the epoch figures (NaN for an empty epoch)."""
    rows, correct, loss_q = int(head_words["rows"]), int(head_words["correct"]), int(head_words["loss_q"])
    return {"rows": rows, "correct": correct, "accuracy": correct / rows if rows else float("nan"),
            "loss": loss_q / LOSS_SCALE / rows if rows else float("nan")}


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------------
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


def step_rule(x, labels, w, b, state: Optional[dict] = None, rows=None, keep=None, keep_scale: float = 1.0, *, lr: float = 1e-3,
              beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0, label_smoothing: float = 0.0,
              decoupled: bool = False, amsgrad: bool = False, clear: bool = False, dtype=np.float64, given: Optional[dict] = None,
              batch: Optional[int] = None) -> dict:
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
    if rows is None:                                   # rows 0 .. B-1: B is the mask's, else `batch`, else the whole cache
        rows = np.arange(len(keep) if keep is not None else (N if batch is None else int(batch)), dtype=np.int64)
    else:
        rows = np.asarray(rows).astype(np.int64)
    B = len(rows)
    st = {k: (np.array(v, dtype) if isinstance(v, np.ndarray) else int(v)) for k, v in (state or fresh_state(D, C, amsgrad, dtype)).items()}
    if clear:
        st["rows"] = st["correct"] = st["loss_q"] = 0
    # declined rows
    row_src = np.full((B,), -1, np.int32)
    for i, r in enumerate(rows):
        if 0 <= r < N and 0 <= labels[r] < C and np.isfinite(x[r]).all():
            row_src[i] = r
    ok = row_src >= 0
    n = int(ok.sum())
    st["n"] = n
    xp = np.zeros((B, D), x.dtype)
    xp[ok] = x[row_src[ok]]
    if keep is not None:
        kept = np.asarray(keep).astype(bool)
        scaled = (xp * F32(keep_scale)).astype(F32) if f32 else xp * float(keep_scale)
        xp = np.where(kept, scaled, 0).astype(x.dtype)
        xp[~ok] = 0
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
        t = st["t"]
        if f32:
            a = adam_scalars32(t, lr, beta1, beta2, eps, weight_decay)
            w, st["m_w"], st["v_w"], vm = adam32(a, dw, w, st["m_w"], st["v_w"], st.get("vmax_w"), decoupled, amsgrad)
            b, st["m_b"], st["v_b"], vb = adam32(a, db, b, st["m_b"], st["v_b"], st.get("vmax_b"), decoupled, amsgrad)
            if amsgrad:
                st["vmax_w"], st["vmax_b"] = vm, vb
        else:
            for p, grad, km, kv, kx in ((w, dw, "m_w", "v_w", "vmax_w"), (b, db, "m_b", "v_b", "vmax_b")):
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
    out["w"], out["b"], out["state"] = w, b, st
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the host twin
# ---------------------------------------------------------------------------------------------------------------------------------
def _flags(decoupled, amsgrad, clear) -> int:
    return (DECOUPLED if decoupled else 0) | (AMSGRAD if amsgrad else 0) | (CLEAR if clear else 0)


def step_host(x, labels, w, b, state: np.ndarray, workspace: Optional[np.ndarray] = None, rows=None, keep=None, keep_scale: float = 1.0, *,
              lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0,
              label_smoothing: float = 0.0, decoupled: bool = False, amsgrad: bool = False, clear: bool = False, given_g: bool = False,
              batch: Optional[int] = None):
    """The step on the CPU over numpy arrays (`frmap_head_fit_step_host`: the kernels' rule header compiled for the host; no GPU).
    ``w`` [C, D], ``b`` [C] (float32) and ``state`` (uint8, `state_bytes` bytes) are updated IN PLACE; ``workspace`` (uint8, exactly
    `workspace_bytes` bytes, or ``None`` for a fresh one) receives z, g, row_loss and row_src - with ``given_g`` its z, g and
    row_loss are inputs.  ``batch``: B when neither ``rows`` nor ``keep`` gives it (default N).  Returns the workspace."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    if x.ndim != 2 or labels.shape != (x.shape[0],):
        raise ValueError("head_fit.step_host: x [N, D] and labels [N] expected")
    N, D = x.shape
    for name, t, dt in (("w", w, np.float32), ("b", b, np.float32), ("state", state, np.uint8)):
        if not (isinstance(t, np.ndarray) and t.dtype == dt and t.flags.c_contiguous and t.flags.writeable):
            raise ValueError(f"head_fit.step_host: {name} must be a writable contiguous {np.dtype(dt).name} array")
    if w.ndim != 2 or w.shape[1] != D or b.shape != (w.shape[0],):
        raise ValueError(f"head_fit.step_host: w [C, {D}] and b [C] expected, got {w.shape} and {b.shape}")
    C = w.shape[0]
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        if rows.ndim != 1:
            raise ValueError("head_fit.step_host: rows [B] expected")
    B = len(rows) if rows is not None else (len(keep) if keep is not None else (N if batch is None else int(batch)))
    if keep is not None:
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        if keep.shape != (B, D):
            raise ValueError(f"head_fit.step_host: keep must be [{B}, {D}], got {keep.shape}")
    if rows is None and B > N:
        raise ValueError(f"head_fit.step_host: {B} batch rows without `rows` exceed the {N} cached rows")
    if state.shape != (state_bytes(D, C, amsgrad),) or state.ctypes.data % 8:
        raise ValueError(f"head_fit.step_host: state must be {state_bytes(D, C, amsgrad)} bytes, 8-byte aligned")
    nbytes = workspace_bytes(B, D, C)
    if workspace is None:
        if given_g:
            raise ValueError("head_fit.step_host: given_g needs the workspace that holds z, g and row_loss")
        workspace = np.zeros((nbytes,), np.uint8)
    if not (isinstance(workspace, np.ndarray) and workspace.dtype == np.uint8 and workspace.flags.c_contiguous and workspace.flags.writeable
            and workspace.shape == (nbytes,) and workspace.ctypes.data % 4 == 0):
        raise ValueError(f"head_fit.step_host: workspace must be a writable uint8 array of exactly {nbytes} bytes")
    _lib.check(_lib.load().frmap_head_fit_step_host(x.ctypes.data, labels.ctypes.data, rows.ctypes.data if rows is not None else 0,
                                                    keep.ctypes.data if keep is not None else 0, float(keep_scale), w.ctypes.data,
                                                    b.ctypes.data, state.ctypes.data, workspace.ctypes.data, N, B, D, C, float(lr),
                                                    float(beta1), float(beta2), float(eps), float(weight_decay), float(label_smoothing),
                                                    _flags(decoupled, amsgrad, clear), int(bool(given_g))), "head_fit.step_host")
    return workspace


# ---------------------------------------------------------------------------------------------------------------------------------
# the step on the device
# ---------------------------------------------------------------------------------------------------------------------------------
@ops._on_operand_device
def step(x: torch.Tensor, labels: torch.Tensor, w: torch.Tensor, b: torch.Tensor, state: torch.Tensor, workspace: torch.Tensor,
         rows: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None, keep_scale: float = 1.0, *, lr: float = 1e-3,
         beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0, label_smoothing: float = 0.0,
         decoupled: bool = False, amsgrad: bool = False, clear: bool = False, batch: Optional[int] = None) -> None:
    """One training step on the current stream (`frmap_head_fit_step`; nothing is copied or synchronised).  ``x`` float32 ``[N, D]``
    (the cache), ``labels`` int32 ``[N]``, ``w`` float32 ``[C, D]`` and ``b`` ``[C]`` (updated in place), ``state`` uint8 of
    `state_bytes` bytes (zeros = fresh; updated in place), ``workspace`` uint8 of exactly `workspace_bytes` bytes (written),
    ``rows`` int32 ``[B]`` or ``None`` (rows ``0 .. B-1``; ``B`` is then ``keep``'s row count, else ``batch``, else ``N``), ``keep`` uint8 ``[B, D]``
    or ``None``.  Every extent that depends on another operand is checked here, before the library sees a pointer."""
    op = "head_fit.step"
    x = _dev(x, f"{op}.x", torch.float32, ("frmap_head_fit_step", "x"))
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{op}: x [N, D] expected, got {tuple(x.shape)}")
    N, D = int(x.shape[0]), int(x.shape[1])
    _sized(labels, op, "labels", (N,), torch.int32)
    _sized(w, op, "w", (w.shape[0] if isinstance(w, torch.Tensor) and w.dim() == 2 else -1, D), torch.float32)
    C = int(w.shape[0])
    _sized(b, op, "b", (C,), torch.float32)
    if rows is not None:
        if isinstance(rows, torch.Tensor) and rows.dim() != 1:
            raise ValueError(f"{op}: rows [B] expected, got {tuple(rows.shape)}")
        rows = _dev(rows, f"{op}.rows", torch.int32, ("frmap_head_fit_step", "rows"))
        B = int(rows.shape[0])
    elif keep is not None and isinstance(keep, torch.Tensor) and keep.dim() == 2:
        B = int(keep.shape[0])
    else:
        B = N if batch is None else int(batch)
    if rows is None and B > N:
        raise ValueError(f"{op}: {B} batch rows without `rows` exceed the {N} cached rows")
    if keep is not None:
        _sized(keep, op, "keep", (B, D), torch.uint8)
    _sized(state, op, "state", (state_bytes(D, C, amsgrad),), torch.uint8)
    _sized(workspace, op, "workspace", (workspace_bytes(B, D, C),), torch.uint8)
    held = []                                                   # copies `_dev` made live until the launch is enqueued
    labels = _dev(labels, f"{op}.labels", torch.int32, ("frmap_head_fit_step", "labels"))
    keep = None if keep is None else _dev(keep, f"{op}.keep", torch.uint8, ("frmap_head_fit_step", "keep"))
    held += [x, labels, rows, keep]
    w = _dev(w, f"{op}.w", torch.float32, ("frmap_head_fit_step", "w"), owned=True)
    b = _dev(b, f"{op}.b", torch.float32, ("frmap_head_fit_step", "b"), owned=True)
    state = _dev(state, f"{op}.state", torch.uint8, ("frmap_head_fit_step", "state"), owned=True)
    workspace = _dev(workspace, f"{op}.workspace", torch.uint8, ("frmap_head_fit_step", "workspace"), owned=True)
    _lib.check(_lib.load().frmap_head_fit_step(x.data_ptr(), labels.data_ptr(), rows.data_ptr() if rows is not None else 0,
                                               keep.data_ptr() if keep is not None else 0, float(keep_scale), w.data_ptr(), b.data_ptr(),
                                               state.data_ptr(), workspace.data_ptr(), N, B, D, C, float(lr), float(beta1), float(beta2),
                                               float(eps), float(weight_decay), float(label_smoothing), _flags(decoupled, amsgrad, clear),
                                               _stream()), op)
    del held


class LinearHead:
    """A linear softmax classifier ``[C, D]`` on the device with its Adam state and a workspace.  ``weight`` / ``bias`` are
    initialised as ``nn.Linear`` does (Kaiming-uniform with a = sqrt(5): both uniform in ±1/sqrt(D)) from ``generator`` (a CPU
    ``torch.Generator``; ``None``: torch's default)."""

    def __init__(self, D: int, C: int, device="cuda", amsgrad: bool = False, generator: Optional[torch.Generator] = None):
        self.D, self.C, self.amsgrad = int(D), int(C), bool(amsgrad)
        nbytes = state_bytes(self.D, self.C, self.amsgrad)          # (refuses a bad shape)
        bound = 1.0 / math.sqrt(self.D)
        w = (torch.rand((self.C, self.D), generator=generator, dtype=torch.float32) * 2 - 1) * bound
        b = (torch.rand((self.C,), generator=generator, dtype=torch.float32) * 2 - 1) * bound
        self.device = torch.device(device)
        self.weight, self.bias = w.to(self.device), b.to(self.device)
        self.state = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        self._workspaces = {}
        self._clear = True

    def _workspace(self, B: int) -> torch.Tensor:
        ws = self._workspaces.get(B)
        if ws is None:
            ws = self._workspaces[B] = torch.empty((workspace_bytes(B, self.D, self.C),), dtype=torch.uint8, device=self.device)
        return ws

    def new_epoch(self) -> "LinearHead":
        """The next `step` clears the epoch figures first."""
        self._clear = True
        return self

    def step(self, x: torch.Tensor, labels: torch.Tensor, rows: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None, *,
             lr: float, keep_scale: Optional[float] = None, dropout: float = 0.0, beta1: float = 0.9, beta2: float = 0.999,
             eps: float = 1e-8, weight_decay: float = 0.0, label_smoothing: float = 0.0, decoupled: bool = False) -> "LinearHead":
        """One step over rows ``rows`` of the cache ``x`` / ``labels`` (`step`).  ``keep``: a uint8 ``[B, D]`` dropout mask, scaled by
        ``keep_scale`` (default ``1 / (1 - dropout)``).  No synchronisation."""
        if keep_scale is None:
            keep_scale = 1.0 / (1.0 - float(dropout)) if keep is not None else 1.0
        B = int(rows.shape[0]) if isinstance(rows, torch.Tensor) and rows.dim() == 1 else (
            int(keep.shape[0]) if isinstance(keep, torch.Tensor) and keep.dim() == 2 else int(x.shape[0]))
        step(x, labels, self.weight, self.bias, self.state, self._workspace(B), rows, keep, keep_scale, lr=lr, beta1=beta1, beta2=beta2,
             eps=eps, weight_decay=weight_decay, label_smoothing=label_smoothing, decoupled=decoupled, amsgrad=self.amsgrad,
             clear=self._clear)
        self._clear = False
        return self

    def epoch_figures(self) -> dict:
        """The one host copy: rows, correct, accuracy and mean loss since the last `new_epoch`, and the step count ``t``."""
        words = self.state[:64].cpu().numpy().view(np.uint64)
        out = figures_of({name: words[k] for k, name in enumerate(HEADER)})
        out["t"] = int(words[0])
        return out

    def logits(self, x: torch.Tensor) -> torch.Tensor:
        return ops.linear_f32(x, self.weight, None, self.bias)

    def state_dict(self) -> dict:
        return {"weight": self.weight.detach().clone(), "bias": self.bias.detach().clone()}

    def load_into(self, model) -> None:
        """Copy the head into ``resnet.fc[1]`` of a ``ResNetTransfer`` in place (the model's plan watches the parameters' versions:
        the next forward rebuilds)."""
        fc = getattr(getattr(model, "resnet", None), "fc", None)
        if not isinstance(fc, torch.nn.Sequential) or tuple(fc[1].weight.shape) != (self.C, self.D):
            raise ValueError(f"LinearHead.load_into: a ResNetTransfer with a [{self.C}, {self.D}] classifier expected")
        with torch.no_grad():
            fc[1].weight.copy_(self.weight)
            fc[1].bias.copy_(self.bias)

    def as_classifier(self):
        """The ``(w, b)`` pair `evaluate.evaluate_model` / `evaluate_stream` take as ``arcface_classifier``."""
        return self.weight, self.bias


# ---------------------------------------------------------------------------------------------------------------------------------
# from images to a head
# ---------------------------------------------------------------------------------------------------------------------------------
def _batches(data, batch_size, device):
    from . import evaluate
    if isinstance(data, (str, os.PathLike)):
        samples, _ = evaluate.image_folder(str(data))
        if not samples:
            raise FileNotFoundError(f"Found 0 files in subfolders of: {data}")
        return evaluate._folder_batches(samples, batch_size, device)
    return iter(data)


def cache_features(model, model_type: str, data, batch_size: int = 256, device="cuda", layer: str = "embedding"):
    """Embed a training set once: ``[N, D]`` float32 features and ``[N]`` int32 labels on the device, through the model's EVAL-mode
    ``get_embedding`` (the deployed trunk; the reference's frozen phase still runs BatchNorm in training mode - DESIGN.md §4).
    ``data``: an image folder (one sub-directory per class) or an iterable of ``(images, labels)`` batches.
    ``layer="pooled"`` (``BaselineNet`` only): cache the ``[N, 128]`` input of ``fc1`` (`BaselineNet.pooled_features`) instead, for a
    `HiddenHead` that fits ``fc1`` and ``fc2``."""
    if model_type == 'siamese':
        raise ValueError("head_fit: a siamese model has no classifier head to fit (pairs are verification_metrics' business)")
    if layer not in ("embedding", "pooled"):
        raise ValueError(f"head_fit.cache_features: layer must be 'embedding' or 'pooled', got {layer!r}")
    if layer == "pooled" and type(model).__name__ != "BaselineNet":
        raise ValueError(f"head_fit.cache_features: layer='pooled' is BaselineNet's (the input of its fc1), got {type(model).__name__}")
    embed = model.pooled_features if layer == "pooled" else model.get_embedding
    if model.training:
        model.eval()
    feats, labs = [], []
    with torch.no_grad():
        for images, labels in _batches(data, batch_size, device):
            emb = embed(images.to(device))
            feats.append(emb.float().reshape(images.shape[0], -1).clone())
            labs.append(torch.as_tensor(labels).to(torch.int64).clamp(-1, 2 ** 31 - 1).to(torch.int32).to(device, non_blocking=True))
    if not feats:
        raise ValueError("head_fit.cache_features: the data set is empty")
    return torch.cat(feats).contiguous(), torch.cat(labs).contiguous()


def fit_head(model, model_type: str, train_data, val_data=None, epochs: int = 10, batch_size: int = 32, lr: float = 1e-3,
             weight_decay: float = 1e-4, dropout: float = 0.1, label_smoothing: float = 0.0, decoupled: bool = False, amsgrad: bool = False,
             generator: Optional[torch.Generator] = None, num_classes: Optional[int] = None, device="cuda", hidden: Optional[int] = None,
             hidden_dropout: float = 0.5):
    """Fit a `LinearHead` on the frozen model's features.  The training set is embedded once (`cache_features`); every epoch then
    draws a fresh device permutation as ``rows`` and fresh dropout masks from ``generator`` (a generator on ``device``; ``None``:
    the device's default) and steps through it ``batch_size`` rows at a time with no host copy inside the epoch; the epoch's figures
    are one 64-byte copy at its end.  With ``val_data`` every epoch's validation logits go through `evaluate.ClassificationTally`.
    The defaults are the reference's for ``cnn`` (`src/training.py:184, 352`: Adam, lr 1e-3, weight decay 1e-4, Dropout(0.1));
    ``decoupled=True, amsgrad=True, label_smoothing=0.05`` are its ArcFace settings (`:341-348`).  Returns ``(head, history)`` with
    ``history = {"train_loss": [...], "train_acc": [...], "val": [metrics dict per epoch]}``.

    ``hidden=Hd``: fit a `HiddenHead` ``Linear(D, Hd) -> ReLU -> Dropout(hidden_dropout) -> Linear(Hd, C)`` instead, with ``dropout`` on
    its input and a second mask draw per step for the hidden layer.  For a ``BaselineNet`` the cache is then its pooled ``[N, 128]``
    features (`cache_features(layer="pooled")`), so that ``hidden=512`` fits its own ``fc1`` / ``fc2`` (`HiddenHead.load_into`); for
    every other model it is the embedding, and ``w1`` a learned projection of it."""
    from . import evaluate
    if model_type == 'siamese':
        raise ValueError("head_fit: a siamese model has no classifier head to fit (pairs are verification_metrics' business)")
    if hidden is not None:
        return _fit_hidden_head(model, model_type, train_data, val_data, epochs, batch_size, lr, weight_decay, dropout, label_smoothing,
                                decoupled, amsgrad, generator, num_classes, device, int(hidden), float(hidden_dropout))
    feats, labels = cache_features(model, model_type, train_data, device=device)
    N, D = int(feats.shape[0]), int(feats.shape[1])
    C = int(num_classes) if num_classes is not None else int(labels.max().item()) + 1
    head_gen = None
    if generator is not None and generator.device.type == "cpu":
        head_gen = generator
    head = LinearHead(D, C, feats.device, amsgrad=amsgrad, generator=head_gen)
    dev_gen = generator if generator is not None and generator.device.type != "cpu" else None
    if generator is not None and dev_gen is None:
        dev_gen = torch.Generator(device=feats.device)
        dev_gen.manual_seed(int(torch.randint(0, 2 ** 62, (1,), generator=generator).item()))
    val = None
    if val_data is not None:
        val = cache_features(model, model_type, val_data, device=device)
    history = {"train_loss": [], "train_acc": [], "val": []}
    for _ in range(int(epochs)):
        perm = torch.randperm(N, device=feats.device, generator=dev_gen).to(torch.int32)
        head.new_epoch()
        for lo in range(0, N, int(batch_size)):
            rows = perm[lo: lo + int(batch_size)]
            keep = None
            if dropout > 0:
                keep = (torch.rand((rows.shape[0], D), device=feats.device, generator=dev_gen) >= dropout).to(torch.uint8)
            head.step(feats, labels, rows, keep, lr=lr, dropout=dropout, weight_decay=weight_decay, label_smoothing=label_smoothing,
                      decoupled=decoupled)
        fig = head.epoch_figures()
        history["train_loss"].append(fig["loss"])
        history["train_acc"].append(fig["accuracy"])
        if val is not None:
            tally = evaluate.ClassificationTally(C, device=feats.device)
            tally.update(head.logits(val[0]), val[1])
            history["val"].append(tally.metrics())
    return head, history


def _fit_hidden_head(model, model_type, train_data, val_data, epochs, batch_size, lr, weight_decay, dropout, label_smoothing, decoupled,
                     amsgrad, generator, num_classes, device, hidden, hidden_dropout):
    """`fit_head(hidden=...)`: `fit_head`'s loop on a `HiddenHead`, with a second mask draw."""
    from . import evaluate
    layer = "pooled" if type(model).__name__ == "BaselineNet" else "embedding"
    feats, labels = cache_features(model, model_type, train_data, device=device, layer=layer)
    N, D = int(feats.shape[0]), int(feats.shape[1])
    C = int(num_classes) if num_classes is not None else int(labels.max().item()) + 1
    head_gen = generator if generator is not None and generator.device.type == "cpu" else None
    head = HiddenHead(D, hidden, C, feats.device, amsgrad=amsgrad, generator=head_gen)
    dev_gen = generator if generator is not None and generator.device.type != "cpu" else None
    if generator is not None and dev_gen is None:
        dev_gen = torch.Generator(device=feats.device)
        dev_gen.manual_seed(int(torch.randint(0, 2 ** 62, (1,), generator=generator).item()))
    val = None
    if val_data is not None:
        val = cache_features(model, model_type, val_data, device=device, layer=layer)
    history = {"train_loss": [], "train_acc": [], "val": []}
    for _ in range(int(epochs)):
        perm = torch.randperm(N, device=feats.device, generator=dev_gen).to(torch.int32)
        head.new_epoch()
        for lo in range(0, N, int(batch_size)):
            rows = perm[lo: lo + int(batch_size)]
            keep1 = keep2 = None
            if dropout > 0:
                keep1 = (torch.rand((rows.shape[0], D), device=feats.device, generator=dev_gen) >= dropout).to(torch.uint8)
            if hidden_dropout > 0:
                keep2 = (torch.rand((rows.shape[0], hidden), device=feats.device, generator=dev_gen) >= hidden_dropout).to(torch.uint8)
            head.step(feats, labels, rows, keep1, keep2, lr=lr, dropout1=dropout, dropout2=hidden_dropout, weight_decay=weight_decay,
                      label_smoothing=label_smoothing, decoupled=decoupled)
        fig = head.epoch_figures()
        history["train_loss"].append(fig["loss"])
        history["train_acc"].append(fig["accuracy"])
        if val is not None:
            tally = evaluate.ClassificationTally(C, device=feats.device)
            tally.update(head.logits(val[0]), val[1])
            history["val"].append(tally.metrics())
    return head, history


# ---------------------------------------------------------------------------------------------------------------------------------
# groups of heads: H independent heads over one cache, advanced by one call
# ---------------------------------------------------------------------------------------------------------------------------------
def group_state_stride(D: int, C: int, amsgrad: bool = False) -> int:
    """Bytes from head h's state to head h + 1's (`frmap_head_fit_group_state_stride`): `state_bytes` rounded up to 8."""
    n = int(_lib.load().frmap_head_fit_group_state_stride(int(D), int(C), int(bool(amsgrad))))
    if n == 0:
        raise ValueError(f"head_fit: unsupported D = {D}, C = {C} (D in 1 ... {MAX_D}, C in 1 ... {MAX_C})")
    return n


def group_state_bytes(H: int, D: int, C: int, amsgrad: bool = False) -> int:
    """Bytes of the states of ``H`` heads (`frmap_head_fit_group_state_bytes`): ``H`` strides."""
    n = int(_lib.load().frmap_head_fit_group_state_bytes(int(H), int(D), int(C), int(bool(amsgrad))))
    if n == 0:
        raise ValueError(f"head_fit: unsupported H = {H}, D = {D}, C = {C} (H in 1 ... {MAX_H}, D in 1 ... {MAX_D}, C in 1 ... {MAX_C})")
    return n


def group_workspace_bytes(H: int, B: int, D: int, C: int) -> int:
    """Bytes of the workspaces of ``H`` heads stepping ``B`` rows each (`frmap_head_fit_group_workspace_bytes`)."""
    n = int(_lib.load().frmap_head_fit_group_workspace_bytes(int(H), int(B), int(D), int(C)))
    if n == 0:
        raise ValueError(f"head_fit: unsupported H = {H}, B = {B}, D = {D}, C = {C} (H in 1 ... {MAX_H}, B in 1 ... {MAX_B}, "
                         f"D in 1 ... {MAX_D}, C in 1 ... {MAX_C})")
    return n


def _per_head(v, H: int, name: str) -> np.ndarray:
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0:
        return np.full((H,), float(a))
    if a.shape != (H,):
        raise ValueError(f"head_fit: {name} must be a scalar or a sequence of {H} values, got shape {a.shape}")
    return a


def hyper_table(H: int, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, label_smoothing=0.0, keep_scale=1.0) -> np.ndarray:
    """The float32 ``[H, 8]`` table a grouped step reads (`HYPER_COLUMNS`, a zero last): every value a scalar or one per head,
    rounded to float32 the way the single step's by-value arguments are."""
    cols = (lr, beta1, beta2, eps, weight_decay, label_smoothing, keep_scale)
    t = np.zeros((int(H), 8), np.float32)
    for k, (name, v) in enumerate(zip(HYPER_COLUMNS, cols)):
        t[:, k] = _per_head(v, int(H), name).astype(np.float32)
    return t


def _group_flags(decoupled, amsgrad, clear, evaluate) -> int:
    return _flags(decoupled, amsgrad, clear) | (EVAL if evaluate else 0)


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
            old = {k: (np.array(v, dtype) if isinstance(v, np.ndarray) else int(v)) for k, v in (st or fresh_state(D, C, amsgrad, dtype)).items()}
            for k in ("n", "rows", "correct", "loss_q"):
                old[k] = r["state"][k]
            r["w"], r["b"], r["state"] = np.array(w[h], dtype), np.array(b[h], dtype), old
        out.append(r)
    return out


def group_step_host(x, labels, rows, hyper, w, b, state: np.ndarray, workspace: Optional[np.ndarray] = None, keep=None, *,
                    decoupled: bool = False, amsgrad: bool = False, clear: bool = False, evaluate: bool = False, given_g: bool = False):
    """The grouped step on the CPU over numpy arrays (`frmap_head_fit_group_step_host`: the single host step looped over the heads).
    ``rows`` int32 ``[H, B]``, ``hyper`` float32 ``[H, 8]`` (`hyper_table`), ``w`` ``[H, C, D]``, ``b`` ``[H, C]`` and ``state`` (uint8,
    `group_state_bytes` bytes, 8-byte aligned) are updated IN PLACE; ``workspace`` (uint8, exactly `group_workspace_bytes` bytes, or
    ``None`` for a fresh one) receives every head's z, g, row_loss and row_src; ``keep`` uint8 ``[H, B, D]`` or ``None``.  Returns the
    workspace."""
    op = "head_fit.group_step_host"
    x = np.ascontiguousarray(x, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    if x.ndim != 2 or labels.shape != (x.shape[0],):
        raise ValueError(f"{op}: x [N, D] and labels [N] expected")
    N, D = x.shape
    for name, t, dt in (("w", w, np.float32), ("b", b, np.float32), ("state", state, np.uint8)):
        if not (isinstance(t, np.ndarray) and t.dtype == dt and t.flags.c_contiguous and t.flags.writeable):
            raise ValueError(f"{op}: {name} must be a writable contiguous {np.dtype(dt).name} array")
    if w.ndim != 3 or w.shape[2] != D or b.shape != w.shape[:2]:
        raise ValueError(f"{op}: w [H, C, {D}] and b [H, C] expected, got {w.shape} and {b.shape}")
    H, C = int(w.shape[0]), int(w.shape[1])
    if rows is None:
        raise ValueError(f"{op}: rows [H, B] is required")
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    if rows.ndim != 2 or rows.shape[0] != H:
        raise ValueError(f"{op}: rows must be [{H}, B], got {rows.shape}")
    B = int(rows.shape[1])
    if hyper is None:
        raise ValueError(f"{op}: hyper [H, 8] is required")
    hyper = np.ascontiguousarray(hyper, dtype=np.float32)
    if hyper.shape != (H, 8):
        raise ValueError(f"{op}: hyper must be [{H}, 8], got {hyper.shape}")
    if keep is not None:
        if evaluate:
            raise ValueError(f"{op}: keep cannot be given with evaluate=True")
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        if keep.shape != (H, B, D):
            raise ValueError(f"{op}: keep must be [{H}, {B}, {D}], got {keep.shape}")
    nstate = group_state_bytes(H, D, C, amsgrad)
    if state.shape != (nstate,) or state.ctypes.data % 8:
        raise ValueError(f"{op}: state must be {nstate} bytes, 8-byte aligned")
    nbytes = group_workspace_bytes(H, B, D, C)
    if workspace is None:
        if given_g:
            raise ValueError(f"{op}: given_g needs the workspace that holds z, g and row_loss")
        workspace = np.zeros((nbytes,), np.uint8)
    if not (isinstance(workspace, np.ndarray) and workspace.dtype == np.uint8 and workspace.flags.c_contiguous and workspace.flags.writeable
            and workspace.shape == (nbytes,) and workspace.ctypes.data % 4 == 0):
        raise ValueError(f"{op}: workspace must be a writable uint8 array of exactly {nbytes} bytes")
    _lib.check(_lib.load().frmap_head_fit_group_step_host(x.ctypes.data, labels.ctypes.data, rows.ctypes.data,
                                                          keep.ctypes.data if keep is not None else 0, hyper.ctypes.data, w.ctypes.data,
                                                          b.ctypes.data, state.ctypes.data, workspace.ctypes.data, N, H, B, D, C,
                                                          _group_flags(decoupled, amsgrad, clear, evaluate), int(bool(given_g))), op)
    return workspace


@ops._on_operand_device
def group_step(x: torch.Tensor, labels: torch.Tensor, rows: torch.Tensor, hyper: torch.Tensor, w: torch.Tensor, b: torch.Tensor,
               state: torch.Tensor, workspace: torch.Tensor, keep: Optional[torch.Tensor] = None, *, decoupled: bool = False,
               amsgrad: bool = False, clear: bool = False, evaluate: bool = False) -> None:
    """One step of ``H`` heads on the current stream (`frmap_head_fit_group_step`; nothing is copied or synchronised).  ``x`` float32
    ``[N, D]`` and ``labels`` int32 ``[N]`` are shared; ``w`` float32 ``[H, C, D]`` and ``b`` ``[H, C]`` (updated in place), ``rows``
    int32 ``[H, B]`` (an entry outside ``[0, N)`` declines that batch row), ``hyper`` float32 ``[H, 8]`` ON THE DEVICE
    (`hyper_table`), ``state`` uint8 of `group_state_bytes` bytes (zeros = fresh), ``workspace`` uint8 of exactly
    `group_workspace_bytes` bytes, ``keep`` uint8 ``[H, B, D]`` or ``None``.  ``evaluate``: figures only (flag 8; no ``keep``).
    Every extent that depends on another operand is checked here, before the library sees a pointer."""
    op, entry = "head_fit.group_step", "frmap_head_fit_group_step"
    x = _dev(x, f"{op}.x", torch.float32, (entry, "x"))
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{op}: x [N, D] expected, got {tuple(x.shape)}")
    N, D = int(x.shape[0]), int(x.shape[1])
    if not isinstance(w, torch.Tensor) or w.dim() != 3:
        raise ValueError(f"{op}: w [H, C, D] expected, got {tuple(w.shape) if isinstance(w, torch.Tensor) else type(w).__name__}")
    H, C = int(w.shape[0]), int(w.shape[1])
    _sized(w, op, "w", (H, C, D), torch.float32)
    _sized(labels, op, "labels", (N,), torch.int32)
    _sized(b, op, "b", (H, C), torch.float32)
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2:
        raise ValueError(f"{op}: rows [H, B] expected, got {tuple(rows.shape) if isinstance(rows, torch.Tensor) else type(rows).__name__}")
    B = int(rows.shape[1])
    _sized(rows, op, "rows", (H, B), torch.int32)
    _sized(hyper, op, "hyper", (H, 8), torch.float32)
    if keep is not None:
        if evaluate:
            raise ValueError(f"{op}: keep cannot be given with evaluate=True (flag 8 takes no dropout mask)")
        _sized(keep, op, "keep", (H, B, D), torch.uint8)
    _sized(state, op, "state", (group_state_bytes(H, D, C, amsgrad),), torch.uint8)
    _sized(workspace, op, "workspace", (group_workspace_bytes(H, B, D, C),), torch.uint8)
    held = []                                                   # copies `_dev` made live until the launch is enqueued
    labels = _dev(labels, f"{op}.labels", torch.int32, (entry, "labels"))
    rows = _dev(rows, f"{op}.rows", torch.int32, (entry, "rows"))
    hyper = _dev(hyper, f"{op}.hyper", torch.float32, (entry, "hyper"))
    keep = None if keep is None else _dev(keep, f"{op}.keep", torch.uint8, (entry, "keep"))
    held += [x, labels, rows, hyper, keep]
    w = _dev(w, f"{op}.w", torch.float32, (entry, "w"), owned=True)
    b = _dev(b, f"{op}.b", torch.float32, (entry, "b"), owned=True)
    state = _dev(state, f"{op}.state", torch.uint8, (entry, "state"), owned=True)
    workspace = _dev(workspace, f"{op}.workspace", torch.uint8, (entry, "workspace"), owned=True)
    _lib.check(_lib.load().frmap_head_fit_group_step(x.data_ptr(), labels.data_ptr(), rows.data_ptr(), keep.data_ptr() if keep is not None else 0,
                                                     hyper.data_ptr(), w.data_ptr(), b.data_ptr(), state.data_ptr(), workspace.data_ptr(),
                                                     N, H, B, D, C, _group_flags(decoupled, amsgrad, clear, evaluate), _stream()), op)
    del held


class HeadGroup:
    """``H`` linear softmax heads ``[C, D]`` over one cache, with their Adam states, workspaces and the device-resident hyper table
    (`group_step`).  The heads are initialised as ``H`` consecutive `LinearHead` objects would be from ``generator``; with ``shared_init``
    all of them start from head 0's draw (a parameter sweep compares settings, not initialisations)."""

    def __init__(self, H: int, D: int, C: int, device="cuda", amsgrad: bool = False, generator: Optional[torch.Generator] = None,
                 shared_init: bool = False):
        self.H, self.D, self.C, self.amsgrad = int(H), int(D), int(C), bool(amsgrad)
        nbytes = group_state_bytes(self.H, self.D, self.C, self.amsgrad)          # (refuses a bad shape)
        self.stride = group_state_stride(self.D, self.C, self.amsgrad)
        bound = 1.0 / math.sqrt(self.D)
        ws, bs = [], []
        for h in range(self.H):
            if h == 0 or not shared_init:
                w = (torch.rand((self.C, self.D), generator=generator, dtype=torch.float32) * 2 - 1) * bound
                b = (torch.rand((self.C,), generator=generator, dtype=torch.float32) * 2 - 1) * bound
            ws.append(w)
            bs.append(b)
        self.device = torch.device(device)
        self.weight, self.bias = torch.stack(ws).to(self.device), torch.stack(bs).to(self.device)
        self.state = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        self.hyper = torch.zeros((self.H, 8), dtype=torch.float32, device=self.device)
        self._hyper_host = np.zeros((self.H, 8), np.float32)
        self._workspaces = {}
        self._clear = True

    def _workspace(self, B: int) -> torch.Tensor:
        ws = self._workspaces.get(B)
        if ws is None:
            ws = self._workspaces[B] = torch.empty((group_workspace_bytes(self.H, B, self.D, self.C),), dtype=torch.uint8, device=self.device)
        return ws

    def set_hyper(self, table: np.ndarray) -> "HeadGroup":
        """Write the hyper table (`hyper_table`) with one host-to-device copy, and only when a value changed."""
        table = np.ascontiguousarray(table, np.float32)
        if table.shape != (self.H, 8):
            raise ValueError(f"HeadGroup.set_hyper: a [{self.H}, 8] table expected, got {table.shape}")
        if not np.array_equal(table.view(np.uint32), self._hyper_host.view(np.uint32)):
            self.hyper.copy_(torch.from_numpy(table))
            self._hyper_host = table.copy()
        return self

    def new_epoch(self) -> "HeadGroup":
        """The next `step` or `evaluate` clears every head's epoch figures first."""
        self._clear = True
        return self

    def step(self, x: torch.Tensor, labels: torch.Tensor, rows: torch.Tensor, keep: Optional[torch.Tensor] = None, *, lr,
             weight_decay=0.0, dropout=0.0, label_smoothing=0.0, beta1=0.9, beta2=0.999, eps=1e-8, decoupled: bool = False) -> "HeadGroup":
        """One step of every head over its rows ``rows[h]`` of the cache (`group_step`).  Every hyper-parameter is a scalar or a
        sequence of ``H`` values; ``keep``: a uint8 ``[H, B, D]`` dropout mask, head ``h``'s scaled by ``1 / (1 - dropout[h])``.  No
        synchronisation beyond the table's copy when a value changed."""
        keep_scale = 1.0 / (1.0 - _per_head(dropout, self.H, "dropout")) if keep is not None else 1.0
        self.set_hyper(hyper_table(self.H, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay,
                                   label_smoothing=label_smoothing, keep_scale=keep_scale))
        B = int(rows.shape[1]) if isinstance(rows, torch.Tensor) and rows.dim() == 2 else 1
        group_step(x, labels, rows, self.hyper, self.weight, self.bias, self.state, self._workspace(B), keep, decoupled=decoupled,
                   amsgrad=self.amsgrad, clear=self._clear)
        self._clear = False
        return self

    def evaluate(self, x: torch.Tensor, labels: torch.Tensor, rows: torch.Tensor) -> "HeadGroup":
        """Add the figures of rows ``rows[h]`` under every head's current weights (flag 8): nothing else changes.  The loss is the
        training loss of the table's ``label_smoothing``."""
        B = int(rows.shape[1]) if isinstance(rows, torch.Tensor) and rows.dim() == 2 else 1
        group_step(x, labels, rows, self.hyper, self.weight, self.bias, self.state, self._workspace(B), None, amsgrad=self.amsgrad,
                   clear=self._clear, evaluate=True)
        self._clear = False
        return self

    def epoch_figures(self) -> list:
        """ONE host copy of the ``H`` headers: per head what `LinearHead.epoch_figures` returns."""
        words = self.state.view(self.H, self.stride)[:, :64].cpu().numpy().view(np.uint64)
        out = []
        for h in range(self.H):
            fig = figures_of({name: words[h, k] for k, name in enumerate(HEADER)})
            fig["t"] = int(words[h, 0])
            out.append(fig)
        return out

    def head(self, h: int) -> LinearHead:
        """Head ``h`` as a `LinearHead` whose ``weight``, ``bias`` and ``state`` are VIEWS of the group's memory: `logits`,
        `state_dict`, `load_into` and `as_classifier` read the group's weights, and a single `step` on it continues head ``h``'s fit."""
        if not 0 <= int(h) < self.H:
            raise IndexError(f"HeadGroup.head: {h} is outside 0 ... {self.H - 1}")
        h = int(h)
        one = LinearHead.__new__(LinearHead)
        one.D, one.C, one.amsgrad, one.device = self.D, self.C, self.amsgrad, self.device
        one.weight, one.bias = self.weight[h], self.bias[h]
        one.state = self.state[h * self.stride: h * self.stride + state_bytes(self.D, self.C, self.amsgrad)]
        one._workspaces, one._clear = {}, False
        return one


def kfold_rows(N: int, n_folds: int = 5, seed: int = 42) -> list:
    """Per fold ``(train_idx, val_idx)`` as ascending int32 arrays: the split of
    ``sklearn.model_selection.KFold(n_folds, shuffle=True, random_state=seed).split(range(N))``, the reference's splitter
    (`src/cross_validation.py:97`), index for index, in numpy: ``RandomState(seed).shuffle(arange(N))``; fold ``k`` validates on
    the next ``N // n_folds`` shuffled indices (one more for the first ``N % n_folds`` folds)."""
    N, k = int(N), int(n_folds)
    if k < 2 or k > N:
        raise ValueError(f"head_fit.kfold_rows: n_folds = {k} must be in 2 ... N = {N}")
    idx = np.arange(N)
    np.random.RandomState(int(seed)).shuffle(idx)
    sizes = np.full((k,), N // k, dtype=np.int64)
    sizes[: N % k] += 1
    out, at = [], 0
    for size in sizes:
        mask = np.zeros((N,), bool)
        mask[idx[at: at + size]] = True
        out.append((np.flatnonzero(~mask).astype(np.int32), np.flatnonzero(mask).astype(np.int32)))
        at += int(size)
    return out


def _generators(generator, device):
    """(the CPU generator the heads are drawn from, the device generator of permutations and masks) of `fit_head`'s convention."""
    head_gen = generator if generator is not None and generator.device.type == "cpu" else None
    dev_gen = generator if generator is not None and generator.device.type != "cpu" else None
    if generator is not None and dev_gen is None:
        dev_gen = torch.Generator(device=device)
        dev_gen.manual_seed(int(torch.randint(0, 2 ** 62, (1,), generator=generator).item()))
    return head_gen, dev_gen


def padded_rows(index_sets, batch_size: int, device) -> torch.Tensor:
    """int32 ``[H, nb * batch_size]`` on ``device``: row ``h`` is ``index_sets[h]`` (a device int32 vector) followed by -1 up to a
    common whole number ``nb`` of batches."""
    B = int(batch_size)
    nb = max(1, max(-(-int(t.shape[0]) // B) for t in index_sets))
    out = torch.full((len(index_sets), nb * B), -1, dtype=torch.int32, device=device)
    for h, t in enumerate(index_sets):
        out[h, : t.shape[0]] = t
    return out


def epoch_rows(index_sets, batch_size: int, generator=None) -> torch.Tensor:
    """One epoch's training rows: a fresh device permutation of every head's index set, in the order of the heads, padded with -1
    (`padded_rows`)."""
    dev = index_sets[0].device
    return padded_rows([t[torch.randperm(int(t.shape[0]), device=dev, generator=generator)] for t in index_sets], batch_size, dev)


def draw_keep(H: int, B: int, D: int, dropout, device, generator=None) -> torch.Tensor:
    """A fresh uint8 ``[H, B, D]`` dropout mask: one uniform draw, kept where it is at least ``dropout`` (a number, or a tensor
    already on ``device`` that broadcasts against ``[H, B, D]``: nothing is uploaded here)."""
    return (torch.rand((H, B, D), device=device, generator=generator) >= dropout).to(torch.uint8)


def _run_epoch(group, feats, labels, rows_all, B, D, dropout, dev_gen, step_kw):
    """All training batches of one epoch; returns the epoch's figures (the one host copy)."""
    use_keep = float(dropout) > 0
    group.new_epoch()
    for lo in range(0, int(rows_all.shape[1]), B):
        keep = draw_keep(group.H, B, D, float(dropout), feats.device, dev_gen) if use_keep else None
        group.step(feats, labels, rows_all[:, lo: lo + B].contiguous(), keep, dropout=dropout, **step_kw)
    return group.epoch_figures()


def _run_eval(group, feats, labels, rows_all, B):
    group.new_epoch()
    for lo in range(0, int(rows_all.shape[1]), B):
        group.evaluate(feats, labels, rows_all[:, lo: lo + B].contiguous())
    return group.epoch_figures()


def cross_validate(feats: torch.Tensor, labels: torch.Tensor, n_folds: int = 5, epochs: int = 15, batch_size: int = 32, seed: int = 42,
                   lr: float = 1e-3, weight_decay: float = 1e-4, dropout: float = 0.1, label_smoothing: float = 0.0, decoupled: bool = False,
                   amsgrad: bool = False, num_classes: Optional[int] = None, generator: Optional[torch.Generator] = None) -> dict:
    """K-fold cross-validation of a head over cached features, all folds in one `HeadGroup` (the reference's
    `src/cross_validation.py` with the trunk frozen: 5 folds x 15 epochs at batch 32, `KFold(shuffle=True, random_state=seed)`).
    Per epoch: one device permutation per fold over that fold's training rows (`epoch_rows`), fresh masks (`draw_keep`), all folds'
    training steps in grouped calls, then grouped `evaluate` calls over the validation rows - two figure copies an epoch and no
    other host copy inside it.  Returns the reference's dict (``n_folds``, ``fold_results`` with ``fold`` from 1 and
    ``best_validation_accuracy``, ``mean_accuracy``, ``std_accuracy`` = ``np.mean`` / ``np.std``) plus ``history``: per fold the
    lists ``train_loss``, ``train_acc``, ``val_loss``, ``val_acc``; and ``group``, the fitted `HeadGroup`."""
    if feats.dim() != 2:
        raise ValueError(f"head_fit.cross_validate: feats [N, D] expected, got {tuple(feats.shape)}")
    N, D, B = int(feats.shape[0]), int(feats.shape[1]), int(batch_size)
    C = int(num_classes) if num_classes is not None else int(labels.max().item()) + 1
    H = int(n_folds)
    folds = kfold_rows(N, H, seed)
    head_gen, dev_gen = _generators(generator, feats.device)
    group = HeadGroup(H, D, C, feats.device, amsgrad=amsgrad, generator=head_gen)
    train = [torch.from_numpy(tr).to(feats.device) for tr, _ in folds]
    val_rows = padded_rows([torch.from_numpy(va).to(feats.device) for _, va in folds], B, feats.device)
    step_kw = dict(lr=lr, weight_decay=weight_decay, label_smoothing=label_smoothing, decoupled=decoupled)
    history = [{"train_loss": [], "train_acc": [], "val_loss": [], "val_acc": []} for _ in range(H)]
    best = [0.0] * H
    for _ in range(int(epochs)):
        tfig = _run_epoch(group, feats, labels, epoch_rows(train, B, dev_gen), B, D, dropout, dev_gen, step_kw)
        vfig = _run_eval(group, feats, labels, val_rows, B)
        for h in range(H):
            history[h]["train_loss"].append(tfig[h]["loss"])
            history[h]["train_acc"].append(tfig[h]["accuracy"])
            history[h]["val_loss"].append(vfig[h]["loss"])
            history[h]["val_acc"].append(vfig[h]["accuracy"])
            if vfig[h]["accuracy"] > best[h]:
                best[h] = vfig[h]["accuracy"]
    fold_results = [{"fold": h + 1, "best_validation_accuracy": best[h]} for h in range(H)]
    acc = [r["best_validation_accuracy"] for r in fold_results]
    return {"n_folds": H, "fold_results": fold_results, "mean_accuracy": float(np.mean(acc)), "std_accuracy": float(np.std(acc)),
            "history": history, "group": group}


def sweep_heads(feats: torch.Tensor, labels: torch.Tensor, val_feats: torch.Tensor, val_labels: torch.Tensor, trials, epochs: int = 10,
                batch_size: int = 32, decoupled: bool = False, amsgrad: bool = False, num_classes: Optional[int] = None,
                generator: Optional[torch.Generator] = None) -> dict:
    """A parameter sweep over cached features (the frozen-trunk part of the reference's `src/hyperparameter_tuning.py`): one head
    per trial in one `HeadGroup`.  ``trials``: a list of dicts over ``lr``, ``weight_decay``, ``dropout``, ``label_smoothing``
    (missing keys: `fit_head`'s defaults).  All trials start from the same weights (``shared_init``) and see the same rows in the
    same permutation and the same uniform draw behind their masks.  The validation rows are appended to the cache so that one grouped
    `evaluate` reads them.  The sampler, pruner and schedulers of the reference stay with the caller, who supplies the trials.
    Returns ``{"trials": [{"params", "val_acc": [...], "val_loss": [...], "best_validation_accuracy"}], "best_trial": index,
    "best_params", "group"}``; ties go to the earlier trial."""
    trials = [dict(t) for t in trials]
    H = len(trials)
    if H < 1:
        raise ValueError("head_fit.sweep_heads: at least one trial expected")
    unknown = sorted({k for t in trials for k in t} - {"lr", "weight_decay", "dropout", "label_smoothing"})
    if unknown:
        raise ValueError(f"head_fit.sweep_heads: a trial may set lr, weight_decay, dropout and label_smoothing, not {unknown}")
    defaults = {"lr": 1e-3, "weight_decay": 1e-4, "dropout": 0.1, "label_smoothing": 0.0}
    col = {k: [float(t.get(k, v)) for t in trials] for k, v in defaults.items()}
    N, D, B = int(feats.shape[0]), int(feats.shape[1]), int(batch_size)
    C = int(num_classes) if num_classes is not None else int(labels.max().item()) + 1
    cache = torch.cat([feats, val_feats]).contiguous()
    cache_labels = torch.cat([labels, val_labels]).to(torch.int32).contiguous()
    head_gen, dev_gen = _generators(generator, feats.device)
    group = HeadGroup(H, D, C, feats.device, amsgrad=amsgrad, generator=head_gen, shared_init=True)
    val_one = torch.arange(N, N + int(val_feats.shape[0]), dtype=torch.int32, device=feats.device)
    val_rows = padded_rows([val_one] * H, B, feats.device)
    step_kw = dict(lr=col["lr"], weight_decay=col["weight_decay"], label_smoothing=col["label_smoothing"], decoupled=decoupled)
    out = [{"params": {k: col[k][h] for k in defaults}, "val_acc": [], "val_loss": [], "train_acc": [], "train_loss": []} for h in range(H)]
    use_keep = any(p > 0 for p in col["dropout"])
    drop = torch.tensor(col["dropout"], dtype=torch.float32, device=feats.device).reshape(H, 1, 1)
    for _ in range(int(epochs)):
        perm = torch.randperm(N, device=feats.device, generator=dev_gen).to(torch.int32)
        rows_all = padded_rows([perm] * H, B, feats.device)
        group.new_epoch()
        for lo in range(0, int(rows_all.shape[1]), B):
            keep = None
            if use_keep:                                          # one uniform draw for all trials: they differ in the threshold only
                u = torch.rand((B, D), device=feats.device, generator=dev_gen)
                keep = (u[None] >= drop).to(torch.uint8)
            group.step(cache, cache_labels, rows_all[:, lo: lo + B].contiguous(), keep, dropout=col["dropout"], **step_kw)
        tfig = group.epoch_figures()
        vfig = _run_eval(group, cache, cache_labels, val_rows, B)
        for h in range(H):
            out[h]["train_acc"].append(tfig[h]["accuracy"])
            out[h]["train_loss"].append(tfig[h]["loss"])
            out[h]["val_acc"].append(vfig[h]["accuracy"])
            out[h]["val_loss"].append(vfig[h]["loss"])
    for t in out:
        t["best_validation_accuracy"] = max(t["val_acc"]) if t["val_acc"] else float("nan")
    best = max(range(H), key=lambda h: (out[h]["best_validation_accuracy"], -out[h]["val_loss"][-1] if out[h]["val_loss"] else 0.0, -h))
    return {"trials": out, "best_trial": best, "best_params": out[best]["params"], "group": group}


# ---------------------------------------------------------------------------------------------------------------------------------
# a head with one hidden layer: Linear(D, Hd) -> ReLU -> dropout -> Linear(Hd, C)
# ---------------------------------------------------------------------------------------------------------------------------------
def hidden_state_bytes(D: int, Hd: int, C: int, amsgrad: bool = False) -> int:
    """Bytes of the state of a hidden-layer head (`frmap_head_fit_hidden_state_bytes`): `state_bytes` of (D, Hd), then of (Hd, C)."""
    n = int(_lib.load().frmap_head_fit_hidden_state_bytes(int(D), int(Hd), int(C), int(bool(amsgrad))))
    if n == 0:
        raise ValueError(f"head_fit: unsupported D = {D}, Hd = {Hd}, C = {C} (each in 1 ... {MAX_D})")
    return n


def hidden_workspace_bytes(B: int, D: int, Hd: int, C: int) -> int:
    """Bytes of the workspace of a hidden-layer step of ``B`` rows (`frmap_head_fit_hidden_workspace_bytes`)."""
    n = int(_lib.load().frmap_head_fit_hidden_workspace_bytes(int(B), int(D), int(Hd), int(C)))
    if n == 0:
        raise ValueError(f"head_fit: unsupported B = {B}, D = {D}, Hd = {Hd}, C = {C} (B in 1 ... {MAX_B}, D, Hd, C in 1 ... {MAX_D})")
    return n


def hidden_state_views(state: np.ndarray, D: int, Hd: int, C: int, amsgrad: bool = False) -> dict:
    """``{"layer1": state_views of (D, Hd), "layer2": state_views of (Hd, C)}`` into a host copy of a hidden state."""
    raw = np.ascontiguousarray(state).view(np.uint8).reshape(-1)
    n1 = state_bytes(D, Hd, amsgrad)
    return {"layer1": state_views(raw[:n1], D, Hd, amsgrad), "layer2": state_views(raw[n1: n1 + state_bytes(Hd, C, amsgrad)], Hd, C, amsgrad)}


def hidden_workspace_views(workspace: np.ndarray, B: int, Hd: int, C: int) -> dict:
    """h, da [B, Hd] (float32), lab, row_src1 [B] (int32) and z, g, row_loss, row_src (layer 2's `workspace_views`) of a host copy."""
    raw = np.ascontiguousarray(workspace).view(np.uint8).reshape(-1)
    at = 8 * B * Hd
    out = {"h": raw[: 4 * B * Hd].view(np.float32).reshape(B, Hd), "da": raw[4 * B * Hd: at].view(np.float32).reshape(B, Hd),
           "lab": raw[at: at + 4 * B].view(np.int32), "row_src1": raw[at + 4 * B: at + 8 * B].view(np.int32)}
    out.update(workspace_views(raw[at + 8 * B:], B, C))
    return out


def _adam_rule(p, grad, st: dict, km: str, kv: str, kx: str, t: int, lr, beta1, beta2, eps, weight_decay, decoupled, amsgrad, f32):
    """The update of `step_rule` on one tensor; returns the new parameter, ``st`` is updated in place."""
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


def hidden_step_rule(x, labels, w1, b1, w2, b2, state: Optional[dict] = None, rows=None, keep1=None, keep1_scale: float = 1.0, keep2=None,
                     keep2_scale: float = 1.0, *, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                     weight_decay: float = 0.0, label_smoothing: float = 0.0, decoupled: bool = False, amsgrad: bool = False,
                     clear: bool = False, dtype=np.float64, given: Optional[dict] = None, batch: Optional[int] = None) -> dict:
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
    if rows is None:
        rows = np.arange(len(keep1) if keep1 is not None else (len(keep2) if keep2 is not None else (N if batch is None else int(batch))),
                         dtype=np.int64)
    else:
        rows = np.asarray(rows).astype(np.int64)
    B = len(rows)
    state = state or {"layer1": fresh_state(D, Hd, amsgrad, dtype), "layer2": fresh_state(Hd, C, amsgrad, dtype)}
    st1 = {k: (np.array(v, dtype) if isinstance(v, np.ndarray) else int(v)) for k, v in state["layer1"].items()}
    row_src1 = np.full((B,), -1, np.int32)
    for i, r in enumerate(rows):
        if 0 <= r < N and 0 <= labels[r] < C and np.isfinite(x[r]).all():
            row_src1[i] = r
    ok1 = row_src1 >= 0
    lab = np.where(ok1, labels[np.clip(row_src1, 0, N - 1)], -1).astype(np.int32)
    xp = np.zeros((B, D), x.dtype)
    xp[ok1] = x[row_src1[ok1]]
    if keep1 is not None:
        kept = np.asarray(keep1).astype(bool)
        scaled = (xp * F32(keep1_scale)).astype(F32) if f32 else xp * float(keep1_scale)
        xp = np.where(kept, scaled, 0).astype(x.dtype)
        xp[~ok1] = 0
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
        w1 = _adam_rule(w1, dw1, st1, "m_w", "v_w", "vmax_w", **kw)
        b1 = _adam_rule(b1, db1, st1, "m_b", "v_b", "vmax_b", **kw)
    out = {"w1": w1, "b1": b1, "w2": r2["w"], "b2": r2["b"], "state": {"layer1": st1, "layer2": r2["state"]}, "h": h, "lab": lab,
           "row_src1": row_src1, "da": da, "dw1": dw1, "db1": db1, "dw2": r2["dw"], "db2": r2["db"]}
    for k in ("z", "g", "row_loss", "row_src", "n", "loss"):
        out[k] = r2[k]
    return out


def _host_array(op, name, t, dt):
    if not (isinstance(t, np.ndarray) and t.dtype == dt and t.flags.c_contiguous and t.flags.writeable):
        raise ValueError(f"{op}: {name} must be a writable contiguous {np.dtype(dt).name} array")


def hidden_step_host(x, labels, w1, b1, w2, b2, state: np.ndarray, workspace: Optional[np.ndarray] = None, rows=None, keep1=None,
                     keep1_scale: float = 1.0, keep2=None, keep2_scale: float = 1.0, *, lr: float = 1e-3, beta1: float = 0.9,
                     beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0, label_smoothing: float = 0.0,
                     decoupled: bool = False, amsgrad: bool = False, clear: bool = False, given_g: bool = False,
                     batch: Optional[int] = None):
    """The hidden-layer step on the CPU over numpy arrays (`frmap_head_fit_hidden_step_host`; no GPU).  ``w1`` [Hd, D], ``b1`` [Hd],
    ``w2`` [C, Hd], ``b2`` [C] (float32) and ``state`` (uint8, `hidden_state_bytes` bytes, 8-byte aligned) are updated IN PLACE;
    ``workspace`` (uint8, exactly `hidden_workspace_bytes` bytes, or ``None`` for a fresh one) receives h, da, lab, row_src1 and
    layer 2's z, g, row_loss and row_src - with ``given_g`` the z, g and row_loss in it are inputs.  Returns the workspace."""
    op = "head_fit.hidden_step_host"
    x = np.ascontiguousarray(x, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    if x.ndim != 2 or labels.shape != (x.shape[0],):
        raise ValueError(f"{op}: x [N, D] and labels [N] expected")
    N, D = x.shape
    for name, t, dt in (("w1", w1, np.float32), ("b1", b1, np.float32), ("w2", w2, np.float32), ("b2", b2, np.float32),
                        ("state", state, np.uint8)):
        _host_array(op, name, t, dt)
    if w1.ndim != 2 or w1.shape[1] != D or b1.shape != (w1.shape[0],):
        raise ValueError(f"{op}: w1 [Hd, {D}] and b1 [Hd] expected, got {w1.shape} and {b1.shape}")
    Hd = w1.shape[0]
    if w2.ndim != 2 or w2.shape[1] != Hd or b2.shape != (w2.shape[0],):
        raise ValueError(f"{op}: w2 [C, {Hd}] and b2 [C] expected, got {w2.shape} and {b2.shape}")
    C = w2.shape[0]
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        if rows.ndim != 1:
            raise ValueError(f"{op}: rows [B] expected")
    B = len(rows) if rows is not None else (len(keep1) if keep1 is not None else (len(keep2) if keep2 is not None else (
        N if batch is None else int(batch))))
    if keep1 is not None:
        keep1 = np.ascontiguousarray(keep1, dtype=np.uint8)
        if keep1.shape != (B, D):
            raise ValueError(f"{op}: keep1 must be [{B}, {D}], got {keep1.shape}")
    if keep2 is not None:
        keep2 = np.ascontiguousarray(keep2, dtype=np.uint8)
        if keep2.shape != (B, Hd):
            raise ValueError(f"{op}: keep2 must be [{B}, {Hd}], got {keep2.shape}")
    if rows is None and B > N:
        raise ValueError(f"{op}: {B} batch rows without `rows` exceed the {N} cached rows")
    nstate = hidden_state_bytes(D, Hd, C, amsgrad)
    if state.shape != (nstate,) or state.ctypes.data % 8:
        raise ValueError(f"{op}: state must be {nstate} bytes, 8-byte aligned")
    nbytes = hidden_workspace_bytes(B, D, Hd, C)
    if workspace is None:
        if given_g:
            raise ValueError(f"{op}: given_g needs the workspace that holds z, g and row_loss")
        workspace = np.zeros((nbytes,), np.uint8)
    if not (isinstance(workspace, np.ndarray) and workspace.dtype == np.uint8 and workspace.flags.c_contiguous and workspace.flags.writeable
            and workspace.shape == (nbytes,) and workspace.ctypes.data % 4 == 0):
        raise ValueError(f"{op}: workspace must be a writable uint8 array of exactly {nbytes} bytes")
    _lib.check(_lib.load().frmap_head_fit_hidden_step_host(
        x.ctypes.data, labels.ctypes.data, rows.ctypes.data if rows is not None else 0, keep1.ctypes.data if keep1 is not None else 0,
        float(keep1_scale), keep2.ctypes.data if keep2 is not None else 0, float(keep2_scale), w1.ctypes.data, b1.ctypes.data, w2.ctypes.data,
        b2.ctypes.data, state.ctypes.data, workspace.ctypes.data, N, B, D, Hd, C, float(lr), float(beta1), float(beta2), float(eps),
        float(weight_decay), float(label_smoothing), _flags(decoupled, amsgrad, clear), int(bool(given_g))), op)
    return workspace


@ops._on_operand_device
def hidden_step(x: torch.Tensor, labels: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
                state: torch.Tensor, workspace: torch.Tensor, rows: Optional[torch.Tensor] = None, keep1: Optional[torch.Tensor] = None,
                keep1_scale: float = 1.0, keep2: Optional[torch.Tensor] = None, keep2_scale: float = 1.0, *, lr: float = 1e-3,
                beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0, label_smoothing: float = 0.0,
                decoupled: bool = False, amsgrad: bool = False, clear: bool = False, batch: Optional[int] = None) -> None:
    """One hidden-layer training step on the current stream (`frmap_head_fit_hidden_step`; nothing is copied or synchronised).
    ``x`` float32 ``[N, D]``, ``labels`` int32 ``[N]``, ``w1`` ``[Hd, D]``, ``b1`` ``[Hd]``, ``w2`` ``[C, Hd]``, ``b2`` ``[C]`` float32
    (updated in place), ``state`` uint8 of `hidden_state_bytes` bytes (zeros = fresh), ``workspace`` uint8 of exactly
    `hidden_workspace_bytes` bytes, ``rows`` int32 ``[B]`` or ``None`` (rows ``0 .. B-1``; ``B`` is then a mask's row count, else
    ``batch``, else ``N``), ``keep1`` uint8 ``[B, D]`` and ``keep2`` uint8 ``[B, Hd]`` or ``None``.  Every extent that depends on another
    operand is checked here, before the library sees a pointer."""
    op, entry = "head_fit.hidden_step", "frmap_head_fit_hidden_step"
    x = _dev(x, f"{op}.x", torch.float32, (entry, "x"))
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{op}: x [N, D] expected, got {tuple(x.shape)}")
    N, D = int(x.shape[0]), int(x.shape[1])
    _sized(labels, op, "labels", (N,), torch.int32)
    _sized(w1, op, "w1", (w1.shape[0] if isinstance(w1, torch.Tensor) and w1.dim() == 2 else -1, D), torch.float32)
    Hd = int(w1.shape[0])
    _sized(b1, op, "b1", (Hd,), torch.float32)
    _sized(w2, op, "w2", (w2.shape[0] if isinstance(w2, torch.Tensor) and w2.dim() == 2 else -1, Hd), torch.float32)
    C = int(w2.shape[0])
    _sized(b2, op, "b2", (C,), torch.float32)
    if rows is not None:
        if isinstance(rows, torch.Tensor) and rows.dim() != 1:
            raise ValueError(f"{op}: rows [B] expected, got {tuple(rows.shape)}")
        rows = _dev(rows, f"{op}.rows", torch.int32, (entry, "rows"))
        B = int(rows.shape[0])
    elif isinstance(keep1, torch.Tensor) and keep1.dim() == 2:
        B = int(keep1.shape[0])
    elif isinstance(keep2, torch.Tensor) and keep2.dim() == 2:
        B = int(keep2.shape[0])
    else:
        B = N if batch is None else int(batch)
    if rows is None and B > N:
        raise ValueError(f"{op}: {B} batch rows without `rows` exceed the {N} cached rows")
    if keep1 is not None:
        _sized(keep1, op, "keep1", (B, D), torch.uint8)
    if keep2 is not None:
        _sized(keep2, op, "keep2", (B, Hd), torch.uint8)
    _sized(state, op, "state", (hidden_state_bytes(D, Hd, C, amsgrad),), torch.uint8)
    _sized(workspace, op, "workspace", (hidden_workspace_bytes(B, D, Hd, C),), torch.uint8)
    held = []                                                   # copies `_dev` made live until the launch is enqueued
    labels = _dev(labels, f"{op}.labels", torch.int32, (entry, "labels"))
    keep1 = None if keep1 is None else _dev(keep1, f"{op}.keep1", torch.uint8, (entry, "keep1"))
    keep2 = None if keep2 is None else _dev(keep2, f"{op}.keep2", torch.uint8, (entry, "keep2"))
    held += [x, labels, rows, keep1, keep2]
    w1 = _dev(w1, f"{op}.w1", torch.float32, (entry, "w1"), owned=True)
    b1 = _dev(b1, f"{op}.b1", torch.float32, (entry, "b1"), owned=True)
    w2 = _dev(w2, f"{op}.w2", torch.float32, (entry, "w2"), owned=True)
    b2 = _dev(b2, f"{op}.b2", torch.float32, (entry, "b2"), owned=True)
    state = _dev(state, f"{op}.state", torch.uint8, (entry, "state"), owned=True)
    workspace = _dev(workspace, f"{op}.workspace", torch.uint8, (entry, "workspace"), owned=True)
    _lib.check(_lib.load().frmap_head_fit_hidden_step(
        x.data_ptr(), labels.data_ptr(), rows.data_ptr() if rows is not None else 0, keep1.data_ptr() if keep1 is not None else 0,
        float(keep1_scale), keep2.data_ptr() if keep2 is not None else 0, float(keep2_scale), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
        b2.data_ptr(), state.data_ptr(), workspace.data_ptr(), N, B, D, Hd, C, float(lr), float(beta1), float(beta2), float(eps),
        float(weight_decay), float(label_smoothing), _flags(decoupled, amsgrad, clear), _stream()), op)
    del held


class HiddenHead:
    """``Linear(D, Hd) -> ReLU -> dropout -> Linear(Hd, C)`` on the device with its Adam state and a workspace: the ``fc1`` / ``fc2`` of
    the reference's ``BaselineNet`` over its pooled features, or a learned ``D -> Hd`` projection of any cached feature.  Both layers
    are initialised as consecutive ``nn.Linear(D, Hd)`` and ``nn.Linear(Hd, C)`` would be from ``generator`` (a CPU
    ``torch.Generator``; ``None``: torch's default).  `embed` is the new embedding layer: it feeds `matching.Gallery`,
    `evaluate.verification_metrics` and `frames.identify_streams` like any other embedding."""

    def __init__(self, D: int, Hd: int, C: int, device="cuda", amsgrad: bool = False, generator: Optional[torch.Generator] = None):
        self.D, self.Hd, self.C, self.amsgrad = int(D), int(Hd), int(C), bool(amsgrad)
        nbytes = hidden_state_bytes(self.D, self.Hd, self.C, self.amsgrad)          # (refuses a bad shape)
        self.device = torch.device(device)
        params = []
        for fan_out, fan_in in ((self.Hd, self.D), (self.C, self.Hd)):
            bound = 1.0 / math.sqrt(fan_in)
            params.append(((torch.rand((fan_out, fan_in), generator=generator, dtype=torch.float32) * 2 - 1) * bound).to(self.device))
            params.append(((torch.rand((fan_out,), generator=generator, dtype=torch.float32) * 2 - 1) * bound).to(self.device))
        self.w1, self.b1, self.w2, self.b2 = params
        self.state = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        self._state2_at = state_bytes(self.D, self.Hd, self.amsgrad)
        self._workspaces = {}
        self._clear = True

    def _workspace(self, B: int) -> torch.Tensor:
        ws = self._workspaces.get(B)
        if ws is None:
            ws = self._workspaces[B] = torch.empty((hidden_workspace_bytes(B, self.D, self.Hd, self.C),), dtype=torch.uint8, device=self.device)
        return ws

    def new_epoch(self) -> "HiddenHead":
        """The next `step` clears the epoch figures first."""
        self._clear = True
        return self

    def step(self, x: torch.Tensor, labels: torch.Tensor, rows: Optional[torch.Tensor] = None, keep1: Optional[torch.Tensor] = None,
             keep2: Optional[torch.Tensor] = None, *, lr: float, dropout1: float = 0.0, dropout2: float = 0.0,
             keep1_scale: Optional[float] = None, keep2_scale: Optional[float] = None, beta1: float = 0.9, beta2: float = 0.999,
             eps: float = 1e-8, weight_decay: float = 0.0, label_smoothing: float = 0.0, decoupled: bool = False) -> "HiddenHead":
        """One step over rows ``rows`` of the cache ``x`` / ``labels`` (`hidden_step`).  ``keep1`` / ``keep2``: uint8 ``[B, D]`` /
        ``[B, Hd]`` dropout masks on the input / the hidden layer, scaled by ``1 / (1 - dropout1)`` / ``1 / (1 - dropout2)`` unless a
        scale is given.  No synchronisation."""
        if keep1_scale is None:
            keep1_scale = 1.0 / (1.0 - float(dropout1)) if keep1 is not None else 1.0
        if keep2_scale is None:
            keep2_scale = 1.0 / (1.0 - float(dropout2)) if keep2 is not None else 1.0
        B = int(x.shape[0])
        for t, dim in ((rows, 1), (keep1, 2), (keep2, 2)):
            if isinstance(t, torch.Tensor) and t.dim() == dim:
                B = int(t.shape[0])
                break
        hidden_step(x, labels, self.w1, self.b1, self.w2, self.b2, self.state, self._workspace(B), rows, keep1, keep1_scale, keep2,
                    keep2_scale, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, label_smoothing=label_smoothing,
                    decoupled=decoupled, amsgrad=self.amsgrad, clear=self._clear)
        self._clear = False
        return self

    def epoch_figures(self) -> dict:
        """The one host copy (layer 2's header): rows, correct, accuracy and mean loss since the last `new_epoch`, and ``t``."""
        words = self.state[self._state2_at: self._state2_at + 64].cpu().numpy().view(np.uint64)
        out = figures_of({name: words[k] for k, name in enumerate(HEADER)})
        out["t"] = int(words[0])
        return out

    def embed(self, x: torch.Tensor) -> torch.Tensor:
        """``relu(x w1^T + b1)``: the embedding the fitted first layer produces from cached-feature rows ``x`` ``[B, D]``."""
        return ops.linear_f32(x, self.w1, None, self.b1, relu=True)

    def logits(self, x: torch.Tensor) -> torch.Tensor:
        return ops.linear_f32(self.embed(x), self.w2, None, self.b2)

    def state_dict(self) -> dict:
        return {"fc1.weight": self.w1.detach().clone(), "fc1.bias": self.b1.detach().clone(), "fc2.weight": self.w2.detach().clone(),
                "fc2.bias": self.b2.detach().clone()}

    def classifier(self) -> LinearHead:
        """Layer 2 as a `LinearHead` whose ``weight``, ``bias`` and ``state`` are VIEWS of this head's memory (the second part of the
        state is a valid single-step state): its `logits` and `as_classifier` take `embed` outputs."""
        one = LinearHead.__new__(LinearHead)
        one.D, one.C, one.amsgrad, one.device = self.Hd, self.C, self.amsgrad, self.device
        one.weight, one.bias = self.w2, self.b2
        one.state = self.state[self._state2_at: self._state2_at + state_bytes(self.Hd, self.C, self.amsgrad)]
        one._workspaces, one._clear = {}, False
        return one

    def load_into(self, model) -> None:
        """Copy both layers into ``fc1`` / ``fc2`` of a ``BaselineNet`` of matching shapes, in place (the model's plan watches the
        parameters' versions: the next forward rebuilds)."""
        fc1, fc2 = getattr(model, "fc1", None), getattr(model, "fc2", None)
        if type(model).__name__ != "BaselineNet" or not isinstance(fc1, torch.nn.Linear) or not isinstance(fc2, torch.nn.Linear):
            raise ValueError(f"HiddenHead.load_into: a BaselineNet expected, got {type(model).__name__}")
        for name, layer, shape in (("fc1", fc1, (self.Hd, self.D)), ("fc2", fc2, (self.C, self.Hd))):
            if tuple(layer.weight.shape) != shape:
                raise ValueError(f"HiddenHead.load_into: {name} is {list(layer.weight.shape)}, the head's layer is {list(shape)}")
        with torch.no_grad():
            fc1.weight.copy_(self.w1)
            fc1.bias.copy_(self.b1)
            fc2.weight.copy_(self.w2)
            fc2.bias.copy_(self.b2)
