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

Out of scope: gradient clipping, learning-rate schedulers (the caller passes ``lr`` per step), the margin schedule of
``ArcMarginProduct``, anything that trains a convolution.
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


def cache_features(model, model_type: str, data, batch_size: int = 256, device="cuda"):
    """Embed a training set once: ``[N, D]`` float32 features and ``[N]`` int32 labels on the device, through the model's EVAL-mode
    ``get_embedding`` (the deployed trunk; the reference's frozen phase still runs BatchNorm in training mode - DESIGN.md §4).
    ``data``: an image folder (one sub-directory per class) or an iterable of ``(images, labels)`` batches."""
    if model_type == 'siamese':
        raise ValueError("head_fit: a siamese model has no classifier head to fit (pairs are verification_metrics' business)")
    if model.training:
        model.eval()
    feats, labs = [], []
    with torch.no_grad():
        for images, labels in _batches(data, batch_size, device):
            emb = model.get_embedding(images.to(device))
            feats.append(emb.float().reshape(images.shape[0], -1).clone())
            labs.append(torch.as_tensor(labels).to(torch.int64).clamp(-1, 2 ** 31 - 1).to(torch.int32).to(device, non_blocking=True))
    if not feats:
        raise ValueError("head_fit.cache_features: the data set is empty")
    return torch.cat(feats).contiguous(), torch.cat(labs).contiguous()


def fit_head(model, model_type: str, train_data, val_data=None, epochs: int = 10, batch_size: int = 32, lr: float = 1e-3,
             weight_decay: float = 1e-4, dropout: float = 0.1, label_smoothing: float = 0.0, decoupled: bool = False, amsgrad: bool = False,
             generator: Optional[torch.Generator] = None, num_classes: Optional[int] = None, device="cuda"):
    """Fit a `LinearHead` on the frozen model's features.  The training set is embedded once (`cache_features`); every epoch then
    draws a fresh device permutation as ``rows`` and fresh dropout masks from ``generator`` (a generator on ``device``; ``None``:
    the device's default) and steps through it ``batch_size`` rows at a time with no host copy inside the epoch; the epoch's figures
    are one 64-byte copy at its end.  With ``val_data`` every epoch's validation logits go through `evaluate.ClassificationTally`.
    The defaults are the reference's for ``cnn`` (`src/training.py:184, 352`: Adam, lr 1e-3, weight decay 1e-4, Dropout(0.1));
    ``decoupled=True, amsgrad=True, label_smoothing=0.05`` are its ArcFace settings (`:341-348`).  Returns ``(head, history)`` with
    ``history = {"train_loss": [...], "train_acc": [...], "val": [metrics dict per epoch]}``."""
    from . import evaluate
    if model_type == 'siamese':
        raise ValueError("head_fit: a siamese model has no classifier head to fit (pairs are verification_metrics' business)")
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
