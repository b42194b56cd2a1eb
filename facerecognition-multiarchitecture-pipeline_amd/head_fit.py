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

* `pair_step_rule` / `pair_step_host` / `pair_step`, `PairHead`, `draw_pairs`, `cache_embeddings`, `fit_pair_head` - one step of a
  contrastive projection ``x -> normalize(x w^T + b)`` over PAIRS of cached rows (`frmap_head_fit_pair_step`) with the reference's
  ``ContrastiveLoss`` (`src/face_models.py:725-774`): the one objective here trained on distances, and so the fit that accepts a siamese
  model.  ``differ`` is the loss's own label: 1 = different identities, pushed apart.  The reference's ``SiameseDataset`` hands that
  loss 1 for SAME-class pairs; that is not reproduced - callers derive ``differ`` from identity labels (`draw_pairs`).  For a
  ``SiameseNet`` the head is its own last layer ``fc.8`` (`cache_embeddings(layer="fc_hidden")`, `PairHead.load_into`).

* `margin_step_rule` / `margin_step_host` / `margin_step`, `MarginHead`, `margin_schedule`, `fit_margin_head` - one step of the class
  centres of an ArcFace margin head (`frmap_head_fit_margin_step`): the reference's ``ArcMarginProduct`` in training mode
  (`src/face_models.py:297-429`) under cross-entropy, the objective the flagship model is trained with, over cached normalised
  embeddings (`cache_embeddings`).  The step takes the effective scale and margin as scalars; the warm-up schedule that produces them is
  host arithmetic (`margin_schedule`).  `MarginHead.load_into` writes ``arcface.weight`` of an ``ArcFaceNet``, which
  `evaluate.evaluate_model`, `evaluate_stream` and `arcface_validate` score against.

* `embed_step_rule` / `embed_step_host` / `embed_step`, `EmbedHead`, `fit_embed_head` - one step of the embedding layer of an
  ``ArcFaceNet`` with the trunk frozen (`frmap_head_fit_embed_step`): ``Linear(512, 512, bias=False)`` -> ``BatchNorm1d`` in TRAINING
  mode (batch statistics, running statistics and its backward pass) -> dropout -> normalize -> the margin head -> cross-entropy, one
  Adam over ``embedding.weight``, ``bn.weight``, ``bn.bias`` and ``arcface.weight`` - the first phase of the reference's two-phase
  ArcFace training (`src/training.py:374-377, 683-700`) over cached POOLED trunk features (`cache_features(layer="pooled")`,
  `ArcFaceNet.pooled_features`).  `EmbedHead.embed` is the deployed arithmetic (running statistics); `EmbedHead.load_into` writes the
  six tensors, after which the model's own ``get_embedding`` produces the fitted embedding.

Structure: the steps differ in their operands, and everything around the operands exists once.  The numpy rules - the specification -
are `head_fit_rules`, which imports neither torch nor the library; every name of it is re-exported here.  `_size` stands behind the size
functions.  `_cache`, `_layer`, `_batch`, `_mask`, `_buffers` and `_reads` are the operand walk of the device steps and `_host_cache`,
`_host_layer`, `_host_batch`, `_host_mask` and `_host_buffers` that of the host steps: every size is checked before the first operand is
converted, after which a step calls the library, its Adam scalars from `_adam`.  `_Head` holds the workspace cache, the pending clear,
the epoch figures, the default mask scale and the batch-row count of every head; `_linear_init` and `_margin_init` are their draws,
`_arcface_parts` and `_load` what their `load_into` methods share, and `LinearHead._over` makes a head of views.  `_fit` is the one epoch
loop (history, `new_epoch`, `epoch_figures`, the validation hook) and `_row_epochs` the row-based epoch (a permutation, one mask per
``(width, dropout)`` spec, `head.step`) of `fit_head`, `fit_margin_head` and `fit_embed_head`; `fit_pair_head` brings its own epoch to
`_fit`.  The ORDER OF DRAWS of a fit is behaviour and stands in its docstring: `fit_head` draws the head first, the others the seed.

Out of scope: groups of hidden heads, more than one hidden layer, gradient clipping, learning-rate schedulers (the caller passes ``lr`` per step), groups of margin and embedding heads, training-mode BatchNorm in the trunk, the reference's backward-hook gradient clipping, triplet loss, in-batch mining and groups of pair heads, anything that trains a convolution, Optuna's sampler, pruner and schedulers (the caller supplies the trials).
"""
from __future__ import annotations

import math
import os
from typing import Optional

import numpy as np
import torch

from . import _lib, ops
from .head_fit_rules import (CHAIN, DIST_EPS, DIST_MIN, F32, LOSS_CLAMP, LOSS_SCALE, MARGIN_CAP, MARGIN_HI, MARGIN_RMAX,  # noqa: F401
                             NORM_EPS, _adam_rule, _copy_state, _powi, _rule_batch, adam32, adam_scalars32, dot32, embed_fresh_state,
                             embed_step_rule, fma32, fresh_state, group_step_rule, hidden_step_rule, loss_q, margin_logits_rule,
                             margin_schedule, margin_step_rule, pair_loss_rule, pair_step_rule, step_rule)
from .ops import _dev, _sized, _stream

MAX_C = MAX_D = 65536
MAX_B = 1 << 20
DECOUPLED, AMSGRAD, CLEAR = 1, 2, 4
EVAL = 8                          # grouped step only: figures, no update
MAX_H = 4096                      # heads of one group
HYPER_COLUMNS = ("lr", "beta1", "beta2", "eps", "weight_decay", "label_smoothing", "keep_scale")     # of the [H, 8] table; column 7 is 0
HEADER = ("t", "n", "rows", "correct", "loss_q")     # words 0 .. 4 of the 8-word header


# ---------------------------------------------------------------------------------------------------------------------------------
# sizes and layouts
# ---------------------------------------------------------------------------------------------------------------------------------
_H_IN, _B_IN, _DC_IN = f"H in 1 ... {MAX_H}, ", f"B in 1 ... {MAX_B}, ", f"D in 1 ... {MAX_D}, C in 1 ... {MAX_C}"


def _size(entry: str, limits: str, names: str, *args) -> int:
    """What the library's size function ``entry(*args)`` returns; 0 is a shape the launcher refuses: ``names`` are the extents among
    ``args`` that the message gives, ``limits`` what it says of them."""
    n = int(getattr(_lib.load(), entry)(*args))
    if n == 0:
        raise ValueError("head_fit: unsupported " + ", ".join(f"{k} = {v}" for k, v in zip(names.split(), args)) + f" ({limits})")
    return n


def state_bytes(D: int, C: int, amsgrad: bool = False) -> int:
    """Bytes of an optimiser state (`frmap_head_fit_state_bytes`); ``ValueError`` for a shape the launcher refuses."""
    return _size("frmap_head_fit_state_bytes", _DC_IN, "D C", int(D), int(C), int(bool(amsgrad)))


def workspace_bytes(B: int, D: int, C: int) -> int:
    """Bytes of the workspace of a step of ``B`` rows (`frmap_head_fit_workspace_bytes`)."""
    return _size("frmap_head_fit_workspace_bytes", _B_IN + _DC_IN, "B D C", int(B), int(D), int(C))


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
# the host twin
# ---------------------------------------------------------------------------------------------------------------------------------
def _flags(decoupled, amsgrad, clear) -> int:
    return (DECOUPLED if decoupled else 0) | (AMSGRAD if amsgrad else 0) | (CLEAR if clear else 0)


def _adam(lr, beta1, beta2, eps, weight_decay):
    """The five Adam scalars as every step, host or device, hands them to the library by value."""
    return float(lr), float(beta1), float(beta2), float(eps), float(weight_decay)


def _host_cache(op, x, labels):
    """``(x, labels, N, D)`` of a host step: the cache as contiguous float32 ``[N, D]`` and int32 ``[N]`` (``labels=None``: a step
    that reads no labels)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if labels is None:
        if x.ndim != 2:
            raise ValueError(f"{op}: x [N, D] expected")
        return x, None, x.shape[0], x.shape[1]
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    if x.ndim != 2 or labels.shape != (x.shape[0],):
        raise ValueError(f"{op}: x [N, D] and labels [N] expected")
    return x, labels, x.shape[0], x.shape[1]


def _host_array(op, name, t, dt):
    if not (isinstance(t, np.ndarray) and t.dtype == dt and t.flags.c_contiguous and t.flags.writeable):
        raise ValueError(f"{op}: {name} must be a writable contiguous {np.dtype(dt).name} array")


def _host_layer(op, wname, bname, w, b, lead, fan_out, fan_in):
    """The leading extents of ``w [*lead, fan_out, fan_in]`` with ``b [*lead, fan_out]``, both writable float32 (``lead``, ``fan_out``:
    the letters of the message)."""
    _host_array(op, wname, w, np.float32)
    _host_array(op, bname, b, np.float32)
    if w.ndim != len(lead) + 2 or w.shape[-1] != fan_in or b.shape != w.shape[:-1]:
        at = "".join(k + ", " for k in lead) + fan_out
        raise ValueError(f"{op}: {wname} [{at}, {fan_in}] and {bname} [{at}] expected, got {w.shape} and {b.shape}")
    return w.shape[:-1]


def _host_batch(op, N, rows, masks, batch):
    """``(rows, B)`` of a single-head host step: ``rows`` as int32 ``[B]``; without it B is the first mask's row count, else
    ``batch``, else N, and at most N."""
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        if rows.ndim != 1:
            raise ValueError(f"{op}: rows [B] expected")
        return rows, len(rows)
    B = next((len(m) for m in masks if m is not None), N if batch is None else int(batch))
    if B > N:
        raise ValueError(f"{op}: {B} batch rows without `rows` exceed the {N} cached rows")
    return None, B


def _host_mask(op, name, keep, shape):
    if keep is None:
        return None
    keep = np.ascontiguousarray(keep, dtype=np.uint8)
    if keep.shape != shape:
        raise ValueError(f"{op}: {name} must be {list(shape)}, got {keep.shape}")
    return keep


def _host_buffers(op, state, nstate, workspace, nbytes, given_g):
    """The state is ``nstate`` bytes, 8-byte aligned; the workspace exactly ``nbytes`` bytes, 4-byte aligned, or ``None`` for a fresh
    one, which ``given_g`` cannot take.  Returns the workspace."""
    _host_array(op, "state", state, np.uint8)
    if state.shape != (nstate,) or state.ctypes.data % 8:
        raise ValueError(f"{op}: state must be {nstate} bytes, 8-byte aligned")
    if workspace is None:
        if given_g:
            raise ValueError(f"{op}: given_g needs the workspace that holds z, g and row_loss")
        workspace = np.zeros((nbytes,), np.uint8)
    if not (isinstance(workspace, np.ndarray) and workspace.dtype == np.uint8 and workspace.flags.c_contiguous and workspace.flags.writeable
            and workspace.shape == (nbytes,) and workspace.ctypes.data % 4 == 0):
        raise ValueError(f"{op}: workspace must be a writable uint8 array of exactly {nbytes} bytes")
    return workspace


def _at(a) -> int:
    """The address of a host array, 0 for ``None``."""
    return 0 if a is None else a.ctypes.data


def step_host(x, labels, w, b, state: np.ndarray, workspace: Optional[np.ndarray] = None, rows=None, keep=None, keep_scale: float = 1.0, *,
              lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0,
              label_smoothing: float = 0.0, decoupled: bool = False, amsgrad: bool = False, clear: bool = False, given_g: bool = False,
              batch: Optional[int] = None):
    """The step on the CPU over numpy arrays (`frmap_head_fit_step_host`: the kernels' rule header compiled for the host; no GPU).
    ``w`` [C, D], ``b`` [C] (float32) and ``state`` (uint8, `state_bytes` bytes) are updated IN PLACE; ``workspace`` (uint8, exactly
    `workspace_bytes` bytes, or ``None`` for a fresh one) receives z, g, row_loss and row_src - with ``given_g`` its z, g and
    row_loss are inputs.  ``batch``: B when neither ``rows`` nor ``keep`` gives it (default N).  Returns the workspace."""
    op = "head_fit.step_host"
    x, labels, N, D = _host_cache(op, x, labels)
    C, = _host_layer(op, "w", "b", w, b, "", "C", D)
    rows, B = _host_batch(op, N, rows, (keep,), batch)
    keep = _host_mask(op, "keep", keep, (B, D))
    workspace = _host_buffers(op, state, state_bytes(D, C, amsgrad), workspace, workspace_bytes(B, D, C), given_g)
    _lib.check(_lib.load().frmap_head_fit_step_host(_at(x), _at(labels), _at(rows), _at(keep), float(keep_scale), _at(w), _at(b), _at(state),
                                                    _at(workspace), N, B, D, C, *_adam(lr, beta1, beta2, eps, weight_decay),
                                                    float(label_smoothing), _flags(decoupled, amsgrad, clear), int(bool(given_g))), op)
    return workspace


# ---------------------------------------------------------------------------------------------------------------------------------
# the step on the device
# ---------------------------------------------------------------------------------------------------------------------------------
def _cache(op, entry, x, labels):
    """``(x, N, D)`` of a device step: the cache ``x`` as the library takes it, float32 ``[N, D]``, with ``labels`` int32 ``[N]``
    (``None``: a step that reads no labels)."""
    x = _dev(x, f"{op}.x", torch.float32, (entry, "x"))
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{op}: x [N, D] expected, got {tuple(x.shape)}")
    N, D = int(x.shape[0]), int(x.shape[1])
    if labels is not None:
        _sized(labels, op, "labels", (N,), torch.int32)
    return x, N, D


def _layer(w, b, op, wname, bname, fan_in) -> int:
    """``fan_out`` of a layer ``w [fan_out, fan_in]``, ``b [fan_out]`` (float32)."""
    _sized(w, op, wname, (w.shape[0] if isinstance(w, torch.Tensor) and w.dim() == 2 else -1, fan_in), torch.float32)
    _sized(b, op, bname, (int(w.shape[0]),), torch.float32)
    return int(w.shape[0])


def _batch(op, entry, N, rows, masks, batch):
    """``(rows, B)`` of a single-head device step: ``rows`` int32 ``[B]`` as the library takes it; without it the rows are
    ``0 .. B-1`` with B the first ``[B, .]`` mask's row count, else ``batch``, else N, and at most N."""
    if rows is not None:
        if isinstance(rows, torch.Tensor) and rows.dim() != 1:
            raise ValueError(f"{op}: rows [B] expected, got {tuple(rows.shape)}")
        rows = _dev(rows, f"{op}.rows", torch.int32, (entry, "rows"))
        return rows, int(rows.shape[0])
    B = N if batch is None else int(batch)
    for m in masks:
        if isinstance(m, torch.Tensor) and m.dim() == 2:
            B = int(m.shape[0])
            break
    if B > N:
        raise ValueError(f"{op}: {B} batch rows without `rows` exceed the {N} cached rows")
    return None, B


def _operand(t, op, entry, name, dtype, owned=False):
    """`_dev` of the operand ``name`` (``None`` stays ``None``).  A read-only operand may come back as a copy, which the caller's name
    for it holds until the launch is enqueued; an ``owned`` one - the call writes it - is refused instead."""
    return None if t is None else _dev(t, f"{op}.{name}", dtype, (entry, name), owned=owned)


def _mask(op, name, keep, shape):
    """An optional uint8 dropout mask is exactly ``shape`` (the device side of `_host_mask`)."""
    if keep is not None:
        _sized(keep, op, name, shape, torch.uint8)


def _buffers(op, entry, state, nstate, workspace, nbytes, **written):
    """The device side of `_host_buffers`, last of a step's size checks: the state is uint8 of ``nstate`` bytes, the workspace of exactly
    ``nbytes``.  Then `_operand` of both and of every other named tensor the call writes: none is copied, the caller's are the operands."""
    _sized(state, op, "state", (nstate,), torch.uint8)
    _sized(workspace, op, "workspace", (nbytes,), torch.uint8)
    for name, t in dict(written, state=state, workspace=workspace).items():
        _operand(t, op, entry, name, None, True)


def _reads(op, entry, **named):
    """`_operand` of every named operand the call only reads, in the order given; `_sized` has checked its dtype and extent."""
    return [_operand(t, op, entry, name, None) for name, t in named.items()]


def _dev_at(t) -> int:
    return 0 if t is None else t.data_ptr()


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
    op, entry = "head_fit.step", "frmap_head_fit_step"
    x, N, D = _cache(op, entry, x, labels)
    C = _layer(w, b, op, "w", "b", D)
    rows, B = _batch(op, entry, N, rows, (keep,), batch)
    _mask(op, "keep", keep, (B, D))
    _buffers(op, entry, state, state_bytes(D, C, amsgrad), workspace, workspace_bytes(B, D, C), w=w, b=b)
    labels, keep = _reads(op, entry, labels=labels, keep=keep)
    _lib.check(_lib.load().frmap_head_fit_step(x.data_ptr(), labels.data_ptr(), _dev_at(rows), _dev_at(keep), float(keep_scale), w.data_ptr(),
                                               b.data_ptr(), state.data_ptr(), workspace.data_ptr(), N, B, D, C,
                                               *_adam(lr, beta1, beta2, eps, weight_decay), float(label_smoothing),
                                               _flags(decoupled, amsgrad, clear), _stream()), op)


def _linear_init(fan_out: int, fan_in: int, generator):
    """``(w, b)`` of an ``nn.Linear(fan_in, fan_out)`` on the CPU (Kaiming-uniform with a = sqrt(5): both uniform in ±1/sqrt(fan_in)),
    two draws from ``generator``, the weight first."""
    bound = 1.0 / math.sqrt(fan_in)
    w = (torch.rand((fan_out, fan_in), generator=generator, dtype=torch.float32) * 2 - 1) * bound
    b = (torch.rand((fan_out,), generator=generator, dtype=torch.float32) * 2 - 1) * bound
    return w, b


def _margin_init(C: int, D: int, generator):
    """The ``[C, D]`` class centres of an ``ArcMarginProduct`` on the CPU (``xavier_normal_`` with gain sqrt(2),
    `src/face_models.py:326`): one draw from ``generator``."""
    std = math.sqrt(2.0) * math.sqrt(2.0 / (D + C))
    return torch.empty((C, D), dtype=torch.float32).normal_(0.0, std, generator=generator)


def _arcface_parts(who: str, model):
    """``(embedding, bn, arcface)`` of an ``ArcFaceNet``; any other class, and one without these modules, is refused in ``who``'s name."""
    emb, bn, arc = (getattr(model, k, None) for k in ("embedding", "bn", "arcface"))
    if type(model).__name__ != "ArcFaceNet" or not isinstance(emb, torch.nn.Linear) or not isinstance(bn, torch.nn.BatchNorm1d) or \
            not isinstance(getattr(arc, "weight", None), torch.Tensor):
        raise ValueError(f"{who}: an ArcFaceNet expected, got {type(model).__name__}")
    return emb, bn, arc


def _load(who: str, mine: str, pairs) -> None:
    """What the `load_into` methods share: every ``(name, dst, src)`` of ``pairs`` has equal shapes - else ``"<who>: <name> is <dst's>,
    <mine> is <src's>"`` -, and only then every ``src`` is copied into its ``dst``, outside autograd.  ``name=None``: a bias, unchecked."""
    for name, dst, src in pairs:
        if name is not None and (not isinstance(dst, torch.Tensor) or tuple(dst.shape) != tuple(src.shape)):
            raise ValueError(f"{who}: {name} is {list(dst.shape) if isinstance(dst, torch.Tensor) else None}, {mine} is {list(src.shape)}")
    with torch.no_grad():
        for _, dst, src in pairs:
            dst.copy_(src)


def _figures(words) -> dict:
    """`figures_of` the 8 words of a state's header, and the step count ``t``."""
    out = figures_of({name: words[k] for k, name in enumerate(HEADER)})
    out["t"] = int(words[0])
    return out


class _Head:
    """What the heads share: ``state`` on ``device``, a workspace per batch size (`_workspace_bytes` is the head's own), the pending
    clear of the epoch figures, and their one host copy.  ``_header_at``: where the 64-byte header with the figures sits in ``state``."""
    _header_at = 0

    def _start(self, state: torch.Tensor, device, clear: bool = True):
        self.state, self.device, self._workspaces, self._clear = state, device, {}, clear

    def _workspace(self, B: int) -> torch.Tensor:
        ws = self._workspaces.get(B)
        if ws is None:
            ws = self._workspaces[B] = torch.empty((self._workspace_bytes(B),), dtype=torch.uint8, device=self.device)
        return ws

    def new_epoch(self):
        """The next `step` (or `evaluate`) clears the epoch figures first."""
        self._clear = True
        return self

    def _run(self, fn, *operands, **kw):
        """One library step ``fn`` with the head's ``amsgrad`` and its pending clear, which only an accepted call spends."""
        fn(*operands, amsgrad=self.amsgrad, clear=self._clear, **kw)
        self._clear = False
        return self

    def epoch_figures(self) -> dict:
        """The one host copy: rows, correct, accuracy and mean loss since the last `new_epoch`, and the step count ``t``."""
        return _figures(self.state[self._header_at: self._header_at + 64].cpu().numpy().view(np.uint64))

    @staticmethod
    def _keep_scale(keep_scale, keep, dropout):
        """The scale of the mask ``keep``: ``keep_scale`` when given, else ``1 / (1 - dropout)`` with a mask and 1 without one."""
        return keep_scale if keep_scale is not None else (1.0 / (1.0 - float(dropout)) if keep is not None else 1.0)

    @staticmethod
    def _batch_rows(x, rows, *masks) -> int:
        """B of a row-based step: ``rows``' length, else the first ``[B, .]`` mask's row count, else ``x``'s."""
        for t, dim in ((rows, 1),) + tuple((m, 2) for m in masks):
            if isinstance(t, torch.Tensor) and t.dim() == dim:
                return int(t.shape[0])
        return int(x.shape[0])


class LinearHead(_Head):
    """A linear softmax classifier ``[C, D]`` on the device with its Adam state and a workspace.  ``weight`` / ``bias`` are
    initialised as ``nn.Linear`` does (Kaiming-uniform with a = sqrt(5): both uniform in ±1/sqrt(D)) from ``generator`` (a CPU
    ``torch.Generator``; ``None``: torch's default)."""

    def __init__(self, D: int, C: int, device="cuda", amsgrad: bool = False, generator: Optional[torch.Generator] = None):
        nbytes = state_bytes(int(D), int(C), bool(amsgrad))          # (refuses a bad shape)
        w, b = _linear_init(int(C), int(D), generator)
        device = torch.device(device)
        self._adopt(w.to(device), b.to(device), torch.zeros((nbytes,), dtype=torch.uint8, device=device), amsgrad, device, True)

    def _adopt(self, weight, bias, state, amsgrad, device, clear):
        self.C, self.D, self.amsgrad = int(weight.shape[0]), int(weight.shape[1]), bool(amsgrad)
        self.weight, self.bias = weight, bias
        self._start(state, device, clear)

    @classmethod
    def _over(cls, weight, bias, state, amsgrad, device) -> "LinearHead":
        """A head whose ``weight`` ``[C, D]``, ``bias`` and ``state`` are the given tensors - views of a larger head's memory - with no
        clear pending."""
        one = cls.__new__(cls)
        one._adopt(weight, bias, state, amsgrad, device, False)
        return one

    def _workspace_bytes(self, B: int) -> int:
        return workspace_bytes(B, self.D, self.C)

    def step(self, x: torch.Tensor, labels: torch.Tensor, rows: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None, *,
             lr: float, keep_scale: Optional[float] = None, dropout: float = 0.0, beta1: float = 0.9, beta2: float = 0.999,
             eps: float = 1e-8, weight_decay: float = 0.0, label_smoothing: float = 0.0, decoupled: bool = False) -> "LinearHead":
        """One step over rows ``rows`` of the cache ``x`` / ``labels`` (`step`).  ``keep``: a uint8 ``[B, D]`` dropout mask, scaled by
        ``keep_scale`` (default ``1 / (1 - dropout)``).  No synchronisation."""
        return self._run(step, x, labels, self.weight, self.bias, self.state, self._workspace(self._batch_rows(x, rows, keep)), rows, keep,
                         self._keep_scale(keep_scale, keep, dropout), lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay,
                         label_smoothing=label_smoothing, decoupled=decoupled)

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
        _load("LinearHead.load_into", "the head", ((None, fc[1].weight, self.weight), (None, fc[1].bias, self.bias)))

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
    ``layer="pooled"`` (``BaselineNet`` and ``ArcFaceNet`` only): cache the ``[N, 128]`` input of ``fc1`` (`BaselineNet.pooled_features`)
    instead, for a `HiddenHead` that fits ``fc1`` and ``fc2``, or the ``[N, 512]`` input of ``embedding`` (`ArcFaceNet.pooled_features`),
    for an `EmbedHead` that fits ``embedding``, ``bn`` and the class centres."""
    if model_type == 'siamese':
        raise ValueError("head_fit: a siamese model has no classifier head to fit (pairs are verification_metrics' business)")
    if layer not in ("embedding", "pooled"):
        raise ValueError(f"head_fit.cache_features: layer must be 'embedding' or 'pooled', got {layer!r}")
    if layer == "pooled" and type(model).__name__ not in ("BaselineNet", "ArcFaceNet"):
        raise ValueError(f"head_fit.cache_features: layer='pooled' is BaselineNet's (the input of its fc1) and ArcFaceNet's (the input of "
                         f"its embedding), got {type(model).__name__}")
    return _cache_rows("head_fit.cache_features", model, model.pooled_features if layer == "pooled" else model.get_embedding, data,
                       batch_size, device)


def _cache_rows(op, model, embed, data, batch_size, device):
    """The loop of `cache_features` and `cache_embeddings`: ``embed`` of every batch of ``data`` in eval mode, as float32 ``[N, D]``
    with the labels as int32 ``[N]``, both on the device."""
    if model.training:
        model.eval()
    feats, labs = [], []
    with torch.no_grad():
        for images, labels in _batches(data, batch_size, device):
            emb = embed(images.to(device))
            feats.append(emb.float().reshape(images.shape[0], -1).clone())
            labs.append(torch.as_tensor(labels).to(torch.int64).clamp(-1, 2 ** 31 - 1).to(torch.int32).to(device, non_blocking=True))
    if not feats:
        raise ValueError(f"{op}: the data set is empty")
    return torch.cat(feats).contiguous(), torch.cat(labs).contiguous()


def cache_embeddings(model, data, batch_size: int = 256, device="cuda", layer: str = "embedding"):
    """`cache_features` for a head that needs no classifier - a `PairHead` - and so for a siamese model too: ``[N, D]`` float32 rows and
    ``[N]`` int32 identity labels on the device.  ``layer="embedding"``: the model's ``get_embedding``; ``layer="fc_hidden"``
    (``SiameseNet`` only): the ``[N, 512]`` input of its last layer ``fc.8`` (`SiameseNet.fc_hidden_features`), so that a
    ``PairHead(512, 256)`` fits that layer itself (`PairHead.load_into`)."""
    if layer not in ("embedding", "fc_hidden"):
        raise ValueError(f"head_fit.cache_embeddings: layer must be 'embedding' or 'fc_hidden', got {layer!r}")
    if layer == "fc_hidden" and type(model).__name__ != "SiameseNet":
        raise ValueError(f"head_fit.cache_embeddings: layer='fc_hidden' is SiameseNet's (the input of its fc.8), got {type(model).__name__}")
    return _cache_rows("head_fit.cache_embeddings", model, model.fc_hidden_features if layer == "fc_hidden" else model.get_embedding, data,
                       batch_size, device)


def _head_generator(generator):
    """The generator heads are drawn from: ``generator`` when it is a CPU one, else torch's default (``None``)."""
    return generator if generator is not None and generator.device.type == "cpu" else None


def _generators(generator, device):
    """``(_head_generator, the device generator of permutations and masks)``: ``generator`` itself when it lives on a device; for a CPU
    one a fresh generator on ``device`` seeded by ONE ``randint(0, 2**62)`` draw from it, taken here; ``None`` for ``None``."""
    dev_gen = generator if generator is not None and generator.device.type != "cpu" else None
    if generator is not None and dev_gen is None:
        dev_gen = torch.Generator(device=device)
        dev_gen.manual_seed(int(torch.randint(0, 2 ** 62, (1,), generator=generator).item()))
    return _head_generator(generator), dev_gen


def _fit(head, epochs, run_epoch, validate=None):
    """The epoch loop of every fit.  Per epoch: `new_epoch`, ``run_epoch(epoch)`` - the steps, with no host copy -, the one copy of the
    epoch's figures and, with ``validate``, ``validate(head)`` as its entry of ``history["val"]``.  Returns ``(head, history)``; no draws."""
    history = {"train_loss": [], "train_acc": [], "val": []}
    for epoch in range(int(epochs)):
        head.new_epoch()
        run_epoch(epoch)
        fig = head.epoch_figures()
        history["train_loss"].append(fig["loss"])
        history["train_acc"].append(fig["accuracy"])
        if validate is not None:
            history["val"].append(validate(head))
    return head, history


def _row_epochs(head, feats, labels, batch_size, masks, dev_gen, step_kw):
    """The ``run_epoch`` of a row-based fit.  Per epoch ``step_kw(epoch)``, the keyword arguments of that epoch's steps, then ONE
    ``randperm`` of the cached rows from ``dev_gen``; per batch of ``batch_size`` permuted rows (the last one may be shorter) one
    ``rand`` per ``(width, p)`` of ``masks``, in their order - none for ``p == 0``, where the mask is ``None`` -, then `head.step`."""
    N, B = int(feats.shape[0]), int(batch_size)

    def run_epoch(epoch):
        kw = step_kw(epoch)
        perm = torch.randperm(N, device=feats.device, generator=dev_gen).to(torch.int32)
        for lo in range(0, N, B):
            rows = perm[lo: lo + B]
            keeps = [(torch.rand((rows.shape[0], width), device=feats.device, generator=dev_gen) >= p).to(torch.uint8) if p > 0 else None
                     for width, p in masks]
            head.step(feats, labels, rows, *keeps, **kw)
    return run_epoch


def _tally(C, logits, labels) -> dict:
    """The validation of a classifier fit: the metrics of an `evaluate.ClassificationTally` over ``logits`` and ``labels``."""
    from . import evaluate
    tally = evaluate.ClassificationTally(C, device=logits.device)
    tally.update(logits, labels)
    return tally.metrics()


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
    every other model it is the embedding, and ``w1`` a learned projection of it.

    Order of draws: the head from the CPU ``generator`` FIRST, then the device generator's seed from it (`fit_margin_head`,
    `fit_embed_head` and `fit_pair_head` draw the seed first: the two orders differ and both are kept, since either change would alter
    every fitted head of a given seed); per epoch one ``randperm``; per batch the input mask's ``rand``, then the hidden mask's; a mask
    with ``p == 0`` is not drawn."""
    if model_type == 'siamese':
        raise ValueError("head_fit: a siamese model has no classifier head to fit (pairs are verification_metrics' business)")
    layer = "pooled" if hidden is not None and type(model).__name__ == "BaselineNet" else "embedding"
    feats, labels = cache_features(model, model_type, train_data, device=device, layer=layer)
    D = int(feats.shape[1])
    C = int(num_classes) if num_classes is not None else int(labels.max().item()) + 1
    if hidden is None:
        head = LinearHead(D, C, feats.device, amsgrad=amsgrad, generator=_head_generator(generator))
        masks, drop_kw = [(D, dropout)], dict(dropout=dropout)
    else:
        hidden, hidden_dropout = int(hidden), float(hidden_dropout)
        head = HiddenHead(D, hidden, C, feats.device, amsgrad=amsgrad, generator=_head_generator(generator))
        masks, drop_kw = [(D, dropout), (hidden, hidden_dropout)], dict(dropout1=dropout, dropout2=hidden_dropout)
    dev_gen = _generators(generator, feats.device)[1]
    val = cache_features(model, model_type, val_data, device=device, layer=layer) if val_data is not None else None
    kw = dict(lr=lr, weight_decay=weight_decay, label_smoothing=label_smoothing, decoupled=decoupled, **drop_kw)
    return _fit(head, epochs, _row_epochs(head, feats, labels, batch_size, masks, dev_gen, lambda epoch: kw),
                None if val is None else lambda head: _tally(C, head.logits(val[0]), val[1]))


# ---------------------------------------------------------------------------------------------------------------------------------
# groups of heads: H independent heads over one cache, advanced by one call
# ---------------------------------------------------------------------------------------------------------------------------------
def group_state_stride(D: int, C: int, amsgrad: bool = False) -> int:
    """Bytes from head h's state to head h + 1's (`frmap_head_fit_group_state_stride`): `state_bytes` rounded up to 8."""
    return _size("frmap_head_fit_group_state_stride", _DC_IN, "D C", int(D), int(C), int(bool(amsgrad)))


def group_state_bytes(H: int, D: int, C: int, amsgrad: bool = False) -> int:
    """Bytes of the states of ``H`` heads (`frmap_head_fit_group_state_bytes`): ``H`` strides."""
    return _size("frmap_head_fit_group_state_bytes", _H_IN + _DC_IN, "H D C", int(H), int(D), int(C), int(bool(amsgrad)))


def group_workspace_bytes(H: int, B: int, D: int, C: int) -> int:
    """Bytes of the workspaces of ``H`` heads stepping ``B`` rows each (`frmap_head_fit_group_workspace_bytes`)."""
    return _size("frmap_head_fit_group_workspace_bytes", _H_IN + _B_IN + _DC_IN, "H B D C", int(H), int(B), int(D), int(C))


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


def group_step_host(x, labels, rows, hyper, w, b, state: np.ndarray, workspace: Optional[np.ndarray] = None, keep=None, *,
                    decoupled: bool = False, amsgrad: bool = False, clear: bool = False, evaluate: bool = False, given_g: bool = False):
    """The grouped step on the CPU over numpy arrays (`frmap_head_fit_group_step_host`: the single host step looped over the heads).
    ``rows`` int32 ``[H, B]``, ``hyper`` float32 ``[H, 8]`` (`hyper_table`), ``w`` ``[H, C, D]``, ``b`` ``[H, C]`` and ``state`` (uint8,
    `group_state_bytes` bytes, 8-byte aligned) are updated IN PLACE; ``workspace`` (uint8, exactly `group_workspace_bytes` bytes, or
    ``None`` for a fresh one) receives every head's z, g, row_loss and row_src; ``keep`` uint8 ``[H, B, D]`` or ``None``.  Returns the
    workspace."""
    op = "head_fit.group_step_host"
    x, labels, N, D = _host_cache(op, x, labels)
    H, C = _host_layer(op, "w", "b", w, b, "H", "C", D)
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
    if keep is not None and evaluate:
        raise ValueError(f"{op}: keep cannot be given with evaluate=True")
    keep = _host_mask(op, "keep", keep, (H, B, D))
    workspace = _host_buffers(op, state, group_state_bytes(H, D, C, amsgrad), workspace, group_workspace_bytes(H, B, D, C), given_g)
    _lib.check(_lib.load().frmap_head_fit_group_step_host(_at(x), _at(labels), _at(rows), _at(keep), _at(hyper), _at(w), _at(b), _at(state),
                                                          _at(workspace), N, H, B, D, C, _group_flags(decoupled, amsgrad, clear, evaluate),
                                                          int(bool(given_g))), op)
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
    x, N, D = _cache(op, entry, x, labels)
    if not isinstance(w, torch.Tensor) or w.dim() != 3:
        raise ValueError(f"{op}: w [H, C, D] expected, got {tuple(w.shape) if isinstance(w, torch.Tensor) else type(w).__name__}")
    H, C = int(w.shape[0]), int(w.shape[1])
    _sized(w, op, "w", (H, C, D), torch.float32)
    _sized(b, op, "b", (H, C), torch.float32)
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2:
        raise ValueError(f"{op}: rows [H, B] expected, got {tuple(rows.shape) if isinstance(rows, torch.Tensor) else type(rows).__name__}")
    B = int(rows.shape[1])
    _sized(rows, op, "rows", (H, B), torch.int32)
    _sized(hyper, op, "hyper", (H, 8), torch.float32)
    if keep is not None and evaluate:
        raise ValueError(f"{op}: keep cannot be given with evaluate=True (flag 8 takes no dropout mask)")
    _mask(op, "keep", keep, (H, B, D))
    _buffers(op, entry, state, group_state_bytes(H, D, C, amsgrad), workspace, group_workspace_bytes(H, B, D, C), w=w, b=b)
    labels, rows, hyper, keep = _reads(op, entry, labels=labels, rows=rows, hyper=hyper, keep=keep)
    _lib.check(_lib.load().frmap_head_fit_group_step(x.data_ptr(), labels.data_ptr(), rows.data_ptr(), _dev_at(keep), hyper.data_ptr(),
                                                     w.data_ptr(), b.data_ptr(), state.data_ptr(), workspace.data_ptr(), N, H, B, D, C,
                                                     _group_flags(decoupled, amsgrad, clear, evaluate), _stream()), op)


class HeadGroup(_Head):
    """``H`` linear softmax heads ``[C, D]`` over one cache, with their Adam states, workspaces and the device-resident hyper table
    (`group_step`).  The heads are initialised as ``H`` consecutive `LinearHead` objects would be from ``generator``; with ``shared_init``
    all of them start from head 0's draw (a parameter sweep compares settings, not initialisations)."""

    def __init__(self, H: int, D: int, C: int, device="cuda", amsgrad: bool = False, generator: Optional[torch.Generator] = None,
                 shared_init: bool = False):
        self.H, self.D, self.C, self.amsgrad = int(H), int(D), int(C), bool(amsgrad)
        nbytes = group_state_bytes(self.H, self.D, self.C, self.amsgrad)          # (refuses a bad shape)
        self.stride = group_state_stride(self.D, self.C, self.amsgrad)
        drawn = []
        for h in range(self.H):
            drawn.append(_linear_init(self.C, self.D, generator) if h == 0 or not shared_init else drawn[0])
        device = torch.device(device)
        self.weight, self.bias = torch.stack([w for w, _ in drawn]).to(device), torch.stack([b for _, b in drawn]).to(device)
        self.hyper = torch.zeros((self.H, 8), dtype=torch.float32, device=device)
        self._hyper_host = np.zeros((self.H, 8), np.float32)
        self._start(torch.zeros((nbytes,), dtype=torch.uint8, device=device), device)

    def _workspace_bytes(self, B: int) -> int:
        return group_workspace_bytes(self.H, B, self.D, self.C)

    def set_hyper(self, table: np.ndarray) -> "HeadGroup":
        """Write the hyper table (`hyper_table`) with one host-to-device copy, and only when a value changed."""
        table = np.ascontiguousarray(table, np.float32)
        if table.shape != (self.H, 8):
            raise ValueError(f"HeadGroup.set_hyper: a [{self.H}, 8] table expected, got {table.shape}")
        if not np.array_equal(table.view(np.uint32), self._hyper_host.view(np.uint32)):
            self.hyper.copy_(torch.from_numpy(table))
            self._hyper_host = table.copy()
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
        return self._run(group_step, x, labels, rows, self.hyper, self.weight, self.bias, self.state, self._workspace(B), keep,
                         decoupled=decoupled)

    def evaluate(self, x: torch.Tensor, labels: torch.Tensor, rows: torch.Tensor) -> "HeadGroup":
        """Add the figures of rows ``rows[h]`` under every head's current weights (flag 8): nothing else changes.  The loss is the
        training loss of the table's ``label_smoothing``."""
        B = int(rows.shape[1]) if isinstance(rows, torch.Tensor) and rows.dim() == 2 else 1
        return self._run(group_step, x, labels, rows, self.hyper, self.weight, self.bias, self.state, self._workspace(B), None, evaluate=True)

    def epoch_figures(self) -> list:
        """ONE host copy of the ``H`` headers: per head what `LinearHead.epoch_figures` returns."""
        words = self.state.view(self.H, self.stride)[:, :64].cpu().numpy().view(np.uint64)
        return [_figures(words[h]) for h in range(self.H)]

    def head(self, h: int) -> LinearHead:
        """Head ``h`` as a `LinearHead` whose ``weight``, ``bias`` and ``state`` are VIEWS of the group's memory: `logits`,
        `state_dict`, `load_into` and `as_classifier` read the group's weights, and a single `step` on it continues head ``h``'s fit."""
        if not 0 <= int(h) < self.H:
            raise IndexError(f"HeadGroup.head: {h} is outside 0 ... {self.H - 1}")
        at = int(h) * self.stride
        return LinearHead._over(self.weight[int(h)], self.bias[int(h)], self.state[at: at + state_bytes(self.D, self.C, self.amsgrad)],
                                self.amsgrad, self.device)


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
    return _size("frmap_head_fit_hidden_state_bytes", f"each in 1 ... {MAX_D}", "D Hd C", int(D), int(Hd), int(C), int(bool(amsgrad)))


def hidden_workspace_bytes(B: int, D: int, Hd: int, C: int) -> int:
    """Bytes of the workspace of a hidden-layer step of ``B`` rows (`frmap_head_fit_hidden_workspace_bytes`)."""
    return _size("frmap_head_fit_hidden_workspace_bytes", _B_IN + f"D, Hd, C in 1 ... {MAX_D}", "B D Hd C", int(B), int(D), int(Hd), int(C))


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
    x, labels, N, D = _host_cache(op, x, labels)
    Hd, = _host_layer(op, "w1", "b1", w1, b1, "", "Hd", D)
    C, = _host_layer(op, "w2", "b2", w2, b2, "", "C", Hd)
    rows, B = _host_batch(op, N, rows, (keep1, keep2), batch)
    keep1, keep2 = _host_mask(op, "keep1", keep1, (B, D)), _host_mask(op, "keep2", keep2, (B, Hd))
    workspace = _host_buffers(op, state, hidden_state_bytes(D, Hd, C, amsgrad), workspace, hidden_workspace_bytes(B, D, Hd, C), given_g)
    _lib.check(_lib.load().frmap_head_fit_hidden_step_host(
        _at(x), _at(labels), _at(rows), _at(keep1), float(keep1_scale), _at(keep2), float(keep2_scale), _at(w1), _at(b1), _at(w2), _at(b2),
        _at(state), _at(workspace), N, B, D, Hd, C, *_adam(lr, beta1, beta2, eps, weight_decay), float(label_smoothing),
        _flags(decoupled, amsgrad, clear), int(bool(given_g))), op)
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
    x, N, D = _cache(op, entry, x, labels)
    Hd = _layer(w1, b1, op, "w1", "b1", D)
    C = _layer(w2, b2, op, "w2", "b2", Hd)
    rows, B = _batch(op, entry, N, rows, (keep1, keep2), batch)
    _mask(op, "keep1", keep1, (B, D))
    _mask(op, "keep2", keep2, (B, Hd))
    _buffers(op, entry, state, hidden_state_bytes(D, Hd, C, amsgrad), workspace, hidden_workspace_bytes(B, D, Hd, C), w1=w1, b1=b1, w2=w2, b2=b2)
    labels, keep1, keep2 = _reads(op, entry, labels=labels, keep1=keep1, keep2=keep2)
    _lib.check(_lib.load().frmap_head_fit_hidden_step(
        x.data_ptr(), labels.data_ptr(), _dev_at(rows), _dev_at(keep1), float(keep1_scale), _dev_at(keep2), float(keep2_scale), w1.data_ptr(),
        b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), state.data_ptr(), workspace.data_ptr(), N, B, D, Hd, C,
        *_adam(lr, beta1, beta2, eps, weight_decay), float(label_smoothing), _flags(decoupled, amsgrad, clear), _stream()), op)


class HiddenHead(_Head):
    """``Linear(D, Hd) -> ReLU -> dropout -> Linear(Hd, C)`` on the device with its Adam state and a workspace: the ``fc1`` / ``fc2`` of
    the reference's ``BaselineNet`` over its pooled features, or a learned ``D -> Hd`` projection of any cached feature.  Both layers
    are initialised as consecutive ``nn.Linear(D, Hd)`` and ``nn.Linear(Hd, C)`` would be from ``generator`` (a CPU
    ``torch.Generator``; ``None``: torch's default).  `embed` is the new embedding layer: it feeds `matching.Gallery`,
    `evaluate.verification_metrics` and `frames.identify_streams` like any other embedding."""

    def __init__(self, D: int, Hd: int, C: int, device="cuda", amsgrad: bool = False, generator: Optional[torch.Generator] = None):
        self.D, self.Hd, self.C, self.amsgrad = int(D), int(Hd), int(C), bool(amsgrad)
        nbytes = hidden_state_bytes(self.D, self.Hd, self.C, self.amsgrad)          # (refuses a bad shape)
        device = torch.device(device)
        layers = [_linear_init(self.Hd, self.D, generator), _linear_init(self.C, self.Hd, generator)]
        self.w1, self.b1, self.w2, self.b2 = (t.to(device) for layer in layers for t in layer)
        self._header_at = state_bytes(self.D, self.Hd, self.amsgrad)              # the figures are layer 2's: the second part of the state
        self._start(torch.zeros((nbytes,), dtype=torch.uint8, device=device), device)

    def _workspace_bytes(self, B: int) -> int:
        return hidden_workspace_bytes(B, self.D, self.Hd, self.C)

    def step(self, x: torch.Tensor, labels: torch.Tensor, rows: Optional[torch.Tensor] = None, keep1: Optional[torch.Tensor] = None,
             keep2: Optional[torch.Tensor] = None, *, lr: float, dropout1: float = 0.0, dropout2: float = 0.0,
             keep1_scale: Optional[float] = None, keep2_scale: Optional[float] = None, beta1: float = 0.9, beta2: float = 0.999,
             eps: float = 1e-8, weight_decay: float = 0.0, label_smoothing: float = 0.0, decoupled: bool = False) -> "HiddenHead":
        """One step over rows ``rows`` of the cache ``x`` / ``labels`` (`hidden_step`).  ``keep1`` / ``keep2``: uint8 ``[B, D]`` /
        ``[B, Hd]`` dropout masks on the input / the hidden layer, scaled by ``1 / (1 - dropout1)`` / ``1 / (1 - dropout2)`` unless a
        scale is given.  No synchronisation."""
        return self._run(hidden_step, x, labels, self.w1, self.b1, self.w2, self.b2, self.state,
                         self._workspace(self._batch_rows(x, rows, keep1, keep2)), rows, keep1, self._keep_scale(keep1_scale, keep1, dropout1),
                         keep2, self._keep_scale(keep2_scale, keep2, dropout2), lr=lr, beta1=beta1, beta2=beta2, eps=eps,
                         weight_decay=weight_decay, label_smoothing=label_smoothing, decoupled=decoupled)

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
        at = self._header_at
        return LinearHead._over(self.w2, self.b2, self.state[at: at + state_bytes(self.Hd, self.C, self.amsgrad)], self.amsgrad, self.device)

    def load_into(self, model) -> None:
        """Copy both layers into ``fc1`` / ``fc2`` of a ``BaselineNet`` of matching shapes, in place (the model's plan watches the
        parameters' versions: the next forward rebuilds)."""
        fc1, fc2 = getattr(model, "fc1", None), getattr(model, "fc2", None)
        if type(model).__name__ != "BaselineNet" or not isinstance(fc1, torch.nn.Linear) or not isinstance(fc2, torch.nn.Linear):
            raise ValueError(f"HiddenHead.load_into: a BaselineNet expected, got {type(model).__name__}")
        _load("HiddenHead.load_into", "the head's layer",
              (("fc1", fc1.weight, self.w1), (None, fc1.bias, self.b1), ("fc2", fc2.weight, self.w2), (None, fc2.bias, self.b2)))


# ---------------------------------------------------------------------------------------------------------------------------------
# a contrastive pair head: pairs of cached rows in, an embedding x -> normalize(x w^T + b) out
# ---------------------------------------------------------------------------------------------------------------------------------
MAX_P = MAX_B // 2                # pairs of one step: 2P batch rows
_PDE_IN = f"P in 1 ... {MAX_P}, D in 1 ... {MAX_D}, E in 1 ... {MAX_C}"


def pair_state_bytes(D: int, E: int, amsgrad: bool = False) -> int:
    """Bytes of the state of a pair head (`frmap_head_fit_pair_state_bytes`): `state_bytes` of (D, E)."""
    return _size("frmap_head_fit_pair_state_bytes", f"D in 1 ... {MAX_D}, E in 1 ... {MAX_C}", "D E", int(D), int(E), int(bool(amsgrad)))


def pair_workspace_bytes(P: int, D: int, E: int) -> int:
    """Bytes of the workspace of a pair step of ``P`` pairs (`frmap_head_fit_pair_workspace_bytes`)."""
    return _size("frmap_head_fit_pair_workspace_bytes", _PDE_IN, "P D E", int(P), int(D), int(E))


def pair_workspace_views(workspace: np.ndarray, P: int, E: int) -> dict:
    """a [2P, E], ga [2P, E], pair_loss [P], dist [P] (float32) and row_src [2P] (int32) of a host copy of a pair workspace."""
    raw = np.ascontiguousarray(workspace).view(np.uint8).reshape(-1)
    nf = 4 * P * E + 2 * P
    f = raw[: 4 * nf].view(np.float32)
    return {"a": f[: 2 * P * E].reshape(2 * P, E), "ga": f[2 * P * E: 4 * P * E].reshape(2 * P, E), "pair_loss": f[4 * P * E: 4 * P * E + P],
            "dist": f[4 * P * E + P:], "row_src": raw[4 * nf: 4 * nf + 8 * P].view(np.int32)}


def pair_step_host(x, left, right, differ, w, b, state: np.ndarray, workspace: Optional[np.ndarray] = None, keep=None, keep_scale: float = 1.0, *,
                   margin: float = 2.0, w_same: float = 0.8, w_diff: float = 1.2, accept: float = 0.5, lr: float = 1e-3, beta1: float = 0.9,
                   beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0, decoupled: bool = False, amsgrad: bool = False,
                   clear: bool = False, given_g: bool = False):
    """The pair step on the CPU over numpy arrays (`frmap_head_fit_pair_step_host`; no GPU).  ``w`` [E, D], ``b`` [E] (float32) and
    ``state`` (uint8, `pair_state_bytes` bytes, 8-byte aligned) are updated IN PLACE; ``workspace`` (uint8, exactly
    `pair_workspace_bytes` bytes, or ``None`` for a fresh one) receives a, ga, pair_loss, dist and row_src - with ``given_g`` its a, ga,
    pair_loss and dist are inputs.  Returns the workspace."""
    op = "head_fit.pair_step_host"
    x, _, N, D = _host_cache(op, x, None)
    E, = _host_layer(op, "w", "b", w, b, "", "E", D)
    left, right, differ = (np.ascontiguousarray(t, dtype=np.int32) for t in (left, right, differ))
    if left.ndim != 1 or right.shape != left.shape or differ.shape != left.shape:
        raise ValueError(f"{op}: left [P], right [P] and differ [P] expected, got {left.shape}, {right.shape} and {differ.shape}")
    P = len(left)
    keep = _host_mask(op, "keep", keep, (2 * P, D))
    workspace = _host_buffers(op, state, pair_state_bytes(D, E, amsgrad), workspace, pair_workspace_bytes(P, D, E), given_g)
    _lib.check(_lib.load().frmap_head_fit_pair_step_host(
        _at(x), _at(left), _at(right), _at(differ), _at(keep), float(keep_scale), _at(w), _at(b), _at(state), _at(workspace), N, P, D, E,
        float(margin), float(w_same), float(w_diff), float(accept), *_adam(lr, beta1, beta2, eps, weight_decay),
        _flags(decoupled, amsgrad, clear), int(bool(given_g))), op)
    return workspace


@ops._on_operand_device
def pair_step(x: torch.Tensor, left: torch.Tensor, right: torch.Tensor, differ: torch.Tensor, w: torch.Tensor, b: torch.Tensor,
              state: torch.Tensor, workspace: torch.Tensor, keep: Optional[torch.Tensor] = None, keep_scale: float = 1.0, *,
              margin: float = 2.0, w_same: float = 0.8, w_diff: float = 1.2, accept: float = 0.5, lr: float = 1e-3, beta1: float = 0.9,
              beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0, decoupled: bool = False, amsgrad: bool = False,
              clear: bool = False) -> None:
    """One pair training step on the current stream (`frmap_head_fit_pair_step`; nothing is copied or synchronised).  ``x`` float32
    ``[N, D]`` (the cache), ``left`` / ``right`` int32 ``[P]`` rows of it, ``differ`` int32 ``[P]`` (0: the same identity, 1: different),
    ``w`` float32 ``[E, D]`` and ``b`` ``[E]`` (updated in place), ``state`` uint8 of `pair_state_bytes` bytes (zeros = fresh),
    ``workspace`` uint8 of exactly `pair_workspace_bytes` bytes, ``keep`` uint8 ``[2P, D]`` or ``None``.  Every extent that depends on
    another operand is checked here, before the library sees a pointer."""
    op, entry = "head_fit.pair_step", "frmap_head_fit_pair_step"
    x, N, D = _cache(op, entry, x, None)
    E = _layer(w, b, op, "w", "b", D)
    if not isinstance(left, torch.Tensor) or left.dim() != 1:
        raise ValueError(f"{op}: left [P] expected, got {tuple(left.shape) if isinstance(left, torch.Tensor) else type(left).__name__}")
    P = int(left.shape[0])
    _sized(left, op, "left", (P,), torch.int32)
    _sized(right, op, "right", (P,), torch.int32)
    _sized(differ, op, "differ", (P,), torch.int32)
    _mask(op, "keep", keep, (2 * P, D))
    _buffers(op, entry, state, pair_state_bytes(D, E, amsgrad), workspace, pair_workspace_bytes(P, D, E), w=w, b=b)
    left, right, differ, keep = _reads(op, entry, left=left, right=right, differ=differ, keep=keep)
    _lib.check(_lib.load().frmap_head_fit_pair_step(
        x.data_ptr(), left.data_ptr(), right.data_ptr(), differ.data_ptr(), _dev_at(keep), float(keep_scale), w.data_ptr(), b.data_ptr(),
        state.data_ptr(), workspace.data_ptr(), N, P, D, E, float(margin), float(w_same), float(w_diff), float(accept),
        *_adam(lr, beta1, beta2, eps, weight_decay), _flags(decoupled, amsgrad, clear), _stream()), op)


class PairHead(_Head):
    """A contrastive projection ``x -> normalize(x w^T + b)``, ``[E, D]``, on the device with its Adam state and a workspace: the last
    layer ``fc.8`` of the reference's ``SiameseNet`` over its hidden features, or a learned projection of any cached embedding, fitted
    on pairs with the reference's ``ContrastiveLoss``.  ``weight`` / ``bias`` are drawn as a ``LinearHead(D, E)``'s would be.  `embed`
    feeds `matching.Gallery`, `evaluate.verification_metrics`, `frames.identify_streams` and `matching.compare_faces`."""

    def __init__(self, D: int, E: int, device="cuda", amsgrad: bool = False, generator: Optional[torch.Generator] = None):
        self.D, self.E, self.amsgrad = int(D), int(E), bool(amsgrad)
        nbytes = pair_state_bytes(self.D, self.E, self.amsgrad)          # (refuses a bad shape)
        w, b = _linear_init(self.E, self.D, generator)
        device = torch.device(device)
        self.weight, self.bias = w.to(device), b.to(device)
        self._start(torch.zeros((nbytes,), dtype=torch.uint8, device=device), device)

    def _workspace_bytes(self, P: int) -> int:
        return pair_workspace_bytes(P, self.D, self.E)

    def step(self, x: torch.Tensor, left: torch.Tensor, right: torch.Tensor, differ: torch.Tensor, keep: Optional[torch.Tensor] = None, *,
             lr: float, margin: float = 2.0, w_same: float = 0.8, w_diff: float = 1.2, accept: float = 0.5,
             keep_scale: Optional[float] = None, dropout: float = 0.0, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
             weight_decay: float = 0.0, decoupled: bool = False) -> "PairHead":
        """One step over the pairs ``(left[p], right[p])`` of rows of the cache ``x`` (`pair_step`); ``differ[p]`` is 1 where the two
        rows are of different identities.  ``keep``: a uint8 ``[2P, D]`` dropout mask (the left rows, then the right rows), scaled by
        ``keep_scale`` (default ``1 / (1 - dropout)``).  The defaults are the reference's loss (margin 2.0, 0.8 on same pairs, 1.2 on
        different ones) and its accept rule (distance below 0.5).  No synchronisation."""
        P = int(left.shape[0]) if isinstance(left, torch.Tensor) and left.dim() == 1 else 1
        return self._run(pair_step, x, left, right, differ, self.weight, self.bias, self.state, self._workspace(P), keep,
                         self._keep_scale(keep_scale, keep, dropout), margin=margin, w_same=w_same, w_diff=w_diff, accept=accept, lr=lr,
                         beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, decoupled=decoupled)

    def embed(self, x: torch.Tensor) -> torch.Tensor:
        """``normalize(x w^T + b)``: the unit-norm embedding of cached-feature rows ``x`` ``[B, D]``."""
        return ops.l2_normalize(ops.linear_f32(x, self.weight, None, self.bias), 1e-12)

    def state_dict(self) -> dict:
        return {"weight": self.weight.detach().clone(), "bias": self.bias.detach().clone()}

    def load_into(self, model) -> None:
        """Copy the head into ``fc.8`` of a ``SiameseNet`` in place - a ``[256, 512]`` head over `SiameseNet.fc_hidden_features` (the
        model's plan watches the parameters' versions: the next forward rebuilds)."""
        fc = getattr(model, "fc", None)
        if type(model).__name__ != "SiameseNet" or not isinstance(fc, torch.nn.Sequential):
            raise ValueError(f"PairHead.load_into: a SiameseNet expected, got {type(model).__name__}")
        _load("PairHead.load_into", "the head", (("fc.8", fc[8].weight, self.weight), (None, fc[8].bias, self.bias)))


def draw_pairs(labels: torch.Tensor, P: int, generator: Optional[torch.Generator] = None):
    """``(left, right, differ)``, int32 ``[P]`` on ``labels``' device, with no host copy: ``P`` anchors uniform over the rows; each gets,
    with probability 1/2, a partner uniform among the OTHER rows of its class (``differ = 0``), and otherwise - or when its class has
    one member, where the reference's sampler would spin - a partner uniform among the rows of other classes (``differ = 1``).  The
    labels are sorted once and everything else is arithmetic on class offsets.  ``left != right`` always; with a single class every
    pair is a same pair.  ``generator`` lives on ``labels``' device."""
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.is_floating_point():
        raise ValueError("head_fit.draw_pairs: labels must be an integer tensor [N]")
    N, P, dev = int(labels.shape[0]), int(P), labels.device
    if N < 2 or P < 1:
        raise ValueError(f"head_fit.draw_pairs: at least two rows and one pair expected, got N = {N}, P = {P}")
    sl, order = torch.sort(labels.to(torch.int64), stable=True)
    pos = torch.arange(N, device=dev)
    first = torch.ones((N,), dtype=torch.bool, device=dev)
    first[1:] = sl[1:] != sl[:-1]
    last = torch.ones((N,), dtype=torch.bool, device=dev)
    last[:-1] = first[1:]
    start = torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), 0).values               # of the class of every sorted position
    end = torch.flip(torch.cummin(torch.flip(torch.where(last, pos + 1, torch.full_like(pos, N)), (0,)), 0).values, (0,))
    anchor = torch.randint(0, N, (P,), device=dev, generator=generator)
    u = torch.rand((3, P), device=dev, generator=generator, dtype=torch.float64)
    s, cnt = start[anchor], (end - start)[anchor]
    others = N - cnt
    same = ((u[0] < 0.5) & (cnt > 1)) | (others == 0)
    k_same = torch.minimum((u[1] * (cnt - 1)).to(torch.int64), (cnt - 2).clamp(min=0))
    p_same = s + k_same
    p_same = p_same + (p_same >= anchor).to(torch.int64)                                          # (skip the anchor itself)
    k_diff = torch.minimum((u[2] * others).to(torch.int64), (others - 1).clamp(min=0))
    p_diff = torch.where(k_diff < s, k_diff, k_diff + cnt)                                        # (skip the anchor's class)
    partner = torch.where(same, p_same, p_diff).clamp(0, N - 1)
    return order[anchor].to(torch.int32), order[partner].to(torch.int32), (~same).to(torch.int32)


def fit_pair_head(model, train_data, val_data=None, epochs: int = 10, batch_pairs: int = 32, lr: float = 1e-3, weight_decay: float = 1e-4,
                  dropout: float = 0.0, margin: float = 2.0, w_same: float = 0.8, w_diff: float = 1.2, accept: float = 0.5,
                  layer: str = "embedding", embed_dim: Optional[int] = None, decoupled: bool = False, amsgrad: bool = False,
                  generator: Optional[torch.Generator] = None, device="cuda"):
    """Fit a `PairHead` on the frozen model's features with the reference's contrastive objective (`src/training.py:484-490`).  The
    training set is embedded once (`cache_embeddings`); every step then draws ``batch_pairs`` pairs (`draw_pairs`) and, with
    ``dropout``, a mask on the device, ``ceil(N / batch_pairs)`` steps an epoch with no host copy inside it; the epoch's figures are one
    64-byte copy at its end.  With ``val_data`` every epoch's `evaluate.verification_metrics` of ``head.embed`` on the validation
    rows.  ``layer="fc_hidden"`` (a ``SiameseNet``): the cache is the input of its ``fc.8`` and the head ``[256, 512]``, that layer
    itself (`PairHead.load_into`); otherwise the head projects the model's embedding to ``embed_dim`` (default: its own width).
    Returns ``(head, history)`` with ``history = {"train_loss": [...], "train_acc": [...], "val": [metrics dict per epoch]}``.
    Order of draws: the device generator's seed from the CPU ``generator`` FIRST, then the head from it (the reverse of `fit_head`,
    kept as it is); per step `draw_pairs` (one ``randint``, one ``rand((3, P))``), then one ``rand((2P, D))`` iff ``dropout > 0``."""
    from . import evaluate
    feats, labels = cache_embeddings(model, train_data, device=device, layer=layer)
    N, D = int(feats.shape[0]), int(feats.shape[1])
    E = int(embed_dim) if embed_dim is not None else (256 if layer == "fc_hidden" else D)
    head_gen, dev_gen = _generators(generator, feats.device)
    head = PairHead(D, E, feats.device, amsgrad=amsgrad, generator=head_gen)
    val = cache_embeddings(model, val_data, device=device, layer=layer) if val_data is not None else None
    P = int(batch_pairs)

    def run_epoch(epoch):
        for _ in range((N + P - 1) // P):
            left, right, differ = draw_pairs(labels, P, dev_gen)
            keep = (torch.rand((2 * P, D), device=feats.device, generator=dev_gen) >= dropout).to(torch.uint8) if dropout > 0 else None
            head.step(feats, left, right, differ, keep, lr=lr, margin=margin, w_same=w_same, w_diff=w_diff, accept=accept, dropout=dropout,
                      weight_decay=weight_decay, decoupled=decoupled)
    return _fit(head, epochs, run_epoch, None if val is None else lambda head: evaluate.verification_metrics(head.embed(val[0]), val[1]))


# ---------------------------------------------------------------------------------------------------------------------------------
# an ArcFace margin head: cached embeddings in, the class centres of `ArcFaceNet.arcface.weight` out
# ---------------------------------------------------------------------------------------------------------------------------------
EASY_MARGIN = 16                  # FRMAP_HEAD_FIT_EASY_MARGIN: bit of the margin step's flags


def margin_state_bytes(D: int, C: int, amsgrad: bool = False) -> int:
    """Bytes of the state of a margin head (`frmap_head_fit_margin_state_bytes`): `state_bytes` of (D, C); the bias moments stay zero,
    so `state_views` reads it."""
    return _size("frmap_head_fit_margin_state_bytes", _DC_IN, "D C", int(D), int(C), int(bool(amsgrad)))


def margin_workspace_bytes(B: int, D: int, C: int) -> int:
    """Bytes of the workspace of a margin step of ``B`` rows (`frmap_head_fit_margin_workspace_bytes`)."""
    return _size("frmap_head_fit_margin_workspace_bytes", _B_IN + _DC_IN, "B D C", int(B), int(D), int(C))


def margin_workspace_views(workspace: np.ndarray, B: int, C: int) -> dict:
    """z, cosv, g, h [B, C], row_loss [B], rx [B], rw [C] (float32) and row_src [B] (int32) of a host copy of a margin workspace."""
    raw = np.ascontiguousarray(workspace).view(np.uint8).reshape(-1)
    nf = 4 * B * C + 2 * B + C
    f = raw[: 4 * nf].view(np.float32)
    out = {k: f[j * B * C: (j + 1) * B * C].reshape(B, C) for j, k in enumerate(("z", "cosv", "g", "h"))}
    at = 4 * B * C
    out.update(row_loss=f[at: at + B], rx=f[at + B: at + 2 * B], rw=f[at + 2 * B: at + 2 * B + C],
               row_src=raw[4 * nf: 4 * nf + 4 * B].view(np.int32))
    return out


def _margin_flags(decoupled, amsgrad, clear, easy_margin) -> int:
    return _flags(decoupled, amsgrad, clear) | (EASY_MARGIN if easy_margin else 0)


def margin_step_host(x, labels, w, state: np.ndarray, workspace: Optional[np.ndarray] = None, rows=None, keep=None, keep_scale: float = 1.0, *,
                     s: float, m: float, easy_margin: bool = False, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999,
                     eps: float = 1e-8, weight_decay: float = 0.0, label_smoothing: float = 0.0, decoupled: bool = False,
                     amsgrad: bool = False, clear: bool = False, given_g: bool = False, batch: Optional[int] = None):
    """The margin step on the CPU over numpy arrays (`frmap_head_fit_margin_step_host`; no GPU).  ``w`` [C, D] (float32) and ``state``
    (uint8, `margin_state_bytes` bytes, 8-byte aligned) are updated IN PLACE; ``workspace`` (uint8, exactly `margin_workspace_bytes`
    bytes, or ``None`` for a fresh one) receives z, cosv, g, h, row_loss, rx, rw and row_src - with ``given_g`` all but row_src are
    inputs.  Returns the workspace."""
    op = "head_fit.margin_step_host"
    x, labels, N, D = _host_cache(op, x, labels)
    _host_array(op, "w", w, np.float32)
    if w.ndim != 2 or w.shape[1] != D:
        raise ValueError(f"{op}: w [C, {D}] expected, got {w.shape}")
    C = int(w.shape[0])
    rows, B = _host_batch(op, N, rows, (keep,), batch)
    keep = _host_mask(op, "keep", keep, (B, D))
    workspace = _host_buffers(op, state, margin_state_bytes(D, C, amsgrad), workspace, margin_workspace_bytes(B, D, C), given_g)
    _lib.check(_lib.load().frmap_head_fit_margin_step_host(
        _at(x), _at(labels), _at(rows), _at(keep), float(keep_scale), _at(w), _at(state), _at(workspace), N, B, D, C, float(s), float(m),
        float(label_smoothing), *_adam(lr, beta1, beta2, eps, weight_decay), _margin_flags(decoupled, amsgrad, clear, easy_margin),
        int(bool(given_g))), op)
    return workspace


@ops._on_operand_device
def margin_step(x: torch.Tensor, labels: torch.Tensor, w: torch.Tensor, state: torch.Tensor, workspace: torch.Tensor,
                rows: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None, keep_scale: float = 1.0, *, s: float, m: float,
                easy_margin: bool = False, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                weight_decay: float = 0.0, label_smoothing: float = 0.0, decoupled: bool = False, amsgrad: bool = False, clear: bool = False,
                batch: Optional[int] = None) -> None:
    """One margin training step on the current stream (`frmap_head_fit_margin_step`; nothing is copied or synchronised).  ``x`` float32
    ``[N, D]`` (the cache), ``labels`` int32 ``[N]``, ``w`` float32 ``[C, D]`` (updated in place), ``state`` uint8 of
    `margin_state_bytes` bytes (zeros = fresh), ``workspace`` uint8 of exactly `margin_workspace_bytes` bytes, ``rows`` int32 ``[B]`` or
    ``None``, ``keep`` uint8 ``[B, D]`` or ``None``; ``s`` and ``m`` are the effective scale and margin of this step
    (`margin_schedule`).  Every extent that depends on another operand is checked here, before the library sees a pointer."""
    op, entry = "head_fit.margin_step", "frmap_head_fit_margin_step"
    x, N, D = _cache(op, entry, x, labels)
    _sized(w, op, "w", (w.shape[0] if isinstance(w, torch.Tensor) and w.dim() == 2 else -1, D), torch.float32)
    C = int(w.shape[0])
    rows, B = _batch(op, entry, N, rows, (keep,), batch)
    _mask(op, "keep", keep, (B, D))
    _buffers(op, entry, state, margin_state_bytes(D, C, amsgrad), workspace, margin_workspace_bytes(B, D, C), w=w)
    labels, keep = _reads(op, entry, labels=labels, keep=keep)
    _lib.check(_lib.load().frmap_head_fit_margin_step(
        x.data_ptr(), labels.data_ptr(), _dev_at(rows), _dev_at(keep), float(keep_scale), w.data_ptr(), state.data_ptr(), workspace.data_ptr(),
        N, B, D, C, float(s), float(m), float(label_smoothing), *_adam(lr, beta1, beta2, eps, weight_decay),
        _margin_flags(decoupled, amsgrad, clear, easy_margin), _stream()), op)


class MarginHead(_Head):
    """The class centres ``[C, D]`` of an ArcFace margin head on the device with their Adam state and a workspace: the ``weight`` of the
    reference's ``ArcMarginProduct``, initialised as it is (``xavier_normal_`` with gain sqrt(2), `src/face_models.py:326`) from
    ``generator`` (a CPU ``torch.Generator``; ``None``: torch's default).  `cosines` is what `evaluate.evaluate_model`,
    `evaluate_stream` and `arcface_validate` score with; `load_into` hands the centres to an ``ArcFaceNet``."""

    def __init__(self, D: int, C: int, device="cuda", amsgrad: bool = False, generator: Optional[torch.Generator] = None):
        self.D, self.C, self.amsgrad = int(D), int(C), bool(amsgrad)
        nbytes = margin_state_bytes(self.D, self.C, self.amsgrad)          # (refuses a bad shape)
        device = torch.device(device)
        self.weight = _margin_init(self.C, self.D, generator).to(device)
        self._start(torch.zeros((nbytes,), dtype=torch.uint8, device=device), device)

    def _workspace_bytes(self, B: int) -> int:
        return margin_workspace_bytes(B, self.D, self.C)

    def step(self, x: torch.Tensor, labels: torch.Tensor, rows: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None, *,
             lr: float, s: float, m: float, easy_margin: bool = False, label_smoothing: float = 0.0, keep_scale: Optional[float] = None,
             dropout: float = 0.0, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0,
             decoupled: bool = False) -> "MarginHead":
        """One step over rows ``rows`` of the cache ``x`` / ``labels`` (`margin_step`) at the effective scale ``s`` and margin ``m``.
        ``keep``: a uint8 ``[B, D]`` dropout mask, scaled by ``keep_scale`` (default ``1 / (1 - dropout)``; the scale cancels in the
        cosine).  No synchronisation."""
        return self._run(margin_step, x, labels, self.weight, self.state, self._workspace(self._batch_rows(x, rows, keep)), rows, keep,
                         self._keep_scale(keep_scale, keep, dropout), s=s, m=m, easy_margin=easy_margin, lr=lr, beta1=beta1, beta2=beta2,
                         eps=eps, weight_decay=weight_decay, label_smoothing=label_smoothing, decoupled=decoupled)

    def cosines(self, x: torch.Tensor) -> torch.Tensor:
        """The cosine of every row of ``x`` ``[B, D]`` with every class centre, ``[B, C]`` (`ops.cosine_logits`)."""
        return self.logits(x, 1.0)

    def logits(self, x: torch.Tensor, s: float = 1.0) -> torch.Tensor:
        """``s`` times `cosines`: the reference's eval-mode output without its margin (arg-max and ranks do not depend on ``s``)."""
        return ops.cosine_logits(x, self.weight, s=float(s), want_argmax=False)[0]

    def state_dict(self) -> dict:
        return {"weight": self.weight.detach().clone()}

    def load_into(self, model) -> None:
        """Copy the centres into ``arcface.weight`` of an ``ArcFaceNet`` in place; any other class and any other shape is refused."""
        arc = _arcface_parts("MarginHead.load_into", model)[2]
        _load("MarginHead.load_into", "the head", (("arcface.weight", arc.weight, self.weight),))


def fit_margin_head(model, train_data, val_data=None, epochs: int = 10, batch_size: int = 32, lr: float = 1e-3, weight_decay: float = 1e-4,
                    s: float = 32.0, m: float = 0.5, easy_margin: bool = False, warm_up: bool = True, dropout: float = 0.0,
                    label_smoothing: float = 0.05, decoupled: bool = True, amsgrad: bool = True,
                    generator: Optional[torch.Generator] = None, num_classes: Optional[int] = None, device="cuda"):
    """Fit a `MarginHead` on the frozen model's embeddings with the reference's ArcFace objective.  The training set is embedded once
    (`cache_embeddings`: the model's normalised embedding; a dropout mask on it reproduces the head input of the reference's training
    mode, since a normalisation follows); epoch ``e`` runs at `margin_schedule(e, s, m)`; every epoch draws a fresh device permutation
    as ``rows`` (and masks, with ``dropout``) and steps through it with no host copy inside the epoch.  The defaults are the reference's
    ArcFace settings (`src/training.py:340-348`: AdamW, AMSGrad, label smoothing 0.05).  With ``val_data`` every epoch's validation
    ``head.logits`` go through `evaluate.ClassificationTally`.  Returns ``(head, history)`` in `fit_head`'s shape.
    Order of draws: the device generator's seed from the CPU ``generator`` FIRST, then the head from it (the reverse of `fit_head`,
    kept as it is); per epoch one ``randperm``; per batch one ``rand`` iff ``dropout > 0``."""
    feats, labels = cache_embeddings(model, train_data, device=device)
    D = int(feats.shape[1])
    C = int(num_classes) if num_classes is not None else int(labels.max().item()) + 1
    head_gen, dev_gen = _generators(generator, feats.device)
    head = MarginHead(D, C, feats.device, amsgrad=amsgrad, generator=head_gen)
    val = cache_embeddings(model, val_data, device=device) if val_data is not None else None
    return _fit(head, epochs, _row_epochs(head, feats, labels, batch_size, [(D, dropout)], dev_gen,
                                          _margin_kw(s, m, warm_up, lr=lr, easy_margin=easy_margin, label_smoothing=label_smoothing,
                                                     dropout=dropout, weight_decay=weight_decay, decoupled=decoupled)),
                None if val is None else lambda head: _tally(C, head.logits(val[0], min(s, 24.0)), val[1]))


def _margin_kw(s, m, warm_up, **kw):
    """The per-epoch keyword arguments of a fit on the margin schedule: ``kw`` with epoch ``e``'s `margin_schedule(e, s, m)`."""
    def step_kw(epoch):
        m_eff, s_eff = margin_schedule(epoch, s, m, warm_up=warm_up)
        return dict(kw, s=s_eff, m=m_eff)
    return step_kw


# ---------------------------------------------------------------------------------------------------------------------------------
# the embedding layer of an ArcFace model: pooled trunk features in; `embedding`, `bn` and `arcface.weight` out
# ---------------------------------------------------------------------------------------------------------------------------------
GIVEN_STATS, GIVEN_MARGIN, GIVEN_DA = 1, 2, 4      # bits of `given` of `embed_step_host`: the float64 stages taken from the workspace
_DEC_IN = f"D, E, C in 1 ... {MAX_D}"


def embed_state_bytes(D: int, E: int, C: int, amsgrad: bool = False) -> int:
    """Bytes of the state of an embedding head (`frmap_head_fit_embed_state_bytes`): `state_bytes` of (D, E), of (1, E) - gamma as the
    weight, beta as the bias - and of (E, C), the margin state of the centres."""
    return _size("frmap_head_fit_embed_state_bytes", _DEC_IN, "D E C", int(D), int(E), int(C), int(bool(amsgrad)))


def embed_workspace_bytes(B: int, D: int, E: int, C: int) -> int:
    """Bytes of the workspace of an embedding step of ``B`` rows (`frmap_head_fit_embed_workspace_bytes`)."""
    return _size("frmap_head_fit_embed_workspace_bytes", _B_IN + _DEC_IN, "B D E C", int(B), int(D), int(E), int(C))


def embed_state_parts(D: int, E: int, C: int, amsgrad: bool = False) -> dict:
    """name -> (byte offset, bytes) of the three parts of an embedding state."""
    n1, n2, n3 = state_bytes(D, E, amsgrad), state_bytes(1, E, amsgrad), state_bytes(E, C, amsgrad)
    assert n1 + n2 + n3 == embed_state_bytes(D, E, C, amsgrad)
    return {"linear": (0, n1), "bn": (n1, n2), "margin": (n1 + n2, n3)}


def embed_state_views(state: np.ndarray, D: int, E: int, C: int, amsgrad: bool = False) -> dict:
    """``{"linear": state_views of (D, E), "bn": of (1, E), "margin": of (E, C)}`` into a host copy of an embedding state."""
    raw = np.ascontiguousarray(state).view(np.uint8).reshape(-1)
    dims = {"linear": (D, E), "bn": (1, E), "margin": (E, C)}
    return {k: state_views(raw[at: at + n], *dims[k], amsgrad) for k, (at, n) in embed_state_parts(D, E, C, amsgrad).items()}


def embed_workspace_views(workspace: np.ndarray, B: int, E: int, C: int) -> dict:
    """a, ah, yp, gy, da [B, E], mean32, rstd, uvar, dbeta, dgamma [E] (float32), lab, row_src1 [B], n1 (int32) and, under
    ``"margin"``, `margin_workspace_views` of the margin stage, of a host copy of an embedding workspace."""
    raw = np.ascontiguousarray(workspace).view(np.uint8).reshape(-1)
    f = raw[: 4 * (5 * B * E + 5 * E)].view(np.float32)
    out = {k: f[j * B * E: (j + 1) * B * E].reshape(B, E) for j, k in enumerate(("a", "ah", "yp", "gy", "da"))}
    out.update({k: f[5 * B * E + j * E: 5 * B * E + (j + 1) * E] for j, k in enumerate(("mean32", "rstd", "uvar", "dbeta", "dgamma"))})
    at = 4 * (5 * B * E + 5 * E)
    out.update(lab=raw[at: at + 4 * B].view(np.int32), row_src1=raw[at + 4 * B: at + 8 * B].view(np.int32),
               n1=raw[at + 8 * B: at + 8 * B + 4].view(np.int32), margin=margin_workspace_views(raw[at + 8 * B + 8:], B, C))
    return out


def _host_vectors(op, E, **vectors):
    for name, v in vectors.items():
        _host_array(op, name, v, np.float32)
        if v.shape != (E,):
            raise ValueError(f"{op}: {name} [{E}] expected, got {v.shape}")


def embed_step_host(x, labels, w1, gamma, beta, running_mean, running_var, wc, state: np.ndarray, workspace: Optional[np.ndarray] = None,
                    rows=None, keep=None, keep_scale: float = 1.0, *, bn_eps: float = 1e-5, bn_momentum: float = 0.1, s: float, m: float,
                    easy_margin: bool = False, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                    weight_decay: float = 0.0, label_smoothing: float = 0.0, decoupled: bool = False, amsgrad: bool = False,
                    clear: bool = False, given: int = 0, batch: Optional[int] = None):
    """The embedding step on the CPU over numpy arrays (`frmap_head_fit_embed_step_host`; no GPU).  ``w1`` [E, D], ``gamma``, ``beta``,
    ``running_mean``, ``running_var`` [E], ``wc`` [C, E] (float32) and ``state`` (uint8, `embed_state_bytes` bytes, 8-byte aligned) are
    updated IN PLACE; ``workspace`` (uint8, exactly `embed_workspace_bytes` bytes, or ``None`` for a fresh one) receives every
    intermediate (`embed_workspace_views`).  ``given``: bits `GIVEN_STATS` | `GIVEN_MARGIN` | `GIVEN_DA` - the float64 stages whose
    outputs in the workspace are inputs.  Returns the workspace."""
    op = "head_fit.embed_step_host"
    x, labels, N, D = _host_cache(op, x, labels)
    for name, t in (("w1", w1), ("wc", wc)):
        _host_array(op, name, t, np.float32)
    if w1.ndim != 2 or w1.shape[1] != D:
        raise ValueError(f"{op}: w1 [E, {D}] expected, got {w1.shape}")
    E = int(w1.shape[0])
    if wc.ndim != 2 or wc.shape[1] != E:
        raise ValueError(f"{op}: wc [C, {E}] expected, got {wc.shape}")
    C = int(wc.shape[0])
    _host_vectors(op, E, gamma=gamma, beta=beta, running_mean=running_mean, running_var=running_var)
    rows, B = _host_batch(op, N, rows, (keep,), batch)
    keep = _host_mask(op, "keep", keep, (B, E))
    workspace = _host_buffers(op, state, embed_state_bytes(D, E, C, amsgrad), workspace, embed_workspace_bytes(B, D, E, C), bool(given))
    _lib.check(_lib.load().frmap_head_fit_embed_step_host(
        _at(x), _at(labels), _at(rows), _at(keep), float(keep_scale), _at(w1), _at(gamma), _at(beta), _at(running_mean), _at(running_var),
        _at(wc), _at(state), _at(workspace), N, B, D, E, C, float(bn_eps), float(bn_momentum), float(s), float(m), float(label_smoothing),
        *_adam(lr, beta1, beta2, eps, weight_decay), _margin_flags(decoupled, amsgrad, clear, easy_margin), int(given)), op)
    return workspace


@ops._on_operand_device
def embed_step(x: torch.Tensor, labels: torch.Tensor, w1: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, running_mean: torch.Tensor,
               running_var: torch.Tensor, wc: torch.Tensor, state: torch.Tensor, workspace: torch.Tensor, rows: Optional[torch.Tensor] = None,
               keep: Optional[torch.Tensor] = None, keep_scale: float = 1.0, *, bn_eps: float = 1e-5, bn_momentum: float = 0.1, s: float,
               m: float, easy_margin: bool = False, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
               weight_decay: float = 0.0, label_smoothing: float = 0.0, decoupled: bool = False, amsgrad: bool = False, clear: bool = False,
               batch: Optional[int] = None) -> None:
    """One embedding training step on the current stream (`frmap_head_fit_embed_step`; nothing is copied or synchronised).  ``x`` float32
    ``[N, D]`` (the cache of pooled features), ``labels`` int32 ``[N]``, ``w1`` ``[E, D]``, ``gamma``, ``beta``, ``running_mean``,
    ``running_var`` ``[E]`` and ``wc`` ``[C, E]`` float32 (updated in place), ``state`` uint8 of `embed_state_bytes` bytes (zeros = fresh),
    ``workspace`` uint8 of exactly `embed_workspace_bytes` bytes, ``rows`` int32 ``[B]`` or ``None``, ``keep`` uint8 ``[B, E]`` or ``None``
    (the dropout behind the BatchNorm); ``s`` and ``m`` are the effective scale and margin of this step (`margin_schedule`).  Every
    extent that depends on another operand is checked here, before the library sees a pointer."""
    op, entry = "head_fit.embed_step", "frmap_head_fit_embed_step"
    x, N, D = _cache(op, entry, x, labels)
    _sized(w1, op, "w1", (w1.shape[0] if isinstance(w1, torch.Tensor) and w1.dim() == 2 else -1, D), torch.float32)
    E = int(w1.shape[0])
    _sized(wc, op, "wc", (wc.shape[0] if isinstance(wc, torch.Tensor) and wc.dim() == 2 else -1, E), torch.float32)
    C = int(wc.shape[0])
    vectors = {"gamma": gamma, "beta": beta, "running_mean": running_mean, "running_var": running_var}
    for name, t in vectors.items():
        _sized(t, op, name, (E,), torch.float32)
    rows, B = _batch(op, entry, N, rows, (keep,), batch)
    _mask(op, "keep", keep, (B, E))
    _buffers(op, entry, state, embed_state_bytes(D, E, C, amsgrad), workspace, embed_workspace_bytes(B, D, E, C), w1=w1, wc=wc, **vectors)
    labels, keep = _reads(op, entry, labels=labels, keep=keep)
    _lib.check(_lib.load().frmap_head_fit_embed_step(
        x.data_ptr(), labels.data_ptr(), _dev_at(rows), _dev_at(keep), float(keep_scale), w1.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
        running_mean.data_ptr(), running_var.data_ptr(), wc.data_ptr(), state.data_ptr(), workspace.data_ptr(), N, B, D, E, C, float(bn_eps),
        float(bn_momentum), float(s), float(m), float(label_smoothing), *_adam(lr, beta1, beta2, eps, weight_decay),
        _margin_flags(decoupled, amsgrad, clear, easy_margin), _stream()), op)


class EmbedHead(_Head):
    """``Linear(D, E, bias=False) -> BatchNorm1d(E) -> dropout -> normalize -> margin`` on the device with its Adam state and a workspace:
    the ``embedding``, ``bn`` and ``arcface`` of the reference's ``ArcFaceNet`` over its pooled trunk features
    (`cache_features(layer="pooled")`).  A new head starts as those modules do (``nn.Linear`` and the margin's ``xavier_normal_`` draws
    from ``generator``, gamma 1, beta 0, running statistics 0 and 1); `from_model` starts from a model's own tensors.  `embed` is the
    deployed embedding - the RUNNING statistics, as `ArcFaceNet.get_embedding` applies them."""

    def __init__(self, D: int, E: int, C: int, device="cuda", amsgrad: bool = False, generator: Optional[torch.Generator] = None,
                 bn_eps: float = 1e-5, bn_momentum: float = 0.1):
        w1 = _linear_init(int(E), int(D), generator)[0]
        wc = _margin_init(int(C), int(E), generator)
        self._adopt(w1, torch.ones(int(E)), torch.zeros(int(E)), torch.zeros(int(E)), torch.ones(int(E)), wc, device, amsgrad, bn_eps, bn_momentum)

    def _adopt(self, w1, gamma, beta, running_mean, running_var, wc, device, amsgrad, bn_eps, bn_momentum):
        self.E, self.D, self.C, self.amsgrad = int(w1.shape[0]), int(w1.shape[1]), int(wc.shape[0]), bool(amsgrad)
        self.bn_eps, self.bn_momentum = float(bn_eps), float(bn_momentum)
        nbytes = embed_state_bytes(self.D, self.E, self.C, self.amsgrad)           # (refuses a bad shape)
        device = torch.device(device)
        self.w1, self.gamma, self.beta, self.running_mean, self.running_var, self.wc = (
            t.detach().to(device=device, dtype=torch.float32).clone().contiguous() for t in (w1, gamma, beta, running_mean, running_var, wc))
        self._header_at = embed_state_parts(self.D, self.E, self.C, self.amsgrad)["margin"][0]    # the figures are the margin state's
        self._start(torch.zeros((nbytes,), dtype=torch.uint8, device=device), device)

    @classmethod
    def from_model(cls, model, device=None, amsgrad: bool = False) -> "EmbedHead":
        """A head that starts from ``embedding.weight``, ``bn`` and ``arcface.weight`` of an ``ArcFaceNet`` (copies: the model changes
        only through `load_into`)."""
        emb, bn, arc = _arcface_parts("EmbedHead.from_model", model)
        if emb.bias is not None:
            raise ValueError("EmbedHead.from_model: embedding has a bias; the head has none")
        one = cls.__new__(cls)
        one._adopt(emb.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, arc.weight, device if device is not None else emb.weight.device,
                   amsgrad, bn.eps, 0.1 if bn.momentum is None else bn.momentum)
        return one

    def _workspace_bytes(self, B: int) -> int:
        return embed_workspace_bytes(B, self.D, self.E, self.C)

    def step(self, x: torch.Tensor, labels: torch.Tensor, rows: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None, *,
             lr: float, s: float, m: float, easy_margin: bool = False, label_smoothing: float = 0.0, keep_scale: Optional[float] = None,
             dropout: float = 0.0, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0,
             decoupled: bool = False) -> "EmbedHead":
        """One step over rows ``rows`` of the cache ``x`` / ``labels`` (`embed_step`) at the effective scale ``s`` and margin ``m``.
        ``keep``: a uint8 ``[B, E]`` dropout mask behind the BatchNorm, scaled by ``keep_scale`` (default ``1 / (1 - dropout)``).  No
        synchronisation."""
        return self._run(embed_step, x, labels, self.w1, self.gamma, self.beta, self.running_mean, self.running_var, self.wc, self.state,
                         self._workspace(self._batch_rows(x, rows, keep)), rows, keep, self._keep_scale(keep_scale, keep, dropout), bn_eps=self.bn_eps,
                         bn_momentum=self.bn_momentum, s=s, m=m, easy_margin=easy_margin, lr=lr, beta1=beta1, beta2=beta2, eps=eps,
                         weight_decay=weight_decay, label_smoothing=label_smoothing, decoupled=decoupled)

    def embed(self, x: torch.Tensor) -> torch.Tensor:
        """``normalize(bn_eval(x w1^T))`` of pooled-feature rows ``x`` ``[B, D]`` with the RUNNING statistics: the arithmetic of the
        deployed ``ArcFaceNet.get_embedding`` behind its trunk (`ops.linear_f32` with the folded scale and shift, `ops.l2_normalize`)."""
        scale = self.gamma / torch.sqrt(self.running_var + self.bn_eps)
        shift = self.beta - self.running_mean * scale
        return ops.l2_normalize(ops.linear_f32(x, self.w1, scale.contiguous(), shift.contiguous()), 1e-12)

    def centres(self) -> "MarginHead":
        """The class centres as a `MarginHead` whose ``weight`` and ``state`` are VIEWS of this head's memory (the last part of the
        state is a valid margin state): its `cosines` and `logits` take `embed` outputs."""
        at, n = embed_state_parts(self.D, self.E, self.C, self.amsgrad)["margin"]
        one = MarginHead.__new__(MarginHead)
        one.D, one.C, one.amsgrad, one.weight = self.E, self.C, self.amsgrad, self.wc
        one._start(self.state[at: at + n], self.device, False)
        return one

    def state_dict(self) -> dict:
        return {"embedding.weight": self.w1.detach().clone(), "bn.weight": self.gamma.detach().clone(), "bn.bias": self.beta.detach().clone(),
                "bn.running_mean": self.running_mean.detach().clone(), "bn.running_var": self.running_var.detach().clone(),
                "arcface.weight": self.wc.detach().clone()}

    def load_into(self, model) -> None:
        """Copy the six tensors into ``embedding.weight``, ``bn.weight``, ``bn.bias``, ``bn.running_mean``, ``bn.running_var`` and
        ``arcface.weight`` of an ``ArcFaceNet`` in place and advance ``bn.num_batches_tracked`` by the steps taken since the last
        `load_into` (one host copy of the step count); any other class and any other shape is refused by name.  The model's plan
        watches its parameters and buffers: the next forward rebuilds."""
        emb, bn, arc = _arcface_parts("EmbedHead.load_into", model)
        _load("EmbedHead.load_into", "the head's",
              (("embedding.weight", emb.weight, self.w1), ("bn.weight", bn.weight, self.gamma), ("bn.bias", bn.bias, self.beta),
               ("bn.running_mean", bn.running_mean, self.running_mean), ("bn.running_var", bn.running_var, self.running_var),
               ("arcface.weight", arc.weight, self.wc)))
        t = self.epoch_figures()["t"]
        if bn.num_batches_tracked is not None:
            with torch.no_grad():
                bn.num_batches_tracked += t - getattr(self, "_loaded_t", 0)
        self._loaded_t = t


def fit_embed_head(model, train_data, val_data=None, epochs: int = 10, batch_size: int = 32, lr: float = 1e-3, weight_decay: float = 1e-4,
                   dropout: float = 0.2, s: float = 32.0, m: float = 0.5, easy_margin: bool = False, warm_up: bool = True,
                   label_smoothing: float = 0.05, decoupled: bool = True, amsgrad: bool = True,
                   generator: Optional[torch.Generator] = None, device="cuda"):
    """Fit ``embedding``, ``bn`` and the class centres of a frozen ``ArcFaceNet`` with the reference's ArcFace objective: the first phase
    of its two-phase training on the device.  The pooled trunk features of the training set are cached once
    (`cache_features(layer="pooled")`); the head starts from the model's own tensors (`EmbedHead.from_model`; the class count is the
    model's); epoch ``e`` runs at `margin_schedule(e, s, m)`; every epoch draws a fresh device permutation as ``rows`` and, with
    ``dropout``, a mask per step, and steps through it with no host copy inside the epoch.  A trailing batch of one row is a step that
    is not taken (BatchNorm has no statistics of one row).  The defaults are the reference's ArcFace settings (`src/training.py:340-348`;
    ``dropout_rate=0.2``).  With ``val_data`` every epoch's validation accuracy is the arg-max of `ops.cosine_logits` of `EmbedHead.embed`
    against the centres.  The model is not changed: call ``head.load_into(model)``.  Returns ``(head, history)`` in `fit_head`'s shape.
    Order of draws: no head is drawn (`EmbedHead.from_model`); the device generator's seed from the CPU ``generator``; per epoch one
    ``randperm``; per batch one ``rand`` of ``[rows, E]`` iff ``dropout > 0`` - for the trailing batch of one row too, which is
    stepped and which the library declines."""
    feats, labels = cache_features(model, "arcface", train_data, device=device, layer="pooled")
    head = EmbedHead.from_model(model, feats.device, amsgrad=amsgrad)
    _, dev_gen = _generators(generator, feats.device)
    val = cache_features(model, "arcface", val_data, device=device, layer="pooled") if val_data is not None else None

    def validate(head):
        pred = ops.cosine_logits(head.embed(val[0]), head.wc, s=1.0, want_logits=False, want_argmax=True)[1]
        return {"accuracy": float((pred.to(torch.int64) == val[1].to(torch.int64)).float().mean().item())}
    return _fit(head, epochs, _row_epochs(head, feats, labels, batch_size, [(head.E, dropout)], dev_gen,
                                          _margin_kw(s, m, warm_up, lr=lr, easy_margin=easy_margin, label_smoothing=label_smoothing,
                                                     dropout=dropout, weight_decay=weight_decay, decoupled=decoupled)),
                validate if val is not None else None)
