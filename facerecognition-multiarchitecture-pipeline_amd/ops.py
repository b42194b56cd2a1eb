"""Thin tensor-level wrappers over the C ABI (``include/frmap_hip.h``).

PyTorch is used here only for device memory (``torch.empty``) and the current HIP stream; every
function validates that its operands live on the GPU and hands raw pointers to the library.
Activations are NHWC tensors in the compute dtype (bf16 / fp16); heads and matching are fp32.
"""
from __future__ import annotations

import functools
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

BF16, F16 = 0, 1
_DT = {torch.bfloat16: BF16, torch.float16: F16}


def _stream() -> int:
    # the CURRENT device's current stream: every public wrapper runs under `_on_operand_device`, which makes the
    # operands' device current first (HIP's current device is per thread, SURVEY.md §8b threading)
    return torch.cuda.current_stream().cuda_stream


def _on_operand_device(fn):
    """Launch on the device the operands live on, whatever the calling thread's current device is: a model on
    ``cuda:1`` works from a thread whose current device is ``cuda:0`` (`src/app.py:43` moves the input to
    ``next(model.parameters()).device``; `:331-335` calls the model from a daemon thread).  Operands on two
    different GPUs are rejected."""
    @functools.wraps(fn)
    def guarded(*args, **kwargs):
        dev = None
        for v in args + tuple(kwargs.values()):
            if isinstance(v, MatchPack):           # (a prepared gallery is an operand too: its buffers are what the kernel reads)
                v = getattr(v, "packed", None)     # (None inside its own constructor)
            if isinstance(v, torch.Tensor) and v.is_cuda:
                if dev is None:
                    dev = v.device
                elif v.device != dev:
                    raise ValueError(f"{fn.__name__}: operands live on different devices ({dev} and {v.device})")
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return guarded


def _dev(t: torch.Tensor, what: str, dtype=None, arg=None, owned: bool = False) -> torch.Tensor:
    """A tensor as the library takes it: on the GPU, of ``dtype``, contiguous and aligned as the header asks of ``arg`` =
    ``(entry point, argument)`` of `_lib.ALIGNMENT` (no ``arg``: 16 bytes, the most any operand needs).  An operand that is not
    contiguous or starts below that alignment - a view with a storage offset such as ``flat[1:]``, a row slice of a ``[B, 35]`` matrix -
    is copied; ``owned`` (a tensor the call writes: a state, a caller-supplied output) cannot be - the update would land in the copy -
    and raises ``ValueError`` in either case."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensor is on {t.device}; the HIP path needs GPU tensors (no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{what}: expected dtype {dtype}, got {t.dtype}")
    need = 16 if arg is None else _lib.align_of(*arg)
    if t.numel() and t.data_ptr() % need:
        if owned:
            raise ValueError(f"{what}: a tensor the call writes must be {need}-byte aligned (data_ptr() % {need} = {t.data_ptr() % need})")
        return t.clone(memory_format=torch.contiguous_format)
    if t.is_contiguous():
        return t
    if owned:
        raise ValueError(f"{what}: a tensor the call writes must be contiguous (shape {tuple(t.shape)}, strides {tuple(t.stride())}): "
                         f"a copy would take the update")
    return t.contiguous()


def _sized(t, op: str, name: str, shape, dtype=None) -> None:
    """Check an operand whose extent the library takes from ANOTHER operand's shape or from a scalar argument (a shift of ``Cout``
    values, a ``pos`` of ``[L, D]``): the library sees a bare pointer and would read past the end of a short one.  A tensor on the
    GPU (``RuntimeError``) of ``dtype`` (``TypeError``) and exactly ``shape`` (``ValueError``), before any pointer is taken."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{op}: {name}: expected a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{op}: {name} is on {t.device}; the HIP path needs GPU tensors (no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{op}: {name} must be {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(int(v) for v in shape):
        raise ValueError(f"{op}: {name} must be {list(int(v) for v in shape)}, got {list(t.shape)}")


def _ptr(keep: list, t: torch.Tensor, what: str, dtype=None, arg=None) -> int:
    """The address of ``_dev(t, ...)`` for an operand used by its address only.  `_dev` may have made a copy: it goes into ``keep``,
    which the caller holds until its launch is enqueued - a temporary dropped right after ``data_ptr()`` hands its block to the next
    copy, and two operands of one call would then share an address."""
    t = _dev(t, what, dtype, arg)
    keep.append(t)
    return t.data_ptr()


def dt_code(dtype: torch.dtype) -> int:
    try:
        return _DT[dtype]
    except KeyError:
        raise TypeError(f"compute dtype must be torch.bfloat16 or torch.float16, got {dtype}") from None


def set_batch_invariant(on: Optional[bool]) -> None:
    """``True``: kernel / tile-layout choices depend on the per-image geometry only, so a face's result is bit-identical in
    any batch, shard or rank (`frmap_set_batch_invariant`); ``False``: default planning (layouts follow the tile count: faster
    at small batches, results of different batch sizes agree to rounding); ``None``: the environment (FRMAP_BATCH_INVARIANT)."""
    _lib.check(_lib.load().frmap_set_batch_invariant(-1 if on is None else int(bool(on))), "set_batch_invariant")


def pack_input(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp32 NCHW B×3×H×W -> NHWC4 (zero 4th channel) in ``dtype``."""
    x = _dev(x, "pack_input.x", torch.float32, ("frmap_pack_input_nchw_f32", "x_nchw"))
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"expected B×3×H×W input, got {tuple(x.shape)}")
    B, _, H, W = x.shape
    out = torch.empty((B, H, W, 4), dtype=dtype, device=x.device)
    _lib.check(_lib.load().frmap_pack_input_nchw_f32(x.data_ptr(), out.data_ptr(), B, H, W, dt_code(dtype), _stream()),
               "pack_input")
    return out


def pack_conv_weight(w_folded: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    w = _dev(w_folded, "pack_conv_weight.w", torch.float32, ("frmap_pack_conv_weight", "w_oihw"))
    Cout, Cin, KH, KW = w.shape
    out = torch.empty((Cout * Cin * KH * KW,), dtype=dtype, device=w.device)
    _lib.check(_lib.load().frmap_pack_conv_weight(w.data_ptr(), out.data_ptr(), Cout, Cin, KH, KW, dt_code(dtype),
                                                  _stream()), "pack_conv_weight")
    return out


def pack_conv_weight_c3(w_folded: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    w = _dev(w_folded, "pack_conv_weight_c3.w", torch.float32, ("frmap_pack_conv_weight_c3", "w_oihw"))
    Cout, Cin, KH, KW = w.shape
    if Cin != 3:
        raise ValueError("pack_conv_weight_c3: Cin must be 3")
    lib = _lib.load()
    out = torch.empty((Cout * lib.frmap_small_cin_kpad(KH, KW),), dtype=dtype, device=w.device)
    _lib.check(lib.frmap_pack_conv_weight_c3(w.data_ptr(), out.data_ptr(), Cout, KH, KW, dt_code(dtype), _stream()),
               "pack_conv_weight_c3")
    return out


def conv_small_cin(x4: torch.Tensor, wpk: torch.Tensor, shift: torch.Tensor, Cout: int, k: int, stride: int,
                   pad: int, relu: bool) -> torch.Tensor:
    keep = []
    x4 = _dev(x4, "conv_small_cin.x", None, ("frmap_conv_small_cin", "in_nhwc4"))
    B, H, W, C = x4.shape
    if C != 4:
        raise ValueError("conv_small_cin: input must be NHWC4")
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    _sized(wpk, "conv_small_cin", "wpk", (Cout * _lib.load().frmap_small_cin_kpad(k, k),), x4.dtype)     # (`pack_conv_weight_c3`'s rows)
    _sized(shift, "conv_small_cin", "shift", (Cout,), torch.float32)
    out = torch.empty((B, Ho, Wo, Cout), dtype=x4.dtype, device=x4.device)
    _lib.check(_lib.load().frmap_conv_small_cin(x4.data_ptr(), _ptr(keep, wpk, "wpk"),
                                                _ptr(keep, shift, "shift", torch.float32), out.data_ptr(),
                                                B, H, W, Cout, k, k, stride, pad, int(relu), dt_code(x4.dtype),
                                                _stream()), "conv_small_cin")
    return out


def conv_small_cin_pool2(x4: torch.Tensor, wpk: torch.Tensor, shift: torch.Tensor, Cout: int, relu: bool) -> torch.Tensor:
    """3x3 s1 p1 conv (Cin = 3 as NHWC4) + shift (+ReLU) + MaxPool2d(2, 2) in one launch (`face_models.py:38`)."""
    keep = []
    x4 = _dev(x4, "conv_small_cin_pool2.x", None, ("frmap_conv_small_cin_pool2", "in_nhwc4"))
    B, H, W, C = x4.shape
    if C != 4:
        raise ValueError("conv_small_cin_pool2: input must be NHWC4")
    if H % 2 or W % 2:
        raise ValueError("conv_small_cin_pool2: H and W must be even")
    _sized(wpk, "conv_small_cin_pool2", "wpk", (Cout * _lib.load().frmap_small_cin_kpad(3, 3),), x4.dtype)
    _sized(shift, "conv_small_cin_pool2", "shift", (Cout,), torch.float32)
    out =torch.empty((B, H // 2, W // 2, Cout), dtype=x4.dtype, device=x4.device)
    _lib.check(_lib.load().frmap_conv_small_cin_pool2(x4.data_ptr(), _ptr(keep, wpk, "wpk"),
                                                      _ptr(keep, shift, "shift", torch.float32), out.data_ptr(),
                                                      B, H, W, Cout, int(relu), dt_code(x4.dtype), _stream()),
               "conv_small_cin_pool2")
    return out


def stem_pool_dims(H: int, W: int):
    Hc, Wc = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    return (Hc + 2 - 3) // 2 + 1, (Wc + 2 - 3) // 2 + 1


def stem7x7_maxpool(x: torch.Tensor, wpk: torch.Tensor, shift: torch.Tensor, dtype: torch.dtype,
                    pool3: bool = True) -> torch.Tensor:
    """fp32 NCHW -> conv7x7 s2 + shift + ReLU -> maxpool (3x3 s2 p1 if ``pool3`` else 2x2 s2) -> NHWC
    B×Hq×Wq×64 (``dtype``)."""
    keep = []
    x = _dev(x, "stem7x7_maxpool.x", torch.float32, ("frmap_stem7x7_maxpool", "x_nchw"))
    B, C, H, W = x.shape
    if C != 3:
        raise ValueError("stem7x7_maxpool: expected 3 input channels")
    if pool3:
        Hq, Wq = stem_pool_dims(H, W)
    else:
        Hq, Wq = ((H + 6 - 7) // 2 + 1) // 2, ((W + 6 - 7) // 2 + 1) // 2
    _sized(wpk, "stem7x7_maxpool", "wpk", (64 * _lib.load().frmap_small_cin_kpad(7, 7),), dtype)
    _sized(shift, "stem7x7_maxpool", "shift", (64,), torch.float32)
    out = torch.empty((B, Hq, Wq, 64), dtype=dtype, device=x.device)
    fn =_lib.load().frmap_stem7x7_maxpool if pool3 else _lib.load().frmap_stem7x7_maxpool2
    _lib.check(fn(x.data_ptr(), _ptr(keep, wpk, "wpk", dtype),
                                                 _ptr(keep, shift, "shift", torch.float32), out.data_ptr(),
                                                 B, H, W, dt_code(dtype), _stream()), "stem7x7_maxpool")
    return out


def stem7x7_maxpool_u8(x_u8: torch.Tensor, wpk: torch.Tensor, shift: torch.Tensor, mean, std, dtype: torch.dtype,
                       pool3: bool = True) -> torch.Tensor:
    """uint8 HWC B×H×W×3 (RGB) -> ToTensor + Normalize(mean, std) -> conv7x7 s2 + shift + ReLU -> maxpool -> NHWC
    B×Hq×Wq×64 (``dtype``): the fused stem fed by the image bytes themselves (needs W % 4 == 0)."""
    keep = []
    import ctypes as C
    if not isinstance(x_u8, torch.Tensor) or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3] != 3:
        raise TypeError("stem7x7_maxpool_u8: expected a uint8 tensor of shape [B, H, W, 3]")
    x_u8 = _dev(x_u8, "stem7x7_maxpool_u8.x", None, ("frmap_stem7x7_maxpool_u8", "x_u8_hwc"))
    B, H, W, _ = x_u8.shape
    if pool3:
        Hq, Wq = stem_pool_dims(H, W)
    else:
        Hq, Wq = ((H + 6 - 7) // 2 + 1) // 2, ((W + 6 - 7) // 2 + 1) // 2
    _sized(wpk, "stem7x7_maxpool_u8", "wpk", (64 * _lib.load().frmap_small_cin_kpad(7, 7),), dtype)
    _sized(shift, "stem7x7_maxpool_u8", "shift", (64,), torch.float32)
    out = torch.empty((B, Hq, Wq, 64), dtype=dtype, device=x_u8.device)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    sd = (C.c_float * 3)(*[float(v) for v in std])
    _lib.check(_lib.load().frmap_stem7x7_maxpool_u8(x_u8.data_ptr(), m, sd, _ptr(keep, wpk, "wpk", dtype),
                                                    _ptr(keep, shift, "shift", torch.float32), out.data_ptr(),
                                                    B, H, W, int(bool(pool3)), dt_code(dtype), _stream()), "stem7x7_maxpool_u8")
    return out


def conv_igemm(x: torch.Tensor, wpk: torch.Tensor, shift: torch.Tensor, Cout: int, k: int, stride: int, pad: int,
               relu, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``relu``: False/0 none, True/1 ReLU, 2 exact GELU."""
    keep = []
    x = _dev(x, "conv_igemm.x")
    B, H, W, Cin = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = torch.empty((B, Ho, Wo, Cout), dtype=x.dtype, device=x.device)
    res_ptr = 0
    if residual is not None:
        residual = _dev(residual, "conv_igemm.residual", x.dtype)
        if tuple(residual.shape) != tuple(out.shape):
            raise ValueError(f"conv_igemm: residual shape {tuple(residual.shape)} != output {tuple(out.shape)}")
        res_ptr = residual.data_ptr()
    _sized(wpk, "conv_igemm", "wpk", (Cout * Cin * k * k,), x.dtype)
    _sized(shift, "conv_igemm", "shift", (Cout,), torch.float32)
    _lib.check(_lib.load().frmap_conv_igemm(x.data_ptr(), _ptr(keep, wpk, "wpk"),
                                            _ptr(keep, shift, "shift", torch.float32), res_ptr, out.data_ptr(),
                                            B, H, W, Cin, Cout, k, stride, pad, int(relu), dt_code(x.dtype),
                                            _stream()), "conv_igemm")
    return out


FUSE_NONE, FUSE_RESIDUAL, FUSE_SHORTCUT, FUSE_POOL2 = 0, 1, 2, 3


def conv_plan_key(B: int, H: int, W: int, Cin: int, Cout: int, k: int = 3, stride: int = 1, fuse: int = FUSE_NONE,
                  ds: Optional[tuple] = None) -> str:
    """The kernel instantiation `conv_igemm` (fuse 0 / 1: without / with a residual), `conv_igemm_ds` (fuse 2, ``ds`` = (dsH, dsW,
    dsCin, ds_stride)) or `conv_igemm_pool2` (fuse 3) launches for the layer under the tuning and hooks now in force, by its
    canonical name without the data type (`frmap_conv_plan_key`), e.g. ``"conv3x3_pp_kernel<7,2,5,1,DS>"``; ``""`` where the
    launcher would refuse the layer (the reason is `frmap_last_error`).  Nothing is launched; no GPU is needed."""
    import ctypes as C
    buf = C.create_string_buffer(96)
    dsH, dsW, dsC, sd = ds if ds is not None else (0, 0, 0, 0)
    n = _lib.load().frmap_conv_plan_key(B, H, W, Cin, Cout, k, stride, fuse, dsH, dsW, dsC, sd, buf, len(buf))
    if n < 0:
        _lib.check(n, "conv_plan_key")
    return buf.value.decode()


def conv_plan_keys() -> list:
    """Every key `conv_plan_key` can answer: one per kernel instantiation the conv launchers can dispatch."""
    import ctypes as C
    lib, buf = _lib.load(), C.create_string_buffer(96)
    out = []
    for i in range(lib.frmap_conv_plan_keys(-1, buf, len(buf))):
        lib.frmap_conv_plan_keys(i, buf, len(buf))
        out.append(buf.value.decode())
    return out


def conv_plan_selfcheck() -> None:
    """Raises unless the launch tables hold a kernel of its own for every (key, data type) (`frmap_conv_plan_selfcheck`)."""
    _lib.check(_lib.load().frmap_conv_plan_selfcheck(), "conv_plan_selfcheck")


_pool2_cache: dict = {}


def conv_pool2_supported(B: int, H: int, W: int, Cin: int, Cout: int) -> bool:
    """True when fusing the 2x2 max-pool into the conv is expected to win (see `frmap_conv_igemm_pool2_supported`)."""
    key = (B, H, W, Cin, Cout)
    if key not in _pool2_cache:
        _pool2_cache[key] = bool(_lib.load().frmap_conv_igemm_pool2_supported(B, H, W, Cin, Cout))
    return _pool2_cache[key]


def conv_pool2_form(B: int, H: int, W: int, Cin: int, Cout: int) -> int:
    """3 = ping-pong kernel, 2 = wave kernel, 1 = generic kernel, 0 = `conv_igemm_pool2` rejects the shape."""
    return int(_lib.load().frmap_conv_igemm_pool2_form(B, H, W, Cin, Cout))


def conv_igemm_pool2(x: torch.Tensor, wpk: torch.Tensor, shift: torch.Tensor, Cout: int, relu) -> torch.Tensor:
    """conv 3x3 s1 p1 + shift (+ReLU) + MaxPool2d(2, 2) in one launch (`face_models.py:39-40,121-141`); the conv map
    never reaches HBM.  Raises ``ValueError`` for shapes `conv_pool2_supported` rejects."""
    keep = []
    x = _dev(x, "conv_igemm_pool2.x")
    B, H, W, Cin = x.shape
    _sized(wpk, "conv_igemm_pool2", "wpk", (Cout * Cin * 9,), x.dtype)
    _sized(shift, "conv_igemm_pool2", "shift", (Cout,), torch.float32)
    out = torch.empty((B, H // 2, W // 2, Cout), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().frmap_conv_igemm_pool2(x.data_ptr(), _ptr(keep, wpk, "wpk"),
                                                  _ptr(keep, shift, "shift", torch.float32), out.data_ptr(),
                                                  B, H, W, Cin, Cout, int(relu), dt_code(x.dtype), _stream()),
               "conv_igemm_pool2")
    return out


_ds_ok_cache: dict = {}


def conv_ds_supported(B: int, H: int, W: int, Cin: int, Cout: int, dsH: int, dsW: int, dsCin: int, ds_stride: int) -> bool:
    key = (B, H, W, Cin, Cout, dsH, dsW, dsCin, ds_stride)
    v = _ds_ok_cache.get(key)
    if v is None:
        v = _ds_ok_cache[key] = bool(_lib.load().frmap_conv_igemm_ds_supported(*key))
    return v


def conv_igemm_ds(x: torch.Tensor, wpk: torch.Tensor, shift: torch.Tensor, Cout: int, x_ds: torch.Tensor, wpk_ds: torch.Tensor,
                  ds_stride: int, relu) -> torch.Tensor:
    """``act(conv3x3_s1_p1(x) + conv1x1_stride(x_ds) + shift)`` — a BasicBlock's second conv with its projection
    shortcut folded in (``shift`` = both folded BatchNorm shifts added).  Check ``conv_ds_supported`` first."""
    keep = []
    x = _dev(x, "conv_igemm_ds.x")
    x_ds = _dev(x_ds, "conv_igemm_ds.x_ds", x.dtype)
    if x.dim() != 4 or x_ds.dim() != 4:
        raise ValueError(f"conv_igemm_ds: x and x_ds must be NHWC maps, got {list(x.shape)} and {list(x_ds.shape)}")
    B, H, W, Cin = x.shape
    Bd, Hd, Wd, Cd = x_ds.shape
    if Bd != B:
        raise ValueError(f"conv_igemm_ds: x_ds holds {Bd} images, x {B}")
    _sized(wpk, "conv_igemm_ds", "wpk", (Cout * Cin * 9,), x.dtype)
    _sized(wpk_ds, "conv_igemm_ds", "wpk_ds", (Cout * Cd,), x.dtype)
    _sized(shift, "conv_igemm_ds", "shift", (Cout,), torch.float32)
    out = torch.empty((B, H, W, Cout), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().frmap_conv_igemm_ds(x.data_ptr(), _ptr(keep, wpk, "wpk"),
                                               _ptr(keep, shift, "shift", torch.float32), x_ds.data_ptr(),
                                               _ptr(keep, wpk_ds, "wpk_ds"), out.data_ptr(), B, H, W, Cin, Cout,
                                               Hd, Wd, Cd, ds_stride, int(relu), dt_code(x.dtype), _stream()), "conv_igemm_ds")
    return out


def linear_mfma(x2d: torch.Tensor, wpk: torch.Tensor, shift: torch.Tensor, N: int, act=0,
                residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``act(x · Wᵀ + shift [+ residual])`` on the MFMA conv kernel (split-K when the output is small)."""
    keep = []
    x2d = _dev(x2d, "linear_mfma.x")
    M, K = x2d.shape
    out = torch.empty((M, N), dtype=x2d.dtype, device=x2d.device)
    lib = _lib.load()
    nbytes = lib.frmap_linear_mfma_workspace_bytes(M, K, N)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=x2d.device) if nbytes else None
    rp = 0
    if residual is not None:
        residual = _dev(residual, "linear_mfma.residual", x2d.dtype)
        if tuple(residual.shape) != (M, N):
            raise ValueError("linear_mfma: residual must be [M, N]")
        rp = residual.data_ptr()
    _sized(wpk, "linear_mfma", "wpk", (N * K,), x2d.dtype)
    _sized(shift, "linear_mfma", "shift", (N,), torch.float32)
    _lib.check(lib.frmap_linear_mfma(x2d.data_ptr(), _ptr(keep, wpk, "wpk"), _ptr(keep, shift, "shift", torch.float32),
                                     rp, out.data_ptr(), ws.data_ptr() if ws is not None else 0, M, K, N, int(act),
                                     dt_code(x2d.dtype), _stream()), "linear_mfma")
    return out


def maxpool(x: torch.Tensor, k: int, stride: int, pad: int) -> torch.Tensor:
    x = _dev(x, "maxpool.x")
    B, H, W, Cc = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = torch.empty((B, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().frmap_maxpool(x.data_ptr(), out.data_ptr(), B, H, W, Cc, k, stride, pad, dt_code(x.dtype),
                                         _stream()), "maxpool")
    return out


def avgpool_global(x: torch.Tensor) -> torch.Tensor:
    x = _dev(x, "avgpool_global.x")
    B, H, W, Cc = x.shape
    out = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().frmap_avgpool_global(x.data_ptr(), out.data_ptr(), B, H * W, Cc, dt_code(x.dtype),
                                                _stream()), "avgpool_global")
    return out


def avgpool_adaptive(x: torch.Tensor, OH: int, OW: int) -> torch.Tensor:
    x = _dev(x, "avgpool_adaptive.x")
    B, H, W, Cc = x.shape
    out = torch.empty((B, OH, OW, Cc), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().frmap_avgpool_adaptive(x.data_ptr(), out.data_ptr(), B, H, W, Cc, OH, OW,
                                                  dt_code(x.dtype), _stream()), "avgpool_adaptive")
    return out


def linear_f32(x: torch.Tensor, w: torch.Tensor, scale: Optional[torch.Tensor] = None,
               shift: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
    keep = []
    x = _dev(x, "linear_f32.x", torch.float32)
    w = _dev(w, "linear_f32.w", torch.float32)
    if x.dim() != 2 or w.dim() != 2:
        raise ValueError(f"linear_f32: x [B, K] and w [N, K] expected, got {list(x.shape)} and {list(w.shape)}")
    B, K = x.shape
    N, K2 = w.shape
    if K != K2:
        raise ValueError(f"linear_f32: x is B×{K} but w is N×{K2}")
    if scale is not None:
        _sized(scale, "linear_f32", "scale", (N,), torch.float32)
    if shift is not None:
        _sized(shift, "linear_f32", "shift", (N,), torch.float32)
    out =torch.empty((B, N), dtype=torch.float32, device=x.device)
    sp = _ptr(keep, scale, "scale", torch.float32, ("frmap_linear_f32", "scale")) if scale is not None else 0
    hp = _ptr(keep, shift, "shift", torch.float32, ("frmap_linear_f32", "shift")) if shift is not None else 0
    _lib.check(_lib.load().frmap_linear_f32(x.data_ptr(), w.data_ptr(), sp, hp, out.data_ptr(), B, K, N, int(relu),
                                            _stream()), "linear_f32")
    return out


def l2_normalize(x: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    x = _dev(x, "l2_normalize.x", torch.float32, ("frmap_l2_normalize_f32", "x"))
    B, D = x.shape
    out = torch.empty_like(x)
    _lib.check(_lib.load().frmap_l2_normalize_f32(x.data_ptr(), out.data_ptr(), B, D, float(eps), _stream()),
               "l2_normalize")
    return out


def cast_to_f32(x: torch.Tensor) -> torch.Tensor:
    x = _dev(x, "cast_to_f32.x", None, ("frmap_cast_to_f32", "in"))
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().frmap_cast_to_f32(x.data_ptr(), out.data_ptr(), x.numel(), dt_code(x.dtype), _stream()),
               "cast_to_f32")
    return out


def cast_from_f32(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    x = _dev(x, "cast_from_f32.x", torch.float32, ("frmap_cast_from_f32", "in"))
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    _lib.check(_lib.load().frmap_cast_from_f32(x.data_ptr(), out.data_ptr(), x.numel(), dt_code(dtype), _stream()),
               "cast_from_f32")
    return out


def add_pos_layernorm(x: torch.Tensor, pos: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                      eps: float = 1e-5, want_sum: bool = False):
    """x: [B, L, D] tokens.  Returns (t, y): t = x + pos (None unless want_sum), y = LayerNorm(t)."""
    keep = []
    x = _dev(x, "add_pos_layernorm.x")
    B, L, D = x.shape
    if pos is not None:
        _sized(pos, "add_pos_layernorm", "pos", (L, D), torch.float32)
    _sized(gamma, "add_pos_layernorm", "gamma", (D,), torch.float32)
    _sized(beta, "add_pos_layernorm", "beta", (D,), torch.float32)
    y = torch.empty_like(x)
    t = torch.empty_like(x) if want_sum else None
    _lib.check(_lib.load().frmap_add_pos_layernorm(
        x.data_ptr(), _ptr(keep, pos, "pos", torch.float32) if pos is not None else 0,
        _ptr(keep, gamma, "gamma", torch.float32), _ptr(keep, beta, "beta", torch.float32),
        t.data_ptr() if t is not None else 0, y.data_ptr(), B, L, D, float(eps), dt_code(x.dtype), _stream()),
        "add_pos_layernorm")
    return t, y


def mha_tokens(qkv: torch.Tensor, H: int) -> torch.Tensor:
    qkv = _dev(qkv, "mha_tokens.qkv")
    if qkv.dim() != 3 or qkv.shape[2] % 3:
        raise ValueError(f"mha_tokens: qkv must be [B, L, 3 D] (q | k | v), got {list(qkv.shape)}")
    B, L, D3 = qkv.shape
    D = D3 // 3          # (D = 128 H is the launcher's to refuse: it is given both)
    out = torch.empty((B, L, D), dtype=qkv.dtype, device=qkv.device)
    _lib.check(_lib.load().frmap_mha_tokens(qkv.data_ptr(), out.data_ptr(), B, L, D, H, dt_code(qkv.dtype), _stream()),
               "mha_tokens")
    return out


def mean_layernorm(t: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    keep = []
    t = _dev(t, "mean_layernorm.t")
    B, L, D = t.shape
    _sized(gamma, "mean_layernorm", "gamma", (D,), torch.float32)
    _sized(beta, "mean_layernorm", "beta", (D,), torch.float32)
    out = torch.empty((B, D), dtype=torch.float32, device=t.device)
    _lib.check(_lib.load().frmap_mean_layernorm(t.data_ptr(), _ptr(keep, gamma, "gamma", torch.float32, ("frmap_mean_layernorm", "gamma")),
                                                _ptr(keep, beta, "beta", torch.float32, ("frmap_mean_layernorm", "beta")), out.data_ptr(), B, L, D,
                                                float(eps), dt_code(t.dtype), _stream()), "mean_layernorm")
    return out


def cnn_attention(qkv: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, spatial_w: torch.Tensor, spatial_b: torch.Tensor,
                  Cq: int, want_map: bool = False, want_pool: bool = True):
    """AttentionNet's attention block (`face_models.py:194-262`) on an NHWC trunk map ``x`` [B,H,W,C] given the packed
    q|k|v projection ``qkv`` [B,H,W,2*Cq+C].  Returns (map [B,H,W,C] | None, pooled fp32 [B,C] | None)."""
    keep = []
    x = _dev(x, "cnn_attention.x")
    qkv = _dev(qkv, "cnn_attention.qkv", x.dtype)
    B, H, W, C = x.shape
    if tuple(qkv.shape) != (B, H, W, 2 * Cq + C):
        raise ValueError(f"cnn_attention: qkv shape {tuple(qkv.shape)} != {(B, H, W, 2 * Cq + C)}")
    sw = _dev(spatial_w, "spatial_w", torch.float32, ("frmap_cnn_attention", "spatial_w"))
    KS = sw.shape[-1]
    if sw.numel() != 2 * KS * KS:
        raise ValueError("cnn_attention: spatial_w must be [1][2][KS][KS]")
    _sized(gamma, "cnn_attention", "gamma", (1,), torch.float32)
    _sized(spatial_b, "cnn_attention", "spatial_b", (1,), torch.float32)
    om = torch.empty((B, H, W, C), dtype=x.dtype, device=x.device) if want_map else None
    op = torch.empty((B, C), dtype=torch.float32, device=x.device) if want_pool else None
    _lib.check(_lib.load().frmap_cnn_attention(qkv.data_ptr(), x.data_ptr(), _ptr(keep, gamma, "gamma", torch.float32, ("frmap_cnn_attention", "gamma")),
                                               sw.data_ptr(), _ptr(keep, spatial_b, "spatial_b", torch.float32, ("frmap_cnn_attention", "spatial_b")),
                                               om.data_ptr() if om is not None else 0, op.data_ptr() if op is not None else 0,
                                               B, H, W, Cq, C, KS, dt_code(x.dtype), _stream()), "cnn_attention")
    return om, op


def normalize_u8(img: torch.Tensor, mean, std, want_nchw: bool = True, nhwc4_dtype: Optional[torch.dtype] = None):
    """uint8 [B, H, W, 3] RGB on the GPU → ToTensor + Normalize.  Returns (fp32 NCHW | None, NHWC4 | None)."""
    import ctypes as C
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3:
        raise TypeError("normalize_u8: expected a uint8 tensor of shape [B, H, W, 3]")
    img = _dev(img, "normalize_u8.img", None, ("frmap_normalize_u8_hwc", "img_u8"))
    B, H, W, _ = img.shape
    o1 = torch.empty((B, 3, H, W), dtype=torch.float32, device=img.device) if want_nchw else None
    o2 = torch.empty((B, H, W, 4), dtype=nhwc4_dtype, device=img.device) if nhwc4_dtype is not None else None
    m = (C.c_float * 3)(*[float(v) for v in mean])
    sd = (C.c_float * 3)(*[float(v) for v in std])
    _lib.check(_lib.load().frmap_normalize_u8_hwc(img.data_ptr(), o1.data_ptr() if o1 is not None else 0,
                                                  o2.data_ptr() if o2 is not None else 0, B, H, W, m, sd,
                                                  dt_code(nhwc4_dtype) if nhwc4_dtype is not None else BF16, _stream()),
               "normalize_u8")
    return o1, o2


def softmax_argmax(logits: torch.Tensor, want_probs: bool = True):
    logits = _dev(logits, "softmax_argmax.logits", torch.float32, ("frmap_softmax_argmax", "logits"))
    B, Cc = logits.shape
    probs = torch.empty_like(logits) if want_probs else None
    pred = torch.empty((B,), dtype=torch.int32, device=logits.device)
    _lib.check(_lib.load().frmap_softmax_argmax(logits.data_ptr(), probs.data_ptr() if want_probs else 0, pred.data_ptr(),
                                                B, Cc, _stream()), "softmax_argmax")
    return probs, pred


def pairwise_distance(a: torch.Tensor, b: torch.Tensor, thresh: Optional[float] = None):
    a = _dev(a, "pairwise_distance.a", torch.float32, ("frmap_pairwise_distance", "a"))
    b = _dev(b, "pairwise_distance.b", torch.float32, ("frmap_pairwise_distance", "b"))
    if a.shape != b.shape or a.dim() != 2:
        raise ValueError(f"pairwise_distance: a and b must be two [B, D] tensors of the same shape, got {list(a.shape)} and {list(b.shape)}")
    B, D = a.shape
    dist = torch.empty((B,), dtype=torch.float32, device=a.device)
    same = torch.empty((B,), dtype=torch.int32, device=a.device) if thresh is not None else None
    _lib.check(_lib.load().frmap_pairwise_distance(a.data_ptr(), b.data_ptr(), dist.data_ptr(),
                                                   same.data_ptr() if same is not None else 0,
                                                   float(thresh) if thresh is not None else 0.0, B, D, _stream()),
               "pairwise_distance")
    return dist, same


# ------------------------------------------------------------------------------------------------
# classification tally (`frmap_classify_tally*`, csrc/classify_tally.hip; the rule is `evaluate.tally_rule`)
# ------------------------------------------------------------------------------------------------
TALLY_HEADER = ("rows", "ignored", "nonfinite", "correct", "loss_q")     # words 0 .. 4 of the 8-word header
TALLY_MAX_RANKS = TALLY_MAX_BINS = 1024
TALLY_MAX_CONFUSION_CLASSES = 4096


def classify_tally_words(C: int, ranks: int = 6, n_bins: int = 10, confusion: bool = True) -> int:
    """uint64 words of a tally state (`frmap_classify_tally_words`); ``ValueError`` for a shape the launcher refuses."""
    n = int(_lib.load().frmap_classify_tally_words(int(C), int(ranks), int(n_bins), int(bool(confusion))))
    if n == 0:
        raise ValueError(f"classify_tally: unsupported C = {C}, ranks = {ranks}, n_bins = {n_bins}, confusion = {confusion} (C >= 1, ranks "
                         f"and n_bins in 1 ... {TALLY_MAX_RANKS}, a kept confusion matrix up to C = {TALLY_MAX_CONFUSION_CLASSES})")
    return n


def classify_tally_layout(C: int, ranks: int = 6, n_bins: int = 10, confusion: bool = True) -> dict:
    """name -> slice of the state, in the order of the state: the five header counters (one word each), ``rank_hist`` [ranks],
    ``support`` / ``predicted`` / ``hit`` [C], ``bin_count`` / ``bin_correct`` / ``bin_conf_q`` [n_bins] and, when kept,
    ``confusion`` [C * C] (row = label, column = prediction)."""
    words = classify_tally_words(C, ranks, n_bins, confusion)
    out = {name: slice(k, k + 1) for k, name in enumerate(TALLY_HEADER)}
    at = 8
    for name, n in (("rank_hist", ranks), ("support", C), ("predicted", C), ("hit", C), ("bin_count", n_bins), ("bin_correct", n_bins),
                    ("bin_conf_q", n_bins)) + ((("confusion", C * C),) if confusion else ()):
        out[name] = slice(at, at + int(n))
        at += int(n)
    assert at == words, (at, words)
    return out


def classify_tally(logits: torch.Tensor, labels: torch.Tensor, state: Optional[torch.Tensor] = None, ranks: int = 6, n_bins: int = 10,
                   confusion: bool = True, want_rows: bool = False):
    """Add a batch to a classification tally in one launch on the current stream (`frmap_classify_tally`; nothing is copied or
    synchronised).  ``logits`` float32 ``[B, C]``, ``labels`` int32 ``[B]`` (a label outside ``[0, C)`` declines its row, and so
    does a non-finite logit); ``state``: an int64 tensor of `classify_tally_words` words from an earlier call with the same ``C``,
    ``ranks``, ``n_bins`` and ``confusion`` (updated in place), or ``None`` for a fresh, zeroed one.  Returns the state, or with
    ``want_rows`` ``(state, (pred int32, rank int32, conf float32, loss float32))``, the row records of the rule."""
    # (a non-contiguous operand is copied by `_dev`; the copies live in these names until the launch is enqueued)
    logits = _dev(logits, "classify_tally.logits", torch.float32, ("frmap_classify_tally", "logits"))
    labels = _dev(labels, "classify_tally.labels", torch.int32, ("frmap_classify_tally", "labels"))
    if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
        raise ValueError(f"classify_tally: logits [B, C] and labels [B] expected, got {tuple(logits.shape)} and {tuple(labels.shape)}")
    B, Cc = int(logits.shape[0]), int(logits.shape[1])
    words = classify_tally_words(Cc, ranks, n_bins, confusion)
    if state is None:
        state = torch.zeros((words,), dtype=torch.int64, device=logits.device)
    else:
        state = _dev(state, "classify_tally.state", torch.int64, ("frmap_classify_tally", "state"), owned=True)
        if state.dim() != 1 or state.numel() != words or not state.is_contiguous():
            raise ValueError(f"classify_tally: state holds {state.numel()} words, C = {Cc}, ranks = {ranks}, n_bins = {n_bins}, "
                             f"confusion = {bool(confusion)} need {words}")
    rows = None
    if want_rows:
        rows = (torch.empty((B,), dtype=torch.int32, device=logits.device), torch.empty((B,), dtype=torch.int32, device=logits.device),
                torch.empty((B,), dtype=torch.float32, device=logits.device), torch.empty((B,), dtype=torch.float32, device=logits.device))
    _lib.check(_lib.load().frmap_classify_tally(logits.data_ptr(), labels.data_ptr(), B, Cc, int(ranks), int(n_bins), int(bool(confusion)),
                                                state.data_ptr(), *((t.data_ptr() for t in rows) if want_rows else (0, 0, 0, 0)), _stream()),
               "classify_tally")
    return (state, rows) if want_rows else state


def classify_tally_host(logits, labels, row_conf, row_loss, state: Optional[np.ndarray] = None, ranks: int = 6, n_bins: int = 10,
                        confusion: bool = True):
    """The accumulation of `classify_tally` on the CPU over numpy arrays (`frmap_classify_tally_host`: the kernel's rule header
    compiled for the host; no GPU).  ``row_conf`` / ``row_loss`` float32 ``[B]`` are INPUTS (the device's own row records, or any
    values to be tallied); pred and rank are computed from the logits.  ``state``: a writable uint64 array (updated in place) or
    ``None`` for a fresh one.  Returns ``(state, pred int32, rank int32)``."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    row_conf = np.ascontiguousarray(row_conf, dtype=np.float32)
    row_loss = np.ascontiguousarray(row_loss, dtype=np.float32)
    if logits.ndim != 2 or labels.shape != (logits.shape[0],) or row_conf.shape != labels.shape or row_loss.shape != labels.shape:
        raise ValueError("classify_tally_host: logits [B, C] and labels, row_conf, row_loss [B] expected")
    B, Cc = logits.shape
    words = classify_tally_words(Cc, ranks, n_bins, confusion)
    if state is None:
        state = np.zeros((words,), np.uint64)
    if not (isinstance(state, np.ndarray) and state.dtype == np.uint64 and state.flags.c_contiguous and state.flags.writeable
            and state.shape == (words,)):
        raise ValueError(f"classify_tally_host: state must be a writable contiguous uint64 array of {words} words")
    pred, rank = np.empty((B,), np.int32), np.empty((B,), np.int32)
    _lib.check(_lib.load().frmap_classify_tally_host(logits.ctypes.data, labels.ctypes.data, B, Cc, int(ranks), int(n_bins),
                                                     int(bool(confusion)), state.ctypes.data, pred.ctypes.data, rank.ctypes.data,
                                                     row_conf.ctypes.data, row_loss.ctypes.data), "classify_tally_host")
    return state, pred, rank


# ------------------------------------------------------------------------------------------------
# one-vs-rest rank counts (`frmap_ovr_*`, csrc/ovr_rank.hip; the rule is `evaluate.ovr_rank_rule`)
# ------------------------------------------------------------------------------------------------
OVR_IGNORED, OVR_NONFINITE = -1, -2         # the stored label of a declined row


def _ovr_store(what: str, entry: str, store: torch.Tensor, store_labels: torch.Tensor, written: bool):
    """A score store as the library takes it, and its ``(C, capacity)``: ``store`` float32 ``[C, capacity]`` class-major,
    ``store_labels`` int32 ``[capacity]``.  A store the call writes must be contiguous and aligned as it stands."""
    if written and not (isinstance(store, torch.Tensor) and isinstance(store_labels, torch.Tensor) and store.is_contiguous()
                        and store_labels.is_contiguous()):
        raise ValueError(f"{what}: store and store_labels are written in place and must be contiguous tensors")
    store = _dev(store, f"{what}.store", torch.float32, (entry, "store"), owned=written)
    store_labels = _dev(store_labels, f"{what}.store_labels", torch.int32, (entry, "store_labels"), owned=written)
    if store.dim() != 2 or store_labels.dim() != 1 or store_labels.shape[0] != store.shape[1] or store.shape[0] < 1:
        raise ValueError(f"{what}: store [C, capacity] and store_labels [capacity] expected, got {tuple(store.shape)} and "
                         f"{tuple(store_labels.shape)}")
    return store, store_labels, int(store.shape[0]), int(store.shape[1])


def ovr_append(scores: torch.Tensor, labels: torch.Tensor, store: torch.Tensor, store_labels: torch.Tensor, first: int) -> None:
    """Append a batch to a score store in one launch on the current stream (`frmap_ovr_append`; nothing is copied back or
    synchronised).  ``scores`` float32 ``[B, C]``, ``labels`` int32 ``[B]``; ``store`` float32 ``[C, capacity]`` (class-major) and
    ``store_labels`` int32 ``[capacity]`` are written in place at rows ``[first, first + B)``: ``store[c, first + b] = scores[b, c]``,
    ``store_labels[first + b]`` = the label, or -1 for a label outside ``[0, C)``, or -2 for a non-finite score under a valid label."""
    keep = []
    store, store_labels, Cc, cap = _ovr_store("ovr_append", "frmap_ovr_append", store, store_labels, True)
    ps = _ptr(keep, scores, "ovr_append.scores", torch.float32, ("frmap_ovr_append", "scores"))
    pl = _ptr(keep, labels, "ovr_append.labels", torch.int32, ("frmap_ovr_append", "labels"))
    scores, labels = keep
    if scores.dim() != 2 or labels.dim() != 1 or labels.shape[0] != scores.shape[0] or scores.shape[1] != Cc:
        raise ValueError(f"ovr_append: scores [B, {Cc}] and labels [B] expected, got {tuple(scores.shape)} and {tuple(labels.shape)}")
    _lib.check(_lib.load().frmap_ovr_append(ps, pl, int(scores.shape[0]), Cc, store.data_ptr(), store_labels.data_ptr(), cap, int(first),
                                            _stream()), "ovr_append")


def ovr_rank_counts(store: torch.Tensor, store_labels: torch.Tensor, n: int):
    """The three exact integers of every row ``i < n`` of a score store (`frmap_ovr_rank_counts`: two launches on the
    current stream, no synchronisation): ``(ge_same, ge_other, eq_other)``, int64 ``[n]`` each (uint64 words) - over the counted
    rows j < n, those of i's class (i included) / of another class whose score in i's class column is >= i's, and those of another
    class whose score there equals i's.  A declined row (stored label < 0) gets 0, 0, 0 and takes part in nobody's count."""
    # (a non-contiguous store is copied by `_dev`; the copies live in these names until the launch is enqueued)
    store, store_labels, Cc, cap = _ovr_store("ovr_rank_counts", "frmap_ovr_rank_counts", store, store_labels, False)
    n = int(n)
    if not 0 <= n <= cap:
        raise ValueError(f"ovr_rank_counts: n = {n} rows of a store of capacity {cap}")
    out = tuple(torch.empty((n,), dtype=torch.int64, device=store.device) for _ in range(3))
    if n:
        _lib.check(_lib.load().frmap_ovr_rank_counts(store.data_ptr(), store_labels.data_ptr(), n, cap, Cc, out[0].data_ptr(),
                                                     out[1].data_ptr(), out[2].data_ptr(), _stream()), "ovr_rank_counts")
    return out


def ovr_rank_counts_host(store, store_labels, n: Optional[int] = None):
    """`ovr_rank_counts` on the CPU over numpy arrays (`frmap_ovr_rank_counts_host`: the kernel's rule header compiled for the
    host; no GPU).  ``store`` float32 ``[C, capacity]``, ``store_labels`` int32 ``[capacity]``; ``n`` defaults to the capacity.
    Returns ``(ge_same, ge_other, eq_other)`` as uint64 ``[n]`` arrays."""
    store = np.ascontiguousarray(store, dtype=np.float32)
    store_labels = np.ascontiguousarray(store_labels, dtype=np.int32)
    if store.ndim != 2 or store.shape[0] < 1 or store_labels.shape != (store.shape[1],):
        raise ValueError("ovr_rank_counts_host: store [C, capacity] and store_labels [capacity] expected")
    Cc, cap = store.shape
    n = cap if n is None else int(n)
    out = tuple(np.empty((max(n, 0),), np.uint64) for _ in range(3))
    _lib.check(_lib.load().frmap_ovr_rank_counts_host(store.ctypes.data if cap else None, store_labels.ctypes.data if cap else None, n, cap,
                                                      Cc, *(o.ctypes.data if n > 0 else None for o in out)), "ovr_rank_counts_host")
    return out


def _workspace(B: int, Cc: int, device) -> torch.Tensor:
    n = _lib.load().frmap_head_workspace_bytes(B, Cc)
    return torch.empty(((n + 15) // 16) * 2, dtype=torch.int64, device=device)


def _match_workspace(B: int, G: int, device) -> torch.Tensor:
    n = _lib.load().frmap_match_workspace_bytes(B, G)
    return torch.empty(((n + 15) // 16) * 2, dtype=torch.int64, device=device)


def _packed_buf(packed, B: int, device):
    """``packed``: False/None -> no record output; True -> a fresh int32 [B, 2]; a tensor -> written in place (a
    contiguous int32 [B, 2] view, e.g. one micro-batch's slice of the step's record buffer)."""
    if packed is None or packed is False:
        return None
    if packed is True:
        return torch.empty((B, 2), dtype=torch.int32, device=device)
    _sized(packed, "match", "packed", (B, 2), torch.int32)
    if not packed.is_contiguous():
        raise ValueError(f"packed output must be a contiguous int32 [{B}, 2] device tensor")
    return _dev(packed, "packed", torch.int32, ("frmap_match_top1", "packed_out"), owned=True)     # (caller-owned: never copied)


class MatchPack:
    """A gallery prepared for the MFMA match path (`frmap_match_pack_gallery`): the fp32 rows split into fp16 (hi, lo)
    pairs in the GEMM kernel's operand order, plus the per-row statistics of the expanded distance.  ``capacity`` > G
    leaves room for `update_rows` (incremental enrolment: only the touched 64-row tiles are re-packed)."""
    __slots__ = ("packed", "stat_w", "G", "D", "capacity", "src_ptr", "src_version", "src_stride", "ready")

    def __init__(self, gallery: torch.Tensor, capacity: Optional[int] = None):
        src, gallery = gallery, _dev(gallery, "match_prepare.gallery", torch.float32, ("frmap_match_pack_gallery", "gallery"))
        if gallery.dim() != 2:
            raise ValueError(f"match_prepare: gallery must be [G, D], got {list(gallery.shape)}")
        self.G, self.D = int(gallery.shape[0]), int(gallery.shape[1])
        self.capacity = max(int(capacity or 0), self.G)
        lib = _lib.load()
        self.packed = torch.empty((lib.frmap_match_gallery_pack_bytes(self.capacity, self.D),), dtype=torch.uint8, device=gallery.device)
        self.stat_w = torch.empty((self.capacity, 4), dtype=torch.float32, device=gallery.device)
        # (the CALLER's tensor is what `matches` recognises, not a copy `_dev` made of a strided or misaligned one)
        self.src_ptr, self.src_version, self.src_stride = src.data_ptr(), src._version, tuple(src.stride())
        _lib.check(lib.frmap_match_pack_gallery(gallery.data_ptr(), self.packed.data_ptr(), self.stat_w.data_ptr(), self.G, self.D,
                                                _stream()), "match_pack_gallery")
        self.ready = torch.cuda.Event()
        self.ready.record()          # consumers on other streams wait for the pack kernels (`wait_ready`)

    def update_rows(self, gallery: torch.Tensor, row_lo: int, row_hi: int) -> None:
        """``gallery`` (same storage, now G rows) had rows [row_lo, row_hi) appended or edited: re-pack those rows only."""
        src, gallery = gallery, _dev(gallery, "match_update.gallery", torch.float32, ("frmap_match_pack_gallery_rows", "gallery"))
        G = int(gallery.shape[0])
        if src.data_ptr() != self.src_ptr or tuple(src.stride()) != self.src_stride or gallery.shape[1] != self.D or G > self.capacity:
            raise ValueError("MatchPack.update_rows: not the gallery storage this pack was built from (or beyond its capacity)")
        torch.cuda.current_stream().wait_event(self.ready)
        _lib.check(_lib.load().frmap_match_pack_gallery_rows(gallery.data_ptr(), self.packed.data_ptr(), self.stat_w.data_ptr(),
                                                             int(row_lo), int(row_hi), G, self.D, _stream()), "match_pack_gallery_rows")
        self.G, self.src_version = G, src._version
        self.ready = torch.cuda.Event()
        self.ready.record()

    def wait_ready(self) -> None:
        torch.cuda.current_stream().wait_event(self.ready)

    def matches(self, gallery: torch.Tensor) -> bool:
        return (gallery.data_ptr() == self.src_ptr and gallery._version == self.src_version and tuple(gallery.stride()) == self.src_stride and
                tuple(gallery.shape) == (self.G, self.D) and gallery.device == self.packed.device)


MATCH_MFMA_MIN_G = 512   # galleries at least this large take the MFMA path when a MatchPack is supplied


def wants_pack(G: int, D: int) -> bool:
    """Whether a gallery of G rows of width D runs on the MFMA path (and so is worth a `MatchPack`)."""
    return G >= MATCH_MFMA_MIN_G and D % 32 == 0


def _usable_pack(prepared: Optional[MatchPack], gallery: torch.Tensor, D: int, what: str) -> Optional[MatchPack]:
    """``prepared`` if this call takes the packed entry point (`wants_pack`), else None; checked against ``gallery``, waited for."""
    if prepared is None or gallery is None or not wants_pack(int(gallery.shape[0]), D):
        return None
    if not prepared.matches(gallery):
        raise ValueError(f"{what}: `prepared` was built from a different (or since modified) gallery")
    if D != prepared.D:
        raise ValueError(f"{what}: embedding dim {D} != prepared gallery dim {prepared.D}")
    prepared.wait_ready()
    return prepared


@_on_operand_device
def match_prepare(gallery: torch.Tensor) -> MatchPack:
    return MatchPack(gallery)


def match_top1(emb: torch.Tensor, gallery: torch.Tensor, thresh: Optional[float] = None, packed: bool = False,
               prepared: Optional[MatchPack] = None):
    """First arg-min over gallery rows of ``||e - g + 1e-6||_2`` and that distance (int32[B], fp32[B]).
    With ``thresh`` a third tensor is returned: idx where dist <= thresh else -1 ("Unknown");
    with ``packed`` a fourth: int32[B, 2] = (id-or-unknown, bits of dist), the all-gather record.
    ``prepared`` (`match_prepare(gallery)`): run the gallery scan on the fp16 MFMA pipe (same contract)."""
    emb = _dev(emb, "match_top1.emb", torch.float32)
    if emb.dim() != 2:
        raise ValueError(f"match_top1: emb must be [B, D], got {list(emb.shape)}")
    B, D = emb.shape
    G = int(gallery.shape[0]) if gallery is not None else 0
    gptr = 0
    if G > 0:
        src, gallery = gallery, _dev(gallery, "match_top1.gallery", torch.float32)
        if gallery.dim() != 2 or gallery.shape[1] != D:
            raise ValueError(f"match_top1: gallery must be [G, {D}] (the embedding dim), got {list(gallery.shape)}")
        gptr = gallery.data_ptr()
    prepared = _usable_pack(prepared, src if G > 0 else gallery, D, "match_top1")
    idx = torch.empty((B,), dtype=torch.int32, device=emb.device)
    dist = torch.empty((B,), dtype=torch.float32, device=emb.device)
    ws = _match_workspace(B, G, emb.device)       # candidate records + per-probe statistics
    ids = torch.empty((B,), dtype=torch.int32, device=emb.device) if thresh is not None else None
    pk = _packed_buf(packed, B, emb.device)
    outs = (idx.data_ptr(), dist.data_ptr(), ids.data_ptr() if ids is not None else 0, pk.data_ptr() if pk is not None else 0,
            float(thresh) if thresh is not None else float("inf"), ws.data_ptr())
    if prepared is not None:
        split = torch.empty((B, 3 * D), dtype=torch.float16, device=emb.device)
        _lib.check(_lib.load().frmap_match_top1_packed(emb.data_ptr(), gptr, prepared.packed.data_ptr(), prepared.stat_w.data_ptr(),
                                                       *outs, split.data_ptr(), B, G, D, _stream()), "match_top1_packed")
    else:
        _lib.check(_lib.load().frmap_match_top1(emb.data_ptr(), gptr, *outs, B, G, D, _stream()), "match_top1")
    if pk is not None:
        return idx, dist, ids, pk
    return (idx, dist) if thresh is None else (idx, dist, ids)


MATCH_TOPK_MAX = 64


def match_topk(emb: torch.Tensor, gallery: Optional[torch.Tensor], k: int, labels: Optional[torch.Tensor] = None,
               prepared: Optional[MatchPack] = None):
    """Exact top-k gallery search: per probe the ``k`` rows nearest under ``||(e - g) + 1e-6||_2`` (the distance of
    `match_top1`: fp32 elements, float64 sum of squares), ordered by (distance, row).  With ``labels`` (int32 [G], values >= 0)
    the k nearest IDENTITIES instead: an identity's distance is the min over its rows, its row the first one attaining it.
    Returns ``(idx int32[B, k], dist fp32[B, k], label int32[B, k] | None)``; missing entries (k > G, NaN / inf rows) are
    ``(-1, +inf, -1)``.  k = 1 without labels is `match_top1` (bit-identical).  Path choice as `match_top1`: ``prepared`` galleries of
    >= `MATCH_MFMA_MIN_G` rows with D % 32 == 0 run on the fp16 MFMA GEMM + exact re-score, everything else on an exact scan."""
    emb = _dev(emb, "match_topk.emb", torch.float32)
    if emb.dim() != 2:
        raise ValueError("match_topk: emb must be [B, D]")
    B, D = emb.shape
    k = int(k)
    if not 1 <= k <= MATCH_TOPK_MAX:
        raise ValueError(f"match_topk: k={k} out of range (1 <= k <= {MATCH_TOPK_MAX})")
    G = int(gallery.shape[0]) if gallery is not None else 0
    gptr = lptr = 0
    if G > 0:
        src, gallery = gallery, _dev(gallery, "match_topk.gallery", torch.float32)
        if gallery.dim() != 2 or gallery.shape[1] != D:
            raise ValueError(f"match_topk: gallery must be [G, {D}] (the embedding dim), got {list(gallery.shape)}")
        gptr = gallery.data_ptr()
    if labels is not None:
        labels = _dev(labels, "match_topk.labels", torch.int32, ("frmap_match_topk", "labels"))
        if tuple(labels.shape) != (G,):
            raise ValueError(f"match_topk: labels must be int32 [{G}], got {tuple(labels.shape)}")
        lptr = labels.data_ptr() if G > 0 else 0
    idx = torch.empty((B, k), dtype=torch.int32, device=emb.device)
    dist = torch.empty((B, k), dtype=torch.float32, device=emb.device)
    lab = torch.empty((B, k), dtype=torch.int32, device=emb.device) if labels is not None else None
    lib = _lib.load()
    ws = torch.empty((lib.frmap_match_topk_workspace_bytes(B, G, D, k),), dtype=torch.uint8, device=emb.device)
    if labels is not None and G == 0:
        lptr = ws.data_ptr()          # (identity mode on an empty gallery: a non-null labels pointer keeps the mode)
    lbp = lab.data_ptr() if lab is not None else 0
    prepared = _usable_pack(prepared, src if G > 0 else gallery, D, "match_topk")
    if prepared is not None:
        _lib.check(lib.frmap_match_topk_packed(emb.data_ptr(), gptr, prepared.packed.data_ptr(), prepared.stat_w.data_ptr(), lptr,
                                               idx.data_ptr(), dist.data_ptr(), lbp, ws.data_ptr(), B, G, D, k, _stream()),
                   "match_topk_packed")
    else:
        _lib.check(lib.frmap_match_topk(emb.data_ptr(), gptr, lptr, idx.data_ptr(), dist.data_ptr(), lbp, ws.data_ptr(),
                                        B, G, D, k, _stream()), "match_topk")
    return idx, dist, lab


VERIFY_MAX_THRESHOLDS = 2048


def verify_thresholds(thresholds, device) -> torch.Tensor:
    """fp32 [T] device tensor of ``thresholds`` after checking the contract of `verify_counts` on the host (finite, >= 0, strictly
    ascending as fp32, 1 <= T <= `VERIFY_MAX_THRESHOLDS`).  A device tensor is checked through one host copy, except while a graph
    is being captured: there the library's own device-side check stands (a violating call writes -1 to every count)."""
    if isinstance(thresholds, torch.Tensor) and thresholds.is_cuda:
        t = _dev(thresholds, "verify_counts.thresholds", torch.float32).reshape(-1)
        host = None if torch.cuda.is_current_stream_capturing() else t.cpu().numpy()
    else:
        host = np.asarray(thresholds.cpu() if isinstance(thresholds, torch.Tensor) else thresholds, dtype=np.float32).reshape(-1)
        t = None
    if host is not None:
        T = host.shape[0]
        if not 1 <= T <= VERIFY_MAX_THRESHOLDS:
            raise ValueError(f"verify_counts: {T} thresholds (1 <= T <= {VERIFY_MAX_THRESHOLDS})")
        if not np.isfinite(host).all() or (host < 0).any():
            raise ValueError("verify_counts: thresholds must be finite and >= 0")
        if T > 1 and not (np.diff(host) > 0).all():
            raise ValueError("verify_counts: thresholds must be strictly ascending")
        if t is None:
            t = torch.from_numpy(np.ascontiguousarray(host)).to(device)
    return t


def _pair_operands(op: str, a, labels_a, b, labels_b, a_row0, absent: dict):
    """The ``a / b / labels / a_row0`` modes of `verify_counts` and `match_radius`: ``(a, la, b, lb, row0)`` as the C entry points
    take them (int32 labels or None; row0 = -1 in cross mode; self mode over ``a``: b = a, lb = la, row0 = 0).  ``absent[what]``:
    the ValueError text for a missing ``what`` (labels_a / labels_b), or None where it may be missing."""
    a = _dev(a, f"{op}.a", torch.float32)
    if a.dim() != 2:
        raise ValueError(f"{op}: a must be [P, D]")
    P, D = int(a.shape[0]), int(a.shape[1])

    def labels(t, n, what):
        if t is None and what in absent:
            if absent[what] is not None:
                raise ValueError(absent[what])
            return None
        t = _dev(t, f"{op}.{what}")
        if t.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{op}: {what} must be int32 or int64, got {t.dtype}")
        if tuple(t.shape) != (n,):
            raise ValueError(f"{op}: {what} must hold {n} labels as [{n}], got {list(t.shape)}")
        return t.to(torch.int32)

    la = labels(labels_a, P, "labels_a")
    if b is None:
        if labels_b is not None or a_row0 not in (None, 0):
            raise ValueError(f"{op}: self mode over `a` (b=None) takes no labels_b / a_row0")
        return a, la, a, la, 0
    b = _dev(b, f"{op}.b", torch.float32)
    if b.dim() != 2 or int(b.shape[1]) != D:
        raise ValueError(f"{op}: b must be [Q, {D}]")
    lb = labels(labels_b, int(b.shape[0]), "labels_b")
    row0 = -1 if a_row0 is None else int(a_row0)
    if a_row0 is not None and not (row0 >= 0 and row0 + P <= int(b.shape[0])):
        raise ValueError(f"{op}: a_row0={row0} with {P} rows is not a block of b's {int(b.shape[0])} rows")
    return a, la, b, lb, row0


def verify_counts(a: torch.Tensor, labels_a: torch.Tensor, thresholds, b: Optional[torch.Tensor] = None,
                  labels_b: Optional[torch.Tensor] = None, *, a_row0: Optional[int] = None, prepared: Optional[MatchPack] = None,
                  return_rescored: bool = False):
    """Exact verification counts: int64 [2, T] on the device, row 0 = genuine pairs (equal labels), row 1 = impostor pairs whose
    distance ``(float) sqrt(d2)`` (the distance `match_topk` reports) is ``<= thresholds[k]``; NaN / inf distances are never accepted.
    ``b=None``: self mode over ``a`` (every unordered pair once).  ``b`` with ``a_row0``: self mode, ``a`` = rows
    [a_row0, a_row0 + len(a)) of ``b`` (pairs with a_row0 + i < j: shards over a_row0 sum to the whole).  ``b`` alone: cross mode,
    every (i, j).  ``thresholds``: finite, >= 0, strictly ascending, at most `VERIFY_MAX_THRESHOLDS`.  Path choice as `match_topk`:
    a ``prepared`` B (`match_prepare(b)`) of >= `MATCH_MFMA_MIN_G` rows with D % 32 == 0 runs on the fp16 MFMA GEMM whose epilogue
    bins the certain pairs and re-scores the rest exactly; everything else on an exact scan.  Same counts either way.
    ``return_rescored``: also return int64 [1] = the pairs the GEMM path re-scored.
    Outside graph capture the thresholds are checked on the host (`verify_thresholds`): host values are uploaded with a blocking
    copy and device values read back, so each call synchronises the stream once.  A caller that repeats calls on fixed device
    thresholds and wants them asynchronous calls the C entry points (`frmap_verify_counts[_packed]`) after checking them once."""
    src = a if b is None else b
    a, la, b, lb, row0 = _pair_operands("verify_counts", a, labels_a, b, labels_b, a_row0,
                                        {"labels_b": "verify_counts: labels_b is required with b"})
    (P, D), Q = a.shape, int(b.shape[0])
    thr = verify_thresholds(thresholds, a.device)
    T = int(thr.shape[0])
    lib = _lib.load()
    out = torch.empty((2, T), dtype=torch.int64, device=a.device)
    resc = torch.empty((1,), dtype=torch.int64, device=a.device) if return_rescored else None
    ws = torch.empty((lib.frmap_verify_workspace_bytes(P, Q, D, T),), dtype=torch.uint8, device=a.device)
    aptr, laptr = (a.data_ptr(), la.data_ptr()) if P else (0, 0)
    bptr, lbptr = (b.data_ptr(), lb.data_ptr()) if Q else (0, 0)
    rptr = resc.data_ptr() if resc is not None else 0
    prepared = _usable_pack(prepared, src, D, "verify_counts")
    if prepared is not None:
        _lib.check(lib.frmap_verify_counts_packed(aptr, laptr, P, bptr, prepared.packed.data_ptr(), prepared.stat_w.data_ptr(), lbptr,
                                                  Q, D, row0, thr.data_ptr(), T, out.data_ptr(), rptr, ws.data_ptr(), _stream()),
                   "verify_counts_packed")
    else:
        _lib.check(lib.frmap_verify_counts(aptr, laptr, P, bptr, lbptr, Q, D, row0, thr.data_ptr(), T, out.data_ptr(), rptr,
                                           ws.data_ptr(), _stream()), "verify_counts")
    return (out, resc) if return_rescored else out


_RADIUS_WHICH = {"all": 0, "same": 1, "different": 2}


def match_radius(a: torch.Tensor, thresh: float, b: Optional[torch.Tensor] = None, *, labels_a: Optional[torch.Tensor] = None,
                 labels_b: Optional[torch.Tensor] = None, which: str = "all", a_row0: Optional[int] = None,
                 prepared: Optional[MatchPack] = None, capacity: Optional[int] = None, return_rescored: bool = False):
    """Exact threshold search: every counted pair (i, j) whose distance ``(float) sqrt(d2)`` (the one `match_topk` reports and
    `verify_counts` thresholds) is ``<= thresh``; NaN / inf distances are never listed.  Modes as `verify_counts`: ``b=None`` is self
    mode over ``a`` (every unordered pair once, i < j); ``b`` with ``a_row0`` is self mode with ``a`` = rows [a_row0, a_row0 + len(a))
    of ``b`` (pairs with a_row0 + i < j; i indexes ``a``, j indexes ``b``; shards over a_row0 partition the whole); ``b`` alone is
    cross mode.  ``which``: "all", or "same" / "different" = pairs of equal / different labels only (then labels are required).
    ``thresh``: a finite host float >= 0.

    ``capacity=None``: a count-only call, one read of the total (the call's one synchronisation), then the fill: returns
    ``(pairs int32 [n, 2], dists fp32 [n], counts int32 [P])`` sorted by (i, j); ``counts[i]`` = accepted pairs of row i.
    ``capacity=<int>``: ONE asynchronous call (graph-capturable) into fresh buffers of that many slots: returns
    ``(pairs int32 [capacity, 2], dists fp32 [capacity], counts int32 [P], total int64 [1])``, the first ``min(total, capacity)``
    slots filled in no particular order; ``counts`` and ``total`` are exact whatever the capacity (0: count only).
    ``return_rescored``: also int64 [1] = the pairs the GEMM path scored exactly, appended to either result.
    Path choice as `verify_counts`: a ``prepared`` B of >= `MATCH_MFMA_MIN_G` rows with D % 32 == 0 runs on the fp16 MFMA GEMM, whose
    epilogue drops the pairs certainly beyond the threshold and re-scores the rest; everything else on an exact scan.  Same answer."""
    if which not in _RADIUS_WHICH:
        raise ValueError(f"match_radius: which must be 'all', 'same' or 'different', got {which!r}")
    filt = _RADIUS_WHICH[which]
    thresh = float(thresh)
    if not 0.0 <= thresh <= float(np.finfo(np.float32).max):          # (NaN fails both; the library takes an fp32)
        raise ValueError(f"match_radius: thresh must be finite and >= 0, got {thresh}")
    src = a if b is None else b
    a, la, b, lb, row0 = _pair_operands("match_radius", a, labels_a, b, labels_b, a_row0, {
        what: f"match_radius: which={which!r} needs {what}" if filt else None for what in ("labels_a", "labels_b")})
    (P, D), Q = a.shape, int(b.shape[0])
    if capacity is not None and int(capacity) < 0:
        raise ValueError(f"match_radius: capacity={capacity} must be >= 0")
    lib = _lib.load()
    dev = a.device
    counts = torch.empty((P,), dtype=torch.int32, device=dev)
    total = torch.empty((1,), dtype=torch.int64, device=dev)
    resc = torch.empty((1,), dtype=torch.int64, device=dev) if return_rescored else None
    ws = torch.empty((lib.frmap_match_radius_workspace_bytes(P, Q, D),), dtype=torch.uint8, device=dev)
    aptr, laptr = (a.data_ptr(), la.data_ptr() if la is not None else 0) if P else (0, 0)
    bptr, lbptr = (b.data_ptr(), lb.data_ptr() if lb is not None else 0) if Q else (0, 0)
    rptr = resc.data_ptr() if resc is not None else 0
    prepared = _usable_pack(prepared, src, D, "match_radius")

    def call(cap):
        pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)
        dists = torch.empty((cap,), dtype=torch.float32, device=dev)
        outs = (counts.data_ptr() if P else 0, total.data_ptr(), pairs.data_ptr() if cap else 0, dists.data_ptr() if cap else 0, cap,
                rptr, ws.data_ptr(), _stream())
        if prepared is not None:
            _lib.check(lib.frmap_match_radius_packed(aptr, laptr, P, bptr, prepared.packed.data_ptr(), prepared.stat_w.data_ptr(), lbptr,
                                                     Q, D, row0, thresh, filt, *outs), "match_radius_packed")
        else:
            _lib.check(lib.frmap_match_radius(aptr, laptr, P, bptr, lbptr, Q, D, row0, thresh, filt, *outs), "match_radius")
        return pairs, dists

    tail = (resc,) if return_rescored else ()
    if capacity is not None:
        pairs, dists = call(int(capacity))
        return (pairs, dists, counts, total) + tail
    call(0)
    n = int(total.item())
    pairs, dists = call(n)
    if n > 1:                     # order by (i, j): one sort of the packed 64-bit key
        order = torch.argsort((pairs[:, 0].to(torch.int64) << 32) | pairs[:, 1].to(torch.int64))
        pairs, dists = pairs[order], dists[order]
    return (pairs, dists, counts) + tail


def gap_linear_norm(fmap: torch.Tensor, wt: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
                    eps: float = 1e-12, want_pre: bool = False, relu: bool = False):
    """ArcFaceNet head in one launch (`face_models.py:573-590`): global average pool of the NHWC trunk map [B,H,W,K] ->
    Linear (``wt`` = weight transposed, fp32 [K][N]) -> folded BatchNorm1d -> L2-normalise.  Returns ``(emb, pre | None)``."""
    keep = []
    fmap = _dev(fmap, "gap_linear_norm.map")
    B, H, W, K = fmap.shape
    wt = _dev(wt, "gap_linear_norm.wt", torch.float32, ("frmap_gap_linear_norm", "wt"))
    if wt.dim() != 2 or wt.shape[0] != K or not wt.is_contiguous():
        raise ValueError(f"gap_linear_norm: wt must be a contiguous [{K}][N] matrix")
    N = int(wt.shape[1])
    if scale is not None:
        _sized(scale, "gap_linear_norm", "scale", (N,), torch.float32)
    if shift is not None:
        _sized(shift, "gap_linear_norm", "shift", (N,), torch.float32)
    emb =torch.empty((B, N), dtype=torch.float32, device=fmap.device)
    pre = torch.empty((B, N), dtype=torch.float32, device=fmap.device) if want_pre else None
    _lib.check(_lib.load().frmap_gap_linear_norm(fmap.data_ptr(), wt.data_ptr(),
                                                 _ptr(keep, scale, "scale", torch.float32, ("frmap_gap_linear_norm", "scale")) if scale is not None else 0,
                                                 _ptr(keep, shift, "shift", torch.float32, ("frmap_gap_linear_norm", "shift")) if shift is not None else 0,
                                                 pre.data_ptr() if pre is not None else 0, emb.data_ptr(), float(eps),
                                                 B, H * W, K, N, int(bool(relu)), dt_code(fmap.dtype), _stream()), "gap_linear_norm")
    return emb, pre


def gap_norm_match(fmap: torch.Tensor, gallery: torch.Tensor, thresh: Optional[float] = None, normalize: bool = False,
                   eps: float = 1e-12, want_emb: bool = False, packed: bool = False):
    """Global-average-pool an NHWC trunk map [B,H,W,C], optionally L2-normalise, and match against a small gallery
    (<= 64 rows) in one launch.  Returns (idx, dist, ids | None, packed | None, emb | None)."""
    fmap = _dev(fmap, "gap_norm_match.map")
    B, H, W, Cc = fmap.shape
    G = int(gallery.shape[0]) if gallery is not None else 0
    gptr = 0
    if G > 0:
        gallery = _dev(gallery, "gap_norm_match.gallery", torch.float32)
        if gallery.dim() != 2 or gallery.shape[1] != Cc:
            raise ValueError(f"gap_norm_match: gallery must be [G, {Cc}] (the map's channels), got {list(gallery.shape)}")
        gptr = gallery.data_ptr()
    idx = torch.empty((B,), dtype=torch.int32, device=fmap.device)
    dist = torch.empty((B,), dtype=torch.float32, device=fmap.device)
    ids = torch.empty((B,), dtype=torch.int32, device=fmap.device) if thresh is not None else None
    pk = _packed_buf(packed, B, fmap.device)
    emb = torch.empty((B, Cc), dtype=torch.float32, device=fmap.device) if want_emb else None
    _lib.check(_lib.load().frmap_gap_norm_match(fmap.data_ptr(), gptr, emb.data_ptr() if emb is not None else 0, idx.data_ptr(),
                                                dist.data_ptr(), ids.data_ptr() if ids is not None else 0,
                                                pk.data_ptr() if pk is not None else 0,
                                                float(thresh) if thresh is not None else float("inf"), int(bool(normalize)),
                                                float(eps), B, H * W, Cc, G, dt_code(fmap.dtype), _stream()), "gap_norm_match")
    return idx, dist, ids, pk, emb


def cosine_logits(x: torch.Tensor, w: torch.Tensor, s: float = 1.0, want_logits: bool = True,
                  want_argmax: bool = True):
    x = _dev(x, "cosine_logits.x", torch.float32)
    w = _dev(w, "cosine_logits.w", torch.float32)
    if x.dim() != 2 or w.dim() != 2 or w.shape[1] != x.shape[1]:
        raise ValueError(f"cosine_logits: x [B, D] and w [C, D] expected, got {list(x.shape)} and {list(w.shape)}")
    B, D = x.shape
    Cc = w.shape[0]
    logits = torch.empty((B, Cc), dtype=torch.float32, device=x.device) if want_logits else None
    arg = torch.empty((B,), dtype=torch.int32, device=x.device) if want_argmax else None
    ws = _workspace(B, Cc, x.device)
    _lib.check(_lib.load().frmap_cosine_logits(x.data_ptr(), w.data_ptr(), logits.data_ptr() if want_logits else 0,
                                               arg.data_ptr() if want_argmax else 0, ws.data_ptr(), B, Cc, D,
                                               float(s), _stream()), "cosine_logits")
    return logits, arg


def arcmargin_eval(x: torch.Tensor, w: torch.Tensor, label: torch.Tensor, s: float, m: float,
                   easy_margin: bool = False, want_minmax: bool = False):
    x = _dev(x, "arcmargin_eval.x", torch.float32)
    w = _dev(w, "arcmargin_eval.w", torch.float32)
    label = _dev(label, "arcmargin_eval.label", torch.int64, ("frmap_arcmargin_eval", "label"))
    if x.dim() != 2 or w.dim() != 2 or w.shape[1] != x.shape[1]:
        raise ValueError(f"arcmargin_eval: x [B, D] and w [C, D] expected, got {list(x.shape)} and {list(w.shape)}")
    B, D = x.shape
    Cc = w.shape[0]
    if tuple(label.shape) != (B,):
        raise ValueError(f"arcmargin_eval: label must be [{B}], one per row of x, got {list(label.shape)}")
    out = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    mm = torch.empty((2,), dtype=torch.float32, device=x.device) if want_minmax else None
    ws = _workspace(B, Cc, x.device)
    _lib.check(_lib.load().frmap_arcmargin_eval(x.data_ptr(), w.data_ptr(), label.data_ptr(), out.data_ptr(),
                                                mm.data_ptr() if want_minmax else 0, ws.data_ptr(), B, Cc, D,
                                                float(s), float(m), int(easy_margin), _stream()), "arcmargin_eval")
    return out, mm


# ------------------------------------------------------------------------------------------------
# the frame loop's IoU tracker over many streams (`frmap_track_*`, csrc/track.hip; the rule is `frames.track_boxes`)
# ------------------------------------------------------------------------------------------------
TRACK_MAX_BOXES = 256


def track_state_bytes(n_streams: int, max_boxes: int) -> int:
    """Bytes of a tracker state buffer; ``ValueError`` outside the supported sizes (``1 <= max_boxes <= 256``)."""
    if n_streams < 0 or not 1 <= max_boxes <= TRACK_MAX_BOXES:
        raise ValueError(f"track_state: n_streams = {n_streams}, max_boxes = {max_boxes} (supported: n_streams >= 0, 1 <= max_boxes <= "
                         f"{TRACK_MAX_BOXES})")
    return int(_lib.load().frmap_track_state_bytes(int(n_streams), int(max_boxes)))


def track_state(n_streams: int, max_boxes: int, device="cuda") -> torch.Tensor:
    """A fresh state for `track_step`: a zeroed uint8 buffer on ``device`` (``"cpu"``: for `track_step_host`, as a tensor)."""
    return torch.zeros(max(track_state_bytes(n_streams, max_boxes), 16), dtype=torch.uint8, device=device)


def track_state_host(n_streams: int, max_boxes: int) -> np.ndarray:
    """A fresh state for `track_step_host`: a zeroed, 16-byte aligned uint8 array."""
    raw = np.zeros(max(track_state_bytes(n_streams, max_boxes), 16) + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + raw.size - 16]


def _track_views(a: np.ndarray, S: int, M: int):
    """The three arrays of a host state buffer as views: ``(meta int32 [S, 2] = (P, next_id), boxes float32 [S, M, 4], ids int32
    [S, M])``.  The one place where Python knows the layout (csrc/track_rule.h): the ids end the buffer, the boxes precede them,
    and the library says where the buffer ends."""
    total = track_state_bytes(S, M)
    i_off = total - 4 * S * M
    b_off = i_off - 16 * S * M
    if a.size < total:
        raise ValueError(f"track state holds {a.size} bytes, {S} streams of {M} boxes need {total}")
    return (a[:8 * S].view(np.int32).reshape(S, 2), a[b_off:i_off].view(np.float32).reshape(S, M, 4),
            a[i_off:total].view(np.int32).reshape(S, M))


def track_state_unpack(buf, n_streams: int, max_boxes: int):
    """The streams of a state buffer (device tensor or host array; a device buffer is copied to the host, which synchronises) as a
    list of `frames.TrackState`: what `frames.track_boxes` would hold for each stream."""
    from . import frames as _frames
    a = buf.detach().cpu().numpy() if isinstance(buf, torch.Tensor) else np.asarray(buf)
    meta, boxes, ids = _track_views(np.ascontiguousarray(a).view(np.uint8).reshape(-1), int(n_streams), int(max_boxes))
    return [_frames.TrackState(boxes[s, :meta[s, 0]].copy(), ids[s, :meta[s, 0]].astype(np.int64), int(meta[s, 1]))
            for s in range(int(n_streams))]


def track_state_pack(states, max_boxes: int) -> np.ndarray:
    """The inverse of `track_state_unpack`: a host state buffer (as `track_state_host`) holding the given `frames.TrackState` of
    every stream (``None``: a fresh one) - to carry tracks of `frames.track_boxes` on to `track_step`, or to restore saved ones."""
    S, M = len(states), int(max_boxes)
    a = track_state_host(S, M)
    meta, boxes, ids = _track_views(a, S, M)
    for s, st in enumerate(states):
        if st is None:
            continue
        P = len(st.ids)
        if P > M:
            raise ValueError(f"track_state_pack: stream {s} holds {P} boxes, max_boxes is {M}")
        meta[s] = (P, st.next_id)
        boxes[s, :P] = np.asarray(st.boxes, np.float32).reshape(P, 4)
        ids[s, :P] = st.ids
    return a


def track_step(state: torch.Tensor, boxes: torch.Tensor, probs: Optional[torch.Tensor], counts: torch.Tensor,
               frame_hw: torch.Tensor, det_thresh: float = 0.9, iou_thresh: float = 0.3) -> Tuple[torch.Tensor, torch.Tensor]:
    """One tracker step of S streams in one launch on the current stream (`frmap_track_step`): ``(ids int32 [S, max_boxes], rois
    int32 [S, max_boxes, 4])``.  Device tensors: ``state`` from `track_state` (updated in place), ``boxes`` float32 ``[S, max_boxes,
    4]``, ``probs`` float32 ``[S, max_boxes]`` or ``None`` (every box confident), ``counts`` int32 ``[S]``, ``frame_hw`` int32
    ``[S, 2]`` = (H, W).  ``ids`` is the `frames.track_boxes` id of each box, -1 for skipped boxes and beyond ``counts[s]``; ``rois``
    the `frames.clip_boxes` crop of every box with an id, 0 elsewhere.  ``counts`` is device data: the kernel clamps it to
    ``[0, max_boxes]``; a caller that has it on the host checks it there (`matching.StreamTracker` does)."""
    boxes = _dev(boxes, "track_step.boxes", torch.float32)
    probs = None if probs is None else _dev(probs, "track_step.probs", torch.float32, ("frmap_track_step", "probs"))
    counts = _dev(counts, "track_step.counts", torch.int32, ("frmap_track_step", "counts"))
    frame_hw = _dev(frame_hw, "track_step.frame_hw", torch.int32, ("frmap_track_step", "frame_hw"))
    state = _dev(state, "track_step.state", torch.uint8, ("frmap_track_step", "state"), owned=True)
    if boxes.dim() != 3 or boxes.shape[2] != 4:
        raise ValueError(f"track_step: boxes must be float32 [S, max_boxes, 4], got {tuple(boxes.shape)}")
    S, M = int(boxes.shape[0]), int(boxes.shape[1])
    if (probs is not None and tuple(probs.shape) != (S, M)) or tuple(counts.shape) != (S,) or tuple(frame_hw.shape) != (S, 2):
        raise ValueError("track_step: probs [S, max_boxes], counts [S] and frame_hw [S, 2] must match boxes")
    if state.dim() != 1:
        raise ValueError(f"track_step: state must be a flat uint8 buffer (`track_state`), got {list(state.shape)}")
    if state.numel() < track_state_bytes(S, M):
        raise ValueError(f"track_step: state holds {state.numel()} bytes, {S} streams of {M} boxes need {track_state_bytes(S, M)}")
    ids = torch.empty((S, M), dtype=torch.int32, device=boxes.device)
    rois = torch.empty((S, M, 4), dtype=torch.int32, device=boxes.device)
    _lib.check(_lib.load().frmap_track_step(state.data_ptr(), boxes.data_ptr(), 0 if probs is None else probs.data_ptr(),
                                            counts.data_ptr(), frame_hw.data_ptr(), S, M, float(det_thresh), float(iou_thresh),
                                            ids.data_ptr(), rois.data_ptr(), _stream()), "track_step")
    return ids, rois


def track_step_host(state: np.ndarray, boxes, probs, counts, frame_hw, det_thresh: float = 0.9,
                    iou_thresh: float = 0.3) -> Tuple[np.ndarray, np.ndarray]:
    """`track_step` on the CPU over numpy arrays (`frmap_track_step_host`: the kernel's rule compiled for the host; no GPU).
    ``state``: a writable uint8 array from `track_state_host`, updated in place.  A ``counts[s]`` outside ``[0, max_boxes]`` or an
    unsupported ``max_boxes`` raises ``ValueError`` with the state untouched."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float32)
    probs = None if probs is None else np.ascontiguousarray(probs, dtype=np.float32)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    frame_hw = np.ascontiguousarray(frame_hw, dtype=np.int32)
    if len(boxes.shape) != 3 or boxes.shape[2] != 4:
        raise ValueError(f"track_step_host: boxes must be float32 [S, max_boxes, 4], got {boxes.shape}")
    S, M = boxes.shape[:2]
    if (probs is not None and probs.shape != (S, M)) or counts.shape != (S,) or frame_hw.shape != (S, 2):
        raise ValueError("track_step_host: probs [S, max_boxes], counts [S] and frame_hw [S, 2] must match boxes")
    if not (isinstance(state, np.ndarray) and state.dtype == np.uint8 and state.flags.c_contiguous and state.flags.writeable):
        raise ValueError("track_step_host: state must be a writable contiguous uint8 array (track_state_host)")
    if 1 <= M <= TRACK_MAX_BOXES and state.size < track_state_bytes(S, M):    # (an unsupported max_boxes is the library's to refuse)
        raise ValueError(f"track_step_host: state holds {state.size} bytes, {S} streams of {M} boxes need {track_state_bytes(S, M)}")
    ids = np.empty((S, M), np.int32)
    rois = np.empty((S, M, 4), np.int32)
    _lib.check(_lib.load().frmap_track_step_host(state.ctypes.data, boxes.ctypes.data, None if probs is None else probs.ctypes.data,
                                                 counts.ctypes.data, frame_hw.ctypes.data, S, M, float(det_thresh), float(iou_thresh),
                                                 ids.ctypes.data, rois.ctypes.data), "track_step_host")
    return ids, rois


# ------------------------------------------------------------------------------------------------
# track templates: a track's embeddings pooled on the device (`frmap_track_fuse*`, csrc/track_fuse.hip; the rule is
# `frames.fuse_tracks`)
# ------------------------------------------------------------------------------------------------
TRACK_FUSE_MAX_DIM = 4096


def track_fuse_state_bytes(n_streams: int, max_boxes: int, dim: int) -> int:
    """Bytes of a template state buffer; ``ValueError`` outside the supported sizes (``1 <= max_boxes <= 256``, ``1 <= dim <= 4096``)."""
    if n_streams < 0 or not 1 <= max_boxes <= TRACK_MAX_BOXES or not 1 <= dim <= TRACK_FUSE_MAX_DIM:
        raise ValueError(f"track_fuse_state: n_streams = {n_streams}, max_boxes = {max_boxes}, dim = {dim} (supported: n_streams >= 0, "
                         f"1 <= max_boxes <= {TRACK_MAX_BOXES}, 1 <= dim <= {TRACK_FUSE_MAX_DIM})")
    return int(_lib.load().frmap_track_fuse_state_bytes(int(n_streams), int(max_boxes), int(dim)))


def track_fuse_state(n_streams: int, max_boxes: int, dim: int, device="cuda") -> torch.Tensor:
    """A fresh state for `track_fuse`: a zeroed uint8 buffer on ``device``."""
    return torch.zeros(max(track_fuse_state_bytes(n_streams, max_boxes, dim), 16), dtype=torch.uint8, device=device)


def track_fuse_state_host(n_streams: int, max_boxes: int, dim: int) -> np.ndarray:
    """A fresh state for `track_fuse_host`: a zeroed, 16-byte aligned uint8 array."""
    raw = np.zeros(max(track_fuse_state_bytes(n_streams, max_boxes, dim), 16) + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + raw.size - 16]


def track_fuse_state_unpack(buf, n_streams: int, max_boxes: int, dim: int):
    """The streams of a template state buffer (device tensor or host array; a device buffer is copied to the host, which
    synchronises) as a list of `frames.TemplateState`: what `frames.fuse_tracks` would hold for each stream.  The one place where
    Python knows the layout (csrc/track_fuse_rule.h): the sums end the buffer, the weights and the ids precede them, two banks of
    ``max_boxes`` slots per stream, and a stream's meta record ``(P, bank)`` says which bank is current."""
    from . import frames as _frames
    S, M, D = int(n_streams), int(max_boxes), int(dim)
    a = buf.detach().cpu().numpy() if isinstance(buf, torch.Tensor) else np.asarray(buf)
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    total, pitch = track_fuse_state_bytes(S, M, D), (D + 3) & ~3
    if a.size < total:
        raise ValueError(f"template state holds {a.size} bytes, {S} streams of {M} boxes of {D} values need {total}")
    s_off = total - 8 * S * M * pitch
    w_off = s_off - 8 * S * M
    i_off = w_off - 8 * S * M
    meta = a[:8 * S].view(np.int32).reshape(S, 2)
    ids = a[i_off:w_off].view(np.int32).reshape(S, 2, M)
    w = a[w_off:s_off].view(np.float32).reshape(S, 2, M)
    sums = a[s_off:total].view(np.float32).reshape(S, 2, M, pitch)
    out = []
    for s in range(S):
        P, b = min(max(int(meta[s, 0]), 0), M), int(meta[s, 1]) & 1
        out.append(_frames.TemplateState(ids[s, b, :P].astype(np.int64), w[s, b, :P].copy(), sums[s, b, :P, :D].copy()))
    return out


def _fuse_check_rows(what: str, rows: np.ndarray, counts: np.ndarray, S: int) -> None:
    """The host's check of ``rows`` against the step's host ``counts``: what `frmap_track_fuse_host` refuses, refused before a launch."""
    if rows.shape[0] == 0:
        return
    st, det = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64)
    if st.min() < 0 or st.max() >= S:
        raise ValueError(f"{what}: a row names a stream outside [0, {S})")
    if det.min() < 0 or (det >= counts.astype(np.int64)[st]).any():
        raise ValueError(f"{what}: a row names a detection outside [0, counts[stream])")
    if len(np.unique(st * (int(det.max()) + 1) + det)) != len(det):
        raise ValueError(f"{what}: two rows name the same detection")


def track_fuse(state: torch.Tensor, ids: torch.Tensor, counts: torch.Tensor, emb: torch.Tensor, rows, decay: float = 1.0,
               host_counts=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One template step of S streams in one launch on the current stream (`frmap_track_fuse`): ``(fused float32 [N, D], frames
    float32 [N])``.  Device tensors: ``state`` from `track_fuse_state` (updated in place), ``ids`` int32 ``[S, max_boxes]`` and
    ``counts`` int32 ``[S]`` of this step's `track_step`, ``emb`` float32 ``[N, D]``.  ``rows``: int32 ``[N, 2]`` = (stream,
    detection index) of every row of ``emb``.  Given as a HOST array together with ``host_counts`` (the step's counts on the host)
    it is checked here - a detection index ``>= counts[stream]``, a stream outside ``[0, S)``, two rows of one detection:
    ``ValueError`` before anything is launched - and uploaded; a device tensor is data the host never saw: the kernel clamps
    ``counts``, passes a row that names no detection through and touches no other stream's slots whatever ``rows`` holds.
    ``fused[r]`` is the template of row r's track after this step and ``frames[r]`` its weight; rows that are passed through
    (`frames.fuse_tracks`) come back as they came with ``frames[r] = 0``."""
    state = _dev(state, "track_fuse.state", torch.uint8, ("frmap_track_fuse", "state"), owned=True)
    ids = _dev(ids, "track_fuse.ids", torch.int32, ("frmap_track_fuse", "ids"))
    counts = _dev(counts, "track_fuse.counts", torch.int32, ("frmap_track_fuse", "counts"))
    emb = _dev(emb, "track_fuse.emb", torch.float32)
    if ids.dim() != 2 or emb.dim() != 2 or tuple(counts.shape) != (ids.shape[0],):
        raise ValueError(f"track_fuse: ids must be int32 [S, max_boxes], counts [S] and emb float32 [N, D]; got {tuple(ids.shape)}, "
                         f"{tuple(counts.shape)} and {tuple(emb.shape)}")
    S, M = int(ids.shape[0]), int(ids.shape[1])
    N, D = int(emb.shape[0]), int(emb.shape[1])
    if not (0.0 < float(np.float32(decay)) <= 1.0):
        raise ValueError(f"track_fuse: decay = {decay} is outside (0, 1]")
    if state.dim() != 1:
        raise ValueError(f"track_fuse: state must be a flat uint8 buffer (`track_fuse_state`), got {list(state.shape)}")
    if state.numel() < track_fuse_state_bytes(S, M, D):
        raise ValueError(f"track_fuse: state holds {state.numel()} bytes, {S} streams of {M} boxes of {D} values need "
                         f"{track_fuse_state_bytes(S, M, D)}")
    if not isinstance(rows, torch.Tensor):
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 2)
        if rows.shape[0] != N:
            raise ValueError(f"track_fuse: {rows.shape[0]} rows for {N} embeddings")
        if host_counts is None:
            raise ValueError("track_fuse: host rows are checked against host_counts, the step's counts on the host")
        host_counts = np.asarray(host_counts).reshape(-1)
        if host_counts.shape != (S,) or (host_counts < 0).any() or (host_counts > M).any():
            raise ValueError("track_fuse: host_counts must be [S] values in [0, max_boxes]")
        _fuse_check_rows("track_fuse", rows, host_counts, S)
        rows = torch.from_numpy(rows).to(emb.device, non_blocking=True)
    rows = _dev(rows, "track_fuse.rows", torch.int32, ("frmap_track_fuse", "rows"))
    if tuple(rows.shape) != (N, 2):
        raise ValueError(f"track_fuse: rows must be int32 [{N}, 2], got {tuple(rows.shape)}")
    if N > S * M:
        raise ValueError(f"track_fuse: {N} rows for {S} streams of {M} boxes")
    fused = torch.empty((N, D), dtype=torch.float32, device=emb.device)
    nframes = torch.empty((N,), dtype=torch.float32, device=emb.device)
    _lib.check(_lib.load().frmap_track_fuse(state.data_ptr(), ids.data_ptr(), counts.data_ptr(), emb.data_ptr() if N else 0,
                                            rows.data_ptr() if N else 0, N, S, M, D, float(decay), fused.data_ptr() if N else 0,
                                            nframes.data_ptr() if N else 0, _stream()), "track_fuse")
    return fused, nframes


def track_fuse_host(state: np.ndarray, ids, counts, emb, rows, decay: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
    """`track_fuse` on the CPU over numpy arrays (`frmap_track_fuse_host`: the kernel's rule compiled for the host; no GPU).
    ``state``: a writable uint8 array from `track_fuse_state_host`, updated in place.  A count outside ``[0, max_boxes]``, a row
    that names no detection of this step, two rows of one detection, an unsupported size or ``decay`` raise ``ValueError`` with the
    state untouched."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    emb = np.ascontiguousarray(emb, dtype=np.float32)
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 2)
    if ids.ndim != 2 or emb.ndim != 2 or counts.shape != (ids.shape[0],) or rows.shape[0] != emb.shape[0]:
        raise ValueError(f"track_fuse_host: ids must be int32 [S, max_boxes], counts [S], emb float32 [N, D] and rows [N, 2]; got "
                         f"{ids.shape}, {counts.shape}, {emb.shape} and {rows.shape}")
    S, M = ids.shape
    N, D = emb.shape
    if not (isinstance(state, np.ndarray) and state.dtype == np.uint8 and state.flags.c_contiguous and state.flags.writeable):
        raise ValueError("track_fuse_host: state must be a writable contiguous uint8 array (track_fuse_state_host)")
    if 1 <= M <= TRACK_MAX_BOXES and 1 <= D <= TRACK_FUSE_MAX_DIM and state.size < track_fuse_state_bytes(S, M, D):
        raise ValueError(f"track_fuse_host: state holds {state.size} bytes, {S} streams of {M} boxes of {D} values need "
                         f"{track_fuse_state_bytes(S, M, D)}")
    fused = np.empty((N, D), np.float32)
    nframes = np.empty((N,), np.float32)
    _lib.check(_lib.load().frmap_track_fuse_host(state.ctypes.data, ids.ctypes.data, counts.ctypes.data, emb.ctypes.data if N else None,
                                                 rows.ctypes.data if N else None, N, S, M, D, float(decay),
                                                 fused.ctypes.data if N else None, nframes.ctypes.data if N else None),
               "track_fuse_host")
    return fused, nframes


# every tensor-taking wrapper launches on its operands' device (see _on_operand_device)
for _name in ("pack_input", "pack_conv_weight", "pack_conv_weight_c3", "conv_small_cin", "stem7x7_maxpool", "stem7x7_maxpool_u8", "conv_igemm",
              "conv_igemm_ds", "linear_mfma", "maxpool", "avgpool_global", "avgpool_adaptive", "linear_f32", "l2_normalize",
              "cast_to_f32", "cast_from_f32", "add_pos_layernorm", "mha_tokens", "mean_layernorm", "cnn_attention",
              "normalize_u8", "softmax_argmax", "pairwise_distance", "match_top1", "match_topk", "verify_counts", "match_radius",
              "gap_norm_match", "cosine_logits", "arcmargin_eval", "conv_small_cin_pool2", "conv_igemm_pool2", "gap_linear_norm", "track_step",
              "track_fuse", "classify_tally", "ovr_append", "ovr_rank_counts"):
    globals()[_name] = _on_operand_device(globals()[_name])
del _name
MatchPack.__init__ = _on_operand_device(MatchPack.__init__)          # (`match_prepare` is decorated where it is defined)
MatchPack.update_rows = _on_operand_device(MatchPack.update_rows)


# ------------------------------------------------------------------------------------------------
# model handles (`frmap_model_*`): the per-layer plan, BatchNorm folding and weight packing live in the library
# ------------------------------------------------------------------------------------------------
IN_F32_NCHW, IN_U8_HWC = 0, 1
OUT_TRUNK_MAP, OUT_POOLED, OUT_EMBEDDING, OUT_LOGITS = 0, 1, 2, 3


class ModelHandle:
    """A `frmap_model` built from a module's ``state_dict`` (the reference's key names, device tensors).  Immutable after
    construction; forwards allocate only their outputs and scratch (torch's caching allocator, capturable into a HIP graph)."""

    def __init__(self, model_type: str, state: dict, num_classes: int, dtype: torch.dtype, mean=None, std=None):
        import ctypes as C
        lib = _lib.load()
        self._lib, self._h = lib, C.c_void_p()
        self.dtype, self.model_type, self.num_classes = dtype, model_type, int(num_classes)
        _lib.check(lib.frmap_model_create(C.byref(self._h), model_type.encode(), int(num_classes), dt_code(dtype)), "model_create")
        try:
            dev = None
            for key, t in state.items():
                if not (isinstance(t, torch.Tensor) and t.is_floating_point()):
                    continue
                if not t.is_cuda:
                    raise RuntimeError(f"{key} is on {t.device}; move the module to the GPU (no CPU fallback)")
                dev = t.device if dev is None else dev
                tt = t.detach().to(torch.float32).contiguous()
                with torch.cuda.device(tt.device):
                    # (1 = a key the inference path does not use, e.g. the trunk's own 1000-way fc: ignored)
                    _lib.check(min(lib.frmap_model_load_tensor(self._h, key.encode(), tt.data_ptr(), tt.numel(), 1), 0), f"model_load_tensor({key})")
            self.device = dev
            if mean is not None:
                m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
                _lib.check(lib.frmap_model_set_input_normalization(self._h, m3, s3), "model_set_input_normalization")
            with torch.cuda.device(dev):
                _lib.check(lib.frmap_model_finalize(self._h, _stream()), "model_finalize")
            self.embedding_dim = int(lib.frmap_model_embedding_dim(self._h))
        except Exception:
            lib.frmap_model_destroy(self._h)
            self._h = None
            raise

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        try:
            if h:
                self._lib.frmap_model_destroy(h)
        except Exception:   # interpreter shutdown: the library object may already be gone
            pass

    @staticmethod
    def _geometry(x):
        if x.dtype == torch.uint8:
            return IN_U8_HWC, x.shape[0], x.shape[1], x.shape[2]
        return IN_F32_NCHW, x.shape[0], x.shape[2], x.shape[3]

    def _gallery(self, op: str, gallery: Optional[torch.Tensor], prepared):
        """(G, the gallery as the library reads it - the caller keeps it until the call is queued -, its pointer, packed pointer, stat
        pointer) of a match call; the pack only where it is this gallery's."""
        if gallery is None or not int(gallery.shape[0]):
            return 0, None, 0, 0, 0
        src, gallery = gallery, _dev(gallery, f"model_{op}.gallery", torch.float32)
        if gallery.shape[1] != self.embedding_dim:
            raise ValueError(f"{op}: embedding dim {self.embedding_dim} != gallery dim {gallery.shape[1]}")
        ppk = pst = 0
        if _usable_pack(prepared, src, self.embedding_dim, op) is not None:
            ppk, pst = prepared.packed.data_ptr(), prepared.stat_w.data_ptr()
        return int(gallery.shape[0]), gallery, gallery.data_ptr(), ppk, pst

    def forward(self, x: torch.Tensor, what: int) -> torch.Tensor:
        x = _dev(x, "model_forward.x", None, ("frmap_model_forward", "x"))
        kind, B, H, W = self._geometry(x)
        with torch.cuda.device(x.device):
            if what == OUT_TRUNK_MAP and self.model_type == "baseline":      # three conv + MaxPool2d(2) stages, 128 channels
                out = torch.empty((B, H // 2 // 2 // 2, W // 2 // 2 // 2, 128), dtype=self.dtype, device=x.device)
            elif what == OUT_TRUNK_MAP and self.model_type == "siamese":     # 7x7 stride 2, then three MaxPool2d(2), 512 channels
                hc, wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
                out = torch.empty((B, hc // 2 // 2 // 2, wc // 2 // 2 // 2, 512), dtype=self.dtype, device=x.device)
            elif what == OUT_TRUNK_MAP:
                hq, wq = stem_pool_dims(H, W)
                for _ in range(3):
                    hq, wq = (hq - 1) // 2 + 1, (wq - 1) // 2 + 1
                out = torch.empty((B, hq, wq, 512), dtype=self.dtype, device=x.device)
            else:
                out = torch.empty((B, self.num_classes if what == OUT_LOGITS else self.embedding_dim), dtype=torch.float32, device=x.device)
            ws = torch.empty((self._lib.frmap_model_workspace_bytes(self._h, B, H, W),), dtype=torch.uint8, device=x.device)
            _lib.check(self._lib.frmap_model_forward(self._h, x.data_ptr(), kind, B, H, W, what, out.data_ptr(), ws.data_ptr(), _stream()),
                       "model_forward")
        return out

    def embed_and_match(self, x: torch.Tensor, gallery: Optional[torch.Tensor], prepared, thresh: float, normalize: bool,
                        packed=False, want_emb: bool = False):
        """One C call: forward + top-1 match.  Returns (idx, dist, ids, packed | None, emb | None)."""
        x = _dev(x, "model_embed_and_match.x", None, ("frmap_model_embed_and_match", "x"))
        kind, B, H, W = self._geometry(x)
        with torch.cuda.device(x.device):
            G, gallery, gptr, ppk, pst = self._gallery("embed_and_match", gallery, prepared)
            idx = torch.empty((B,), dtype=torch.int32, device=x.device)
            dist = torch.empty((B,), dtype=torch.float32, device=x.device)
            ids = torch.empty((B,), dtype=torch.int32, device=x.device)
            pk = _packed_buf(packed, B, x.device)
            emb = torch.empty((B, self.embedding_dim), dtype=torch.float32, device=x.device) if want_emb else None
            ws = torch.empty((self._lib.frmap_model_match_workspace_bytes(self._h, B, H, W, G),), dtype=torch.uint8, device=x.device)
            _lib.check(self._lib.frmap_model_embed_and_match(self._h, x.data_ptr(), kind, B, H, W, gptr, ppk, pst, G, float(thresh),
                                                             int(bool(normalize)), idx.data_ptr(), dist.data_ptr(), ids.data_ptr(),
                                                             pk.data_ptr() if pk is not None else 0,
                                                             emb.data_ptr() if emb is not None else 0, ws.data_ptr(), _stream()),
                       "model_embed_and_match")
        return idx, dist, ids, pk, emb

    def embed_and_search(self, x: torch.Tensor, gallery: Optional[torch.Tensor], prepared, k: int, labels: Optional[torch.Tensor] = None,
                         normalize: bool = False, want_emb: bool = False):
        """One C call: forward + exact top-k search (`match_topk`).  Returns (idx [B, k], dist [B, k], label [B, k] | None, emb | None)."""
        x = _dev(x, "model_embed_and_search.x", None, ("frmap_model_embed_and_search", "x"))
        kind, B, H, W = self._geometry(x)
        k = int(k)
        if not 1 <= k <= MATCH_TOPK_MAX:
            raise ValueError(f"embed_and_search: k={k} out of range (1 <= k <= {MATCH_TOPK_MAX})")
        with torch.cuda.device(x.device):
            G, gallery, gptr, ppk, pst = self._gallery("embed_and_search", gallery, prepared)
            lptr = 0
            if labels is not None:
                labels = _dev(labels, "model_embed_and_search.labels", torch.int32, ("frmap_model_embed_and_search", "labels"))
                if tuple(labels.shape) != (G,):
                    raise ValueError(f"embed_and_search: labels must be int32 [{G}]")
            idx = torch.empty((B, k), dtype=torch.int32, device=x.device)
            dist = torch.empty((B, k), dtype=torch.float32, device=x.device)
            lab = torch.empty((B, k), dtype=torch.int32, device=x.device) if labels is not None else None
            emb = torch.empty((B, self.embedding_dim), dtype=torch.float32, device=x.device) if want_emb else None
            ws = torch.empty((self._lib.frmap_model_search_workspace_bytes(self._h, B, H, W, G, k),), dtype=torch.uint8, device=x.device)
            if labels is not None:
                lptr = labels.data_ptr() if G else ws.data_ptr()
            _lib.check(self._lib.frmap_model_embed_and_search(self._h, x.data_ptr(), kind, B, H, W, gptr, ppk, pst, lptr, G, k,
                                                              int(bool(normalize)), idx.data_ptr(), dist.data_ptr(),
                                                              lab.data_ptr() if lab is not None else 0,
                                                              emb.data_ptr() if emb is not None else 0, ws.data_ptr(), _stream()),
                       "model_embed_and_search")
        return idx, dist, lab, emb

    def trace(self, enable: bool) -> None:
        _lib.check(self._lib.frmap_model_trace(self._h, int(bool(enable))), "model_trace")

    def trace_read(self, max_records: int = 4096):
        """[(kernel label, algorithmic FLOPs, algorithmic bytes, microseconds)] of the forwards since the last read."""
        import ctypes as C

        class Rec(C.Structure):
            _fields_ = [("kernel", C.c_char * 64), ("flop", C.c_double), ("bytes", C.c_double), ("us", C.c_float)]
        buf = (Rec * max_records)()
        n = self._lib.frmap_model_trace_read(self._h, C.cast(buf, C.c_void_p), max_records)
        _lib.check(min(n, 0), "model_trace_read")
        return [(buf[i].kernel.decode(), buf[i].flop, buf[i].bytes, buf[i].us) for i in range(n)]
