"""Host-side mirror of the reference model zoo's inference surface, computing on the HIP kernels.

Same names, argument meaning, ``state_dict`` keys and error behaviour as
``/root/reference/src/face_models.py`` for the hot path:

* ``get_model(model_type, num_classes=18, input_size=(224, 224))``  (`face_models.py:785-813`)
* ``BaselineNet`` (`:16-60`), ``ResNetTransfer`` (`:62-102`), ``SiameseNet`` (`:104-192`),
  ``ArcMarginProduct`` eval (`:297-445`), ``ArcFaceNet`` eval (`:447-613`), ``HybridNet`` (`:650-721`)

The modules are ordinary ``nn.Module`` parameter containers (so ``.to()``, ``.eval()``,
``.state_dict()`` and ``load_state_dict()`` of a reference ``best_model.pth`` work), but
``forward`` / ``get_embedding`` do not call ``torch.nn`` ops: they fold BatchNorm into the
neighbouring conv / linear (fp32), pack the weights once into the kernels' layout, and launch the
hand-written gfx950 kernels through the C ABI (``ops.py``).  Inputs must be fp32 NCHW tensors on
the GPU and the module must be on the GPU and in ``eval()`` mode; anything else raises — there is
no eager / CPU fallback.  Training (`face_models.py:527-572`, losses `:725-782`) is out of scope.
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops

MODEL_TYPES = ['baseline', 'cnn', 'siamese', 'attention', 'arcface', 'hybrid', 'ensemble']

_DEFAULT_DTYPE = torch.bfloat16
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)   # `src/testing.py:102-103`


def set_default_compute_dtype(dtype: torch.dtype) -> None:
    """bf16 (default; BASELINE.json's benchmark precision) or fp16 (the precision at which the
    ≤1e-3 embedding-cosine bound of the north star is stated)."""
    global _DEFAULT_DTYPE
    ops.dt_code(dtype)
    _DEFAULT_DTYPE = dtype


# --------------------------------------------------------------------------------------------
# folding helpers (fp32, one-off per weight version)
# --------------------------------------------------------------------------------------------
def _bn_scale_shift(bn: nn.Module, bias: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Eval BatchNorm as y = x*scale + shift; a preceding conv/linear bias is absorbed in shift."""
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    shift = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
    if bias is not None:
        shift = shift + bias.detach().float() * scale
    return scale.contiguous(), shift.contiguous()


_PY_PLAN = os.environ.get("FRMAP_PY_PLAN", "0") == "1"      # A/B switch: 1 = plan the ResNet-18 families in Python (per-op C ABI calls)
_HEAD_FUSE = os.environ.get("FRMAP_HEAD_FUSE", "1") != "0"   # A/B switch: 0 = ArcFace head as avgpool + linear + normalize launches
_POOL_FUSE = os.environ.get("FRMAP_POOL_FUSE", "1") != "0"   # A/B switch: 0 = conv and 2x2 max-pool as two launches


@contextlib.contextmanager
def planned_in_python(on: bool = True):
    """Plans BUILT inside are per-op (`on`) or on the model handle, as under FRMAP_PY_PLAN=1 / 0; a plan that exists keeps its route."""
    global _PY_PLAN
    old, _PY_PLAN = _PY_PLAN, bool(on)
    try:
        yield
    finally:
        _PY_PLAN = old


# Every per-op forward below takes an optional recorder `rec`.  After each step it is called as `rec(name, stored, by, inputs)`: the step's
# name, the tensor the step stored, the packed object (or, where there is none, the `ops` function) that computed it, and that
# one's input tensors - what tests/test_model_twin_gpu.py needs to hold every step to its float64 twin.  Without one a step costs
# the `is None` test.
class _PackedConv:
    __slots__ = ("wpk", "shift", "cout", "k", "stride", "pad", "small")

    def __init__(self, conv: nn.Conv2d, bn: Optional[nn.Module], dtype: torch.dtype):
        w = conv.weight.detach().float()
        if bn is not None:
            scale, shift = _bn_scale_shift(bn, conv.bias)
            w = w * scale.view(-1, 1, 1, 1)
        else:
            shift = conv.bias.detach().float() if conv.bias is not None else torch.zeros(w.shape[0], device=w.device)
        self.cout, cin, kh, kw = w.shape
        self.k, self.stride, self.pad = kh, conv.stride[0], conv.padding[0]
        self.small = cin == 3
        self.wpk = ops.pack_conv_weight_c3(w.contiguous(), dtype) if self.small else ops.pack_conv_weight(w.contiguous(), dtype)
        self.shift = shift.contiguous()

    def __call__(self, x: torch.Tensor, relu: bool, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.small:
            return ops.conv_small_cin(x, self.wpk, self.shift, self.cout, self.k, self.stride, self.pad, relu)
        return ops.conv_igemm(x, self.wpk, self.shift, self.cout, self.k, self.stride, self.pad, relu, residual)

    def pooled(self, x: torch.Tensor, relu: bool = True, rec=None, name: str = "") -> torch.Tensor:
        """conv + shift (+ReLU) + MaxPool2d(2, 2) (`face_models.py:38-40,121-141`): one launch when the kernels take the
        shape (the conv map never reaches HBM; step `name+pool2`), conv + pool kernels otherwise (steps `name`, `name.pool2`)."""
        B, H, W, C = x.shape
        fusable = self.k == 3 and self.stride == 1 and self.pad == 1 and H % 2 == 0 and W % 2 == 0 and _POOL_FUSE
        if fusable and (self.cout == 32 if self.small else ops.conv_pool2_supported(B, H, W, C, self.cout)):
            fused = ops.conv_small_cin_pool2 if self.small else ops.conv_igemm_pool2
            y = fused(x, self.wpk, self.shift, self.cout, relu)
            if rec is not None:
                rec(name + "+pool2", y, self, (x,))
            return y
        c = self(x, relu)
        y = ops.maxpool(c, 2, 2, 0)
        if rec is not None:
            rec(name, c, self, (x,))
            rec(name + ".pool2", y, ops.maxpool, (c,))
        return y


class _PackedLinearAsConv:
    """Wide nn.Linear (+BatchNorm1d) run on the MFMA conv kernel as a 1x1 conv over H=W=1."""
    __slots__ = ("wpk", "shift", "cout")

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor], bn: Optional[nn.Module], dtype: torch.dtype):
        w = weight.detach().float()
        if bn is not None:
            scale, shift = _bn_scale_shift(bn, bias)
            w = w * scale.view(-1, 1)
        else:
            shift = bias.detach().float() if bias is not None else torch.zeros(w.shape[0], device=w.device)
        self.cout = w.shape[0]
        self.wpk = ops.pack_conv_weight(w.reshape(w.shape[0], w.shape[1], 1, 1).contiguous(), dtype)
        self.shift = shift.contiguous()

    def __call__(self, x2d: torch.Tensor, relu, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        return ops.linear_mfma(x2d, self.wpk, self.shift, self.cout, relu, residual)


# --------------------------------------------------------------------------------------------
# base class: plan cache + input checks
# --------------------------------------------------------------------------------------------
class _HipModule(nn.Module):
    """nn.Module whose inference runs on the HIP kernels.  The packed-weight "plan" is rebuilt
    whenever a parameter/buffer is replaced, moved or modified in place (tensor version counters).  A plan is the family's
    own model handle (`_TrunkPlan`) where the A/B switches allow it and the family's per-op plan otherwise (`_build_plan`); the
    public methods ask it for `embedding` / `logits` / `features` / `pooled` / `unit_embedding` and either kind answers."""

    def __init__(self):
        super().__init__()
        self._plans = {}          # per_op -> (plan, the signature it was built from)
        self.compute_dtype = _DEFAULT_DTYPE
        # uint8 HWC inputs (B×H×W×3 RGB, what `transforms.Resize` leaves, `src/testing.py:99-100`) are normalised on the
        # device: ToTensor + Normalize(mean, std) of `src/testing.py:101-104` (ImageNet statistics by default)
        self.input_mean, self.input_std = IMAGENET_MEAN, IMAGENET_STD

    supports_u8_input = True

    def set_input_normalization(self, mean, std):
        self.input_mean, self.input_std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        return self

    def set_compute_dtype(self, dtype: torch.dtype):
        ops.dt_code(dtype)
        self.compute_dtype = dtype
        self._plans.clear()
        return self

    def _signature(self):
        sig = [self.compute_dtype, self.input_mean, self.input_std]
        for t in list(self.parameters()) + list(self.buffers()):
            sig.append((t.data_ptr(), t._version))
        return tuple(sig)

    def _get_plan(self, per_op: bool = False):
        """The plan the switches choose, or with `per_op` the family's per-op plan whatever they say (the other one is not touched)."""
        sig = self._signature()
        cached = self._plans.get(per_op)
        if cached is None or sig != cached[1]:
            dev = next(self.parameters()).device
            if dev.type != "cuda":
                raise RuntimeError(f"{type(self).__name__} is on {dev}; move it to the GPU (.to('cuda')) — "
                                   "the HIP path has no CPU fallback")
            with torch.no_grad():
                plan = self._build_plan(self.compute_dtype, per_op)
            self._plans[per_op] = cached = (plan, self._signature())
        return cached[0]

    def _build_plan(self, dtype, per_op=False):  # pragma: no cover - abstract
        raise NotImplementedError

    def model_handle(self):
        """The `frmap_model` of this family behind the module, on which `matching.embed_and_match` runs in one call; None when
        the plan is per-op (FRMAP_PY_PLAN=1, a fusing switch off, AttentionNet) - a bare-trunk handle inside such a plan is not it."""
        return self._get_plan().handle

    def get_embedding(self, x):
        x = self._check_input(x)
        return self._get_plan().embedding(x)

    def _check_input(self, x: torch.Tensor) -> torch.Tensor:
        """fp32 NCHW B×3×H×W (the reference's tensor) or uint8 HWC B×H×W×3 (the image bytes; normalised on the device)."""
        u8 = isinstance(x, torch.Tensor) and x.dtype == torch.uint8
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or (x.shape[3] != 3 if u8 else x.shape[1] != 3):
            raise ValueError(f"expected a B×3×H×W float tensor or a B×H×W×3 uint8 tensor, got "
                             f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
        if not x.is_cuda:
            raise RuntimeError("input is on the CPU; the HIP path needs GPU tensors (no CPU fallback)")
        if self.training:
            raise NotImplementedError(f"{type(self).__name__}: only eval-mode inference is implemented on the HIP path; "
                                      "call .eval() (training is out of scope, SURVEY.md §2.1)")
        if u8:
            return x
        return x.float() if x.dtype != torch.float32 else x

    def _as_nhwc4(self, x: torch.Tensor, rec=None) -> torch.Tensor:
        return _nhwc4(x, self.compute_dtype, self.input_mean, self.input_std, rec)


def _nhwc4(x: torch.Tensor, dtype: torch.dtype, mean, std, rec=None) -> torch.Tensor:
    """First-layer operand of the unfused paths (step `pack_input`): NHWC4 in the compute dtype from either input kind."""
    if x.dtype == torch.uint8:
        x4 = ops.normalize_u8(x, mean, std, want_nchw=False, nhwc4_dtype=dtype)[1]
    else:
        x4 = ops.pack_input(x, dtype)
    if rec is not None:
        rec("pack_input", x4, ops.normalize_u8 if x.dtype == torch.uint8 else ops.pack_input, (x,))
    return x4


# --------------------------------------------------------------------------------------------
# ResNet-18 parameter container with torchvision's attribute names / order
# (torchvision is un-vendored; call sites face_models.py:67,269,463,658)
# --------------------------------------------------------------------------------------------
class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        raise RuntimeError("BasicBlock is a parameter container; inference runs through the owning HIP module")


class ResNet18(nn.Module):
    """Parameter container: ``conv1 bn1 relu maxpool layer1..4 avgpool fc`` (children order matters —
    the reference slices ``children()[:-1]`` / ``[:-2]``, `face_models.py:100,464,660`)."""

    def __init__(self, num_classes: int = 1000):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inpl = 64
        for i, (planes, stride) in enumerate(((64, 1), (128, 2), (256, 2), (512, 2)), start=1):
            ds = None
            if stride != 1 or inpl != planes:
                ds = nn.Sequential(nn.Conv2d(inpl, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))
            setattr(self, f"layer{i}", nn.Sequential(BasicBlock(inpl, planes, stride, ds), BasicBlock(planes, planes)))
            inpl = planes
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512, num_classes)

    def forward(self, x):
        raise RuntimeError("ResNet18 is a parameter container; inference runs through the owning HIP module")


HANDLE_BN_EPS = 1e-5      # the eps `frmap_model_finalize` folds every BatchNorm with (include/frmap_hip.h)


def _check_handle_eps(owner: nn.Module) -> None:
    """A `state_dict` does not carry `eps`, so a model handle cannot see it: refuse a module whose BatchNorm has another one
    instead of computing other numbers than the Python planner (which folds with `bn.eps`) without a word."""
    for name, mod in owner.named_modules():
        if isinstance(mod, (nn.BatchNorm1d, nn.BatchNorm2d)) and mod.eps != HANDLE_BN_EPS:
            raise ValueError(f"{type(owner).__name__}.{name}: BatchNorm eps = {mod.eps:g}, but the model handle folds with eps = "
                             f"{HANDLE_BN_EPS:g} (frmap_model_finalize); set FRMAP_PY_PLAN=1 to plan this module in Python")


class _TrunkPlan:
    """A family, or the bare ResNet-18 trunk ('resnet18_trunk'), on a MODEL HANDLE of the C ABI (`frmap_model_*`,
    csrc/model_api.cpp): BatchNorm folding, weight packing and the per-layer kernel plan live in the library; this class only
    hands over the tensors under the reference's ``state_dict`` key names and asks for outputs."""

    def __init__(self, model_type: str, state: Dict[str, torch.Tensor], num_classes: int, dtype: torch.dtype,
                 mean=IMAGENET_MEAN, std=IMAGENET_STD, owner: Optional[nn.Module] = None):
        if owner is not None:
            _check_handle_eps(owner)
        self.dtype = dtype
        self.handle = ops.ModelHandle(model_type, state, num_classes, dtype, mean, std)

    def _out(self, x: torch.Tensor, what: int, rec=None) -> torch.Tensor:
        if rec is not None:
            raise ValueError("a model handle stores no per-step tensors to record: build the plan under planned_in_python()")
        return self.handle.forward(x, what)

    def features(self, x: torch.Tensor, rec=None) -> torch.Tensor:
        """fp32 NCHW (or uint8 HWC) → NHWC B×7×7×512 (for 224² input) in the compute dtype."""
        return self._out(x, ops.OUT_TRUNK_MAP, rec)

    def pooled(self, x: torch.Tensor, rec=None) -> torch.Tensor:
        return self._out(x, ops.OUT_POOLED, rec)  # fp32 B×512

    def embedding(self, x: torch.Tensor) -> torch.Tensor:
        return self.handle.forward(x, ops.OUT_EMBEDDING)

    def logits(self, x: torch.Tensor) -> torch.Tensor:
        return self.handle.forward(x, ops.OUT_LOGITS)

    def unit_embedding(self, x: torch.Tensor) -> torch.Tensor:
        return ops.l2_normalize(self.embedding(x), 1e-12)


def _trunk_plan(rn: "ResNet18", dtype: torch.dtype, mean, std, owner: Optional[nn.Module] = None):
    """The bare trunk of HybridNet / AttentionNet: a 'resnet18_trunk' handle, or the Python planner under FRMAP_PY_PLAN=1."""
    if _PY_PLAN:
        return _PyTrunkPlan(rn, dtype, mean, std)
    return _TrunkPlan("resnet18_trunk", dict(rn.state_dict()), 0, dtype, mean, std, owner=owner or rn)


class _PyTrunkPlan:
    """The same trunk planned in Python, one C-ABI op per call (`FRMAP_PY_PLAN=1`): the A/B twin of the model handle - same
    launches on the same folded weights, bit-identical outputs (tests/test_model_cabi_gpu.py) - and the path per-op tools wrap."""

    handle = None     # (no model handle: `_HipModule.model_handle`)

    def __init__(self, rn: ResNet18, dtype: torch.dtype, mean=IMAGENET_MEAN, std=IMAGENET_STD, fc: Optional[nn.Linear] = None):
        self.dtype = dtype
        self.mean, self.std = mean, std
        self.fc = fc      # 'cnn': the classifier over the pooled map
        self.stem = _PackedConv(rn.conv1, rn.bn1, dtype)
        self.blocks = []
        for li in range(1, 5):
            for blk in getattr(rn, f"layer{li}"):
                ds = _PackedConv(blk.downsample[0], blk.downsample[1], dtype) if blk.downsample is not None else None
                c2 = _PackedConv(blk.conv2, blk.bn2, dtype)
                # (shift of the fused conv2 + shortcut launch: both folded BatchNorm shifts)
                fshift = (c2.shift + ds.shift).contiguous() if ds is not None else None
                self.blocks.append((_PackedConv(blk.conv1, blk.bn1, dtype), c2, ds, fshift))

    def features(self, x: torch.Tensor, rec=None) -> torch.Tensor:
        """fp32 NCHW (or uint8 HWC) → NHWC B×7×7×512 (for 224² input) in the compute dtype."""
        u8, img = x.dtype == torch.uint8, x
        H, W = (x.shape[1], x.shape[2]) if u8 else (x.shape[2], x.shape[3])
        if ops.stem_pool_dims(H, W)[1] <= 56 and (not u8 or W % 4 == 0):     # fused stem, one kernel
            if u8:   # it reads the image bytes; ToTensor + Normalize happen while its rows are staged
                x = ops.stem7x7_maxpool_u8(x, self.stem.wpk, self.stem.shift, self.mean, self.std, self.dtype)
            else:
                x = ops.stem7x7_maxpool(x, self.stem.wpk, self.stem.shift, self.dtype)
            if rec is not None:
                rec("stem+pool3", x, self.stem, (img,))
        else:  # wider than the fused kernel's 8 column strips (or bytes whose rows are no multiple of 4)
            x4 = _nhwc4(x, self.dtype, self.mean, self.std, rec)
            c = self.stem(x4, relu=True)
            x = ops.maxpool(c, 3, 2, 1)
            if rec is not None:
                rec("stem", c, self.stem, (x4,))
                rec("stem.pool3", x, ops.maxpool, (c,))
        for i, (c1, c2, ds, fshift) in enumerate(self.blocks):
            h = c1(x, relu=True)
            fused = ds is not None and ds.k == 1 and ops.conv_ds_supported(*h.shape, c2.cout, *x.shape[1:], ds.stride)
            if fused:   # conv2 + bn2 + projection shortcut + add + ReLU in one launch (the shortcut as extra K stages)
                y = ops.conv_igemm_ds(h, c2.wpk, fshift, c2.cout, x, ds.wpk, ds.stride, True)
            else:
                res = x if ds is None else ds(x, relu=False)
                y = c2(h, relu=True, residual=res)
            if rec is not None:
                name = f"layer{i // 2 + 1}.{i % 2}."
                rec(name + "conv1", h, c1, (x,))
                if fused:
                    rec(name + "conv2+ds", y, (c2, ds), (h, x))
                else:
                    if ds is not None:
                        rec(name + "downsample", res, ds, (x,))
                    rec(name + "conv2", y, c2, (h, res))
            x = y
        return x

    def pooled(self, x: torch.Tensor, rec=None) -> torch.Tensor:
        f = self.features(x, rec)
        y = ops.avgpool_global(f)  # fp32 B×512
        if rec is not None:
            rec("avgpool", y, ops.avgpool_global, (f,))
        return y

    def logits(self, x: torch.Tensor) -> torch.Tensor:
        return ops.linear_f32(self.pooled(x), self.fc.weight.detach(), None, self.fc.bias.detach())


class _PerOpPlan(dict):
    """A family planned in Python: its packed operands by name (a dict: bench.py's roofline pass looks up "trunk") and, in the
    subclasses, the family's one per-op forward over them, `embedding(x, rec=None)`."""
    handle = None     # (no model handle of the family's own: `_HipModule.model_handle`)

    def __init__(self, m: nn.Module, fc: Optional[nn.Linear] = None, **operands):
        super().__init__(operands)
        self.m, self.fc = m, fc      # the owning module; its classifier over the embedding

    def logits(self, x: torch.Tensor) -> torch.Tensor:
        return ops.linear_f32(self.embedding(x), self.fc.weight.detach(), None, self.fc.bias.detach())


# --------------------------------------------------------------------------------------------
# a2  BaselineNet
# --------------------------------------------------------------------------------------------
class _PyBaselinePlan(_PerOpPlan):
    def __init__(self, m: "BaselineNet", dtype: torch.dtype):
        super().__init__(m, m.fc2, c1=_PackedConv(m.conv1, m.bn1, dtype), c2=_PackedConv(m.conv2, m.bn2, dtype),
                         c3=_PackedConv(m.conv3, m.bn3, dtype), fc1_t=m.fc1.weight.detach().float().t().contiguous())

    def pooled_map(self, x: torch.Tensor, rec=None) -> torch.Tensor:
        x = self.m._as_nhwc4(x, rec)
        for key, name in (("c1", "conv1"), ("c2", "conv2"), ("c3", "conv3")):   # self.pool(F.relu(self.bn1(self.conv1(x)))), `face_models.py:38-40`
            x = self[key].pooled(x, rec=rec, name=name)
        return x

    def pooled(self, x: torch.Tensor) -> torch.Tensor:
        return ops.avgpool_global(self.pooled_map(x))

    def embed(self, x: torch.Tensor, rec=None):
        """-> (embedding as the reference returns it, its unit-norm copy or None)."""
        x, fc1 = self.pooled_map(x, rec), self.m.fc1
        if _HEAD_FUSE:   # adaptive_pool + fc1 + ReLU (`face_models.py:41-46`) in one launch, the unit-norm copy for the matcher with it
            emb, pre = ops.gap_linear_norm(x, self["fc1_t"], None, fc1.bias.detach(), 1e-12, want_pre=True, relu=True)
            if rec is not None:
                rec("fc1+relu", pre, ops.gap_linear_norm, (x,))
                rec("fc1+relu.unit", emb, ops.gap_linear_norm, (x,))
            return pre, emb
        f = ops.avgpool_global(x)
        pre = ops.linear_f32(f, fc1.weight.detach(), None, fc1.bias.detach(), relu=True)
        if rec is not None:
            rec("avgpool", f, ops.avgpool_global, (x,))
            rec("fc1+relu", pre, ops.linear_f32, (f,))
        return pre, None

    def embedding(self, x: torch.Tensor, rec=None) -> torch.Tensor:
        return self.embed(x, rec)[0]

    def unit_embedding(self, x: torch.Tensor) -> torch.Tensor:
        pre, emb = self.embed(x)
        return emb if emb is not None else ops.l2_normalize(pre, 1e-12)


class BaselineNet(_HipModule):
    """`face_models.py:16-60`."""

    def __init__(self, num_classes: int = 18, input_size: Tuple[int, int] = (224, 224)):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 32, 3, padding=1)
        self.bn1 = nn.BatchNorm2d(32)
        self.conv2 = nn.Conv2d(32, 64, 3, padding=1)
        self.bn2 = nn.BatchNorm2d(64)
        self.conv3 = nn.Conv2d(64, 128, 3, padding=1)
        self.bn3 = nn.BatchNorm2d(128)
        self.pool = nn.MaxPool2d(2, 2)
        self.adaptive_pool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Linear(128, 512)
        self.fc2 = nn.Linear(512, num_classes)
        self.dropout = nn.Dropout(0.5)

    def _build_plan(self, dtype, per_op=False):
        if per_op or _PY_PLAN or not (_HEAD_FUSE and _POOL_FUSE):
            return _PyBaselinePlan(self, dtype)
        return _TrunkPlan("baseline", dict(self.state_dict()), self.fc2.out_features, dtype, self.input_mean, self.input_std, owner=self)

    def pooled_features(self, x):
        """fp32 ``[B, 128]``: the output of ``adaptive_pool``, the input of ``fc1`` - what `head_fit.cache_features(layer="pooled")`
        caches so that a `head_fit.HiddenHead` can fit ``fc1`` / ``fc2``.  The per-op route (three conv + pool launches and the
        global average pool) on the per-op plan, whatever the switches say; the model handle is not touched."""
        x = self._check_input(x)
        return self._get_plan(per_op=True).pooled(x)

    def unit_embedding(self, x):
        """``F.normalize(get_embedding(x))`` (what `embed_and_match(normalize=True)` matches on) without a second launch."""
        x = self._check_input(x)
        return self._get_plan().unit_embedding(x)

    def forward(self, x):
        return self._get_plan().logits(self._check_input(x))


# --------------------------------------------------------------------------------------------
# a3  ResNetTransfer ('cnn')
# --------------------------------------------------------------------------------------------
class ResNetTransfer(_HipModule):
    """`face_models.py:62-102`.  No pretrained-weight fetch (offline); load a checkpoint instead."""

    def __init__(self, num_classes: int = 18, freeze_backbone: bool = False):
        super().__init__()
        self.resnet = ResNet18()
        in_feats = self.resnet.fc.in_features
        self.dropout = nn.Dropout(0.1)
        self.resnet.fc = nn.Sequential(self.dropout, nn.Linear(in_feats, num_classes))
        if freeze_backbone:
            self._freeze_backbone()

    def _freeze_backbone(self):
        for name, param in self.resnet.named_parameters():
            if "fc" not in name:
                param.requires_grad = False

    def unfreeze_backbone(self):
        for param in self.resnet.parameters():
            param.requires_grad = True

    def _build_plan(self, dtype, per_op=False):
        fc = self.resnet.fc[1]
        if per_op or _PY_PLAN:
            return _PyTrunkPlan(self.resnet, dtype, self.input_mean, self.input_std, fc=fc)
        return _TrunkPlan("cnn", {f"resnet.{k}": v for k, v in self.resnet.state_dict().items()}, fc.out_features, dtype,
                          self.input_mean, self.input_std, owner=self)

    def forward(self, x):
        x = self._check_input(x)
        return self._get_plan().logits(x)

    def trunk_map(self, x):
        """The NHWC trunk output whose global average pool is ``get_embedding`` (`face_models.py:98-102`); lets
        ``matching.embed_and_match`` pool, normalise and match in one kernel."""
        x = self._check_input(x)
        return self._get_plan().features(x)

    def get_embedding(self, x):
        x = self._check_input(x)
        return self._get_plan().pooled(x).squeeze()  # `.squeeze()` as the reference (`:102`): (512,) at B == 1


# --------------------------------------------------------------------------------------------
# a6  SiameseNet
# --------------------------------------------------------------------------------------------
class _PySiamesePlan(_PerOpPlan):
    def __init__(self, m: "SiameseNet", dtype: torch.dtype):
        c, fc = m.conv, m.fc
        # fc.1 consumes the NCHW flatten (index c*36 + s, `face_models.py:171`); our pooled tensor is
        # NHWC (index s*512 + c): permute the weight's input axis once here.
        w1 = fc[1].weight.detach().float().view(1024, 512, 36).permute(0, 2, 1).reshape(1024, 36 * 512)
        super().__init__(m, None,    # convs: (packed conv + BatchNorm, a MaxPool2d(2) follows), named by CONVS
                         convs=[(_PackedConv(c[i], c[i + 1], dtype), pool) for i, pool in
                                ((0, True), (4, False), (7, True), (11, False), (14, True), (18, False))],
                         fc1=_PackedLinearAsConv(w1, fc[1].bias, fc[2], dtype), fc2=_PackedLinearAsConv(fc[5].weight, fc[5].bias, fc[6], dtype),
                         fc3=_PackedLinearAsConv(fc[8].weight, fc[8].bias, None, dtype))

    CONVS = ("conv.0", "conv.4", "conv.7", "conv.11", "conv.14", "conv.18")     # step names: the layers' indices in `conv`
    FCS = (("fc.1", "fc1", True), ("fc.5", "fc2", True), ("fc.8", "fc3", False))  # (step name, operand, ReLU): Linear -> BN -> ReLU twice, Linear

    def embedding(self, x: torch.Tensor, rec=None, last_fc: int = 3) -> torch.Tensor:
        """``last_fc=2``: stop before ``fc.8`` and return its fp32 ``[B, 512]`` input (`SiameseNet.fc_hidden_features`)."""
        m, convs, names = self.m, self["convs"], self.CONVS
        u8, img = x.dtype == torch.uint8, x
        Wi = x.shape[2] if u8 else x.shape[3]
        if ((Wi + 6 - 7) // 2 + 1) // 2 <= 64 and (not u8 or Wi % 4 == 0):   # fused conv.0-3: 7x7 conv + bias + BN + ReLU + MaxPool2d(2,2)
            stem = convs[0][0]
            if u8:
                x = ops.stem7x7_maxpool_u8(x, stem.wpk, stem.shift, m.input_mean, m.input_std, m.compute_dtype, pool3=False)
            else:
                x = ops.stem7x7_maxpool(x, stem.wpk, stem.shift, m.compute_dtype, pool3=False)
            if rec is not None:
                rec("conv.0+pool2", x, stem, (img,))
            convs, names = convs[1:], names[1:]
        else:
            x = m._as_nhwc4(x, rec)
        for name, (conv, pool) in zip(names, convs):     # conv -> BN -> ReLU (-> MaxPool2d(2)), `face_models.py:121-146`
            if pool:
                x = conv.pooled(x, rec=rec, name=name)
                continue
            xin, x = x, conv(x, relu=True)
            if rec is not None:
                rec(name, x, conv, (xin,))
        a = ops.avgpool_adaptive(x, 6, 6)  # NHWC B×6×6×512
        if rec is not None:
            rec("avgpool6x6", a, ops.avgpool_adaptive, (x,))
        feats = a.view(a.shape[0], -1)
        for name, key, relu in self.FCS[:last_fc]:
            fin, feats = feats, self[key](feats, relu=relu)
            if rec is not None:
                rec(name, feats, self[key], (fin,))
        if last_fc < len(self.FCS):
            return ops.cast_to_f32(feats)
        f32 = ops.cast_to_f32(feats)
        y = ops.l2_normalize(f32, 1e-12)
        if rec is not None:
            rec("cast_f32", f32, ops.cast_to_f32, (feats,))
            rec("normalize", y, ops.l2_normalize, (f32,))
        return y


class SiameseNet(_HipModule):
    """`face_models.py:104-192`."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Sequential(
            nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
            nn.MaxPool2d(2, stride=2),
            nn.Conv2d(64, 128, kernel_size=3, padding=1), nn.BatchNorm2d(128), nn.ReLU(inplace=True),
            nn.Conv2d(128, 128, kernel_size=3, padding=1), nn.BatchNorm2d(128), nn.ReLU(inplace=True),
            nn.MaxPool2d(2, stride=2),
            nn.Conv2d(128, 256, kernel_size=3, padding=1), nn.BatchNorm2d(256), nn.ReLU(inplace=True),
            nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.BatchNorm2d(256), nn.ReLU(inplace=True),
            nn.MaxPool2d(2, stride=2),
            nn.Conv2d(256, 512, kernel_size=3, padding=1), nn.BatchNorm2d(512), nn.ReLU(inplace=True),
            nn.AdaptiveAvgPool2d((6, 6)),
        )
        self.fc = nn.Sequential(
            nn.Dropout(0.3), nn.Linear(512 * 6 * 6, 1024), nn.BatchNorm1d(1024), nn.ReLU(inplace=True),
            nn.Dropout(0.2), nn.Linear(1024, 512), nn.BatchNorm1d(512), nn.ReLU(inplace=True),
            nn.Linear(512, 256),
        )
        self.debug_shapes = {}

    def _build_plan(self, dtype, per_op=False):
        if per_op or _PY_PLAN or not _POOL_FUSE:
            return _PySiamesePlan(self, dtype)
        return _TrunkPlan("siamese", dict(self.state_dict()), 0, dtype, self.input_mean, self.input_std, owner=self)

    def forward_one(self, x):
        x = self._check_input(x)
        p, B = self._get_plan(), x.size(0)
        # the reference's shape log is static (the adaptive pool fixes 6 x 6): on the model handle the whole tower is one call
        self.debug_shapes.update(input=x.shape, after_conv=torch.Size((B, 512, 6, 6)), flattened=torch.Size((B, 512 * 6 * 6)),
                                 before_norm=torch.Size((B, 256)))
        return p.embedding(x)

    def forward(self, x1, x2):
        return self.forward_one(x1), self.forward_one(x2)

    def fc_hidden_features(self, x):
        """fp32 ``[B, 512]``: the output of ``fc.5`` + BatchNorm + ReLU, the input of the last layer ``fc.8`` - what
        `head_fit.cache_embeddings(layer="fc_hidden")` caches so that a `head_fit.PairHead` can fit ``fc.8``.  On the per-op plan,
        whatever the switches say; the model handle is not touched."""
        x = self._check_input(x)
        return self._get_plan(per_op=True).embedding(x, last_fc=2)

    def get_embedding(self, x):
        return self.forward_one(x)

    def get_debug_info(self):
        return self.debug_shapes


# --------------------------------------------------------------------------------------------
# a5  ArcMarginProduct (eval)      a4  ArcFaceNet (eval)
# --------------------------------------------------------------------------------------------
class ArcMarginProduct(nn.Module):
    """`face_models.py:297-445`; only the eval-mode forward is implemented (margin = m, scale =
    min(s, 24), `:369,401-404`)."""

    def __init__(self, in_feats, out_feats, s=32.0, m=0.5, use_warm_up=True, easy_margin=False):
        super().__init__()
        self.in_feats, self.out_feats = in_feats, out_feats
        self.s, self.m, self.easy_margin = s, m, easy_margin
        self.use_warm_up = use_warm_up
        self.warm_up_epochs = 10
        self.margin_factor = 0.0
        self.scale_factor = 0.3
        self.current_epoch = 0
        self.weight = nn.Parameter(torch.empty(out_feats, in_feats))
        nn.init.xavier_normal_(self.weight, gain=math.sqrt(2))
        self.register_buffer('u', torch.zeros(1))
        self.max_cos_theta = 0.0
        self.min_cos_theta = 0.0
        self.easy_margin_used = False
        self._minmax = None

    def forward(self, input, label):
        if self.training:
            raise NotImplementedError("ArcMarginProduct: the training-mode margin schedule (face_models.py:336-348,"
                                      "404-420) is out of scope; call .eval()")
        if self.easy_margin:
            self.easy_margin_used = True
        out, mm = ops.arcmargin_eval(input.float(), self.weight.detach(), label, self.s, self.m, self.easy_margin,
                                     want_minmax=True)
        self._minmax = mm  # fetched lazily: the reference's two .item() syncs (`:358-360`) are not forced here
        return out

    def _sync_minmax(self):
        if self._minmax is not None:
            mx, mn = self._minmax.tolist()
            self.max_cos_theta, self.min_cos_theta = mx, mn
            self._minmax = None

    def update_epoch(self, epoch):
        self.current_epoch = epoch

    def get_margin_stats(self):
        self._sync_minmax()
        return {'margin_factor': self.margin_factor, 'scale_factor': self.scale_factor,
                'effective_margin': self.m * self.margin_factor, 'effective_scale': self.s * self.scale_factor,
                'max_cos_theta': self.max_cos_theta, 'min_cos_theta': self.min_cos_theta,
                'easy_margin_used': self.easy_margin_used if self.easy_margin else False}


class _PyArcFacePlan(_PerOpPlan):
    def __init__(self, m: "ArcFaceNet", dtype: torch.dtype):
        scale, shift = _bn_scale_shift(m.bn)
        super().__init__(m, None, trunk=_trunk_plan(m.backbone, dtype, m.input_mean, m.input_std, owner=m), bn_scale=scale, bn_shift=shift,
                         wt=m.embedding.weight.detach().float().t().contiguous())   # [K][N] for the fused head

    def embedding(self, x: torch.Tensor, rec=None) -> torch.Tensor:
        if _HEAD_FUSE and self["wt"].shape[1] in (256, 512):
            # avgpool + embedding + bn + F.normalize (`face_models.py:584-590`) in one launch
            f = self["trunk"].features(x, rec)
            y = ops.gap_linear_norm(f, self["wt"], self["bn_scale"], self["bn_shift"], 1e-12)[0]
            if rec is not None:
                rec("embedding+bn+normalize", y, ops.gap_linear_norm, (f,))
            return y
        f = self["trunk"].pooled(x, rec)
        pre = ops.linear_f32(f, self.m.embedding.weight.detach(), self["bn_scale"], self["bn_shift"])
        y = ops.l2_normalize(pre, 1e-12)
        if rec is not None:
            rec("embedding+bn", pre, ops.linear_f32, (f,))
            rec("normalize", y, ops.l2_normalize, (pre,))
        return y


class ArcFaceNet(_HipModule):
    """`face_models.py:447-613` (eval branch `:573-582`, ``get_embedding`` `:584-590`)."""

    def __init__(self, num_classes=18, dropout_rate=0.2, s=32.0, m=0.5, easy_margin=False):
        super().__init__()
        self.backbone = ResNet18()
        self.features = nn.Sequential(*list(self.backbone.children())[:-1])
        self.embedding = nn.Linear(512, 512, bias=False)
        self.bn = nn.BatchNorm1d(512, eps=1e-5)
        self.dropout = nn.Dropout(p=dropout_rate)
        self.arcface = ArcMarginProduct(512, num_classes, s=s, m=m, use_warm_up=True, easy_margin=easy_margin)
        self.last_grad_norm = 0.0
        self.max_grad_norm = 1.0
        self.current_epoch = 0
        self.phase = 1
        self.backbone_frozen = False
        self.val_classifier = nn.Linear(512, num_classes)
        nn.init.xavier_normal_(self.val_classifier.weight, gain=math.sqrt(2))

    def freeze_backbone(self):
        self.backbone_frozen = True
        self.phase = 1
        for param_name, param in self.named_parameters():
            if 'backbone' in param_name or 'features' in param_name:
                param.requires_grad = False

    def unfreeze_backbone(self):
        self.backbone_frozen = False
        self.phase = 2
        for param in self.parameters():
            param.requires_grad = True

    def set_max_grad_norm(self, max_norm):
        self.max_grad_norm = max_norm

    def _build_plan(self, dtype, per_op=False):
        if per_op or _PY_PLAN or not _HEAD_FUSE:
            return _PyArcFacePlan(self, dtype)
        # avgpool + embedding + bn + F.normalize (`face_models.py:584-590`): the handle's head, one launch after the trunk
        state = {f"backbone.{k}": v for k, v in self.backbone.state_dict().items()}
        state.update({"embedding.weight": self.embedding.weight, "val_classifier.weight": self.val_classifier.weight,
                      "val_classifier.bias": self.val_classifier.bias})
        state.update({f"bn.{k}": v for k, v in self.bn.state_dict().items()})
        return _TrunkPlan("arcface", state, self.val_classifier.out_features, dtype, self.input_mean, self.input_std, owner=self)

    def pooled_features(self, x):
        """fp32 ``[B, 512]``: the globally pooled trunk output, the input of ``embedding`` - what
        `head_fit.cache_features(layer="pooled")` caches so that a `head_fit.EmbedHead` can fit ``embedding``, ``bn`` and the class
        centres.  The per-op plan's ``trunk.pooled``, whatever the switches say; the model's own handle is not touched."""
        x = self._check_input(x)
        return self._get_plan(per_op=True)["trunk"].pooled(x)

    def forward(self, x, labels=None):
        if self.training:
            if labels is None:
                raise ValueError("Labels must be provided during training")
            raise NotImplementedError("ArcFaceNet: the training branch (face_models.py:527-572) is out of scope")
        emb = self.get_embedding(x)
        # `face_models.py:576`: the classifier rows are re-normalised in place on every eval call
        if self.val_classifier.weight.is_cuda:
            self.val_classifier.weight.data.copy_(ops.l2_normalize(self.val_classifier.weight.data, 1e-12))
            sig = self._signature()   # the plan does not depend on the classifier rows: no rebuild for this write
            self._plans = {k: (plan, sig) for k, (plan, _) in self._plans.items()}
        if labels is not None:
            return ops.linear_f32(emb, self.val_classifier.weight.detach(), None, self.val_classifier.bias.detach())
        return emb

    def update_epoch(self, epoch):
        self.current_epoch = epoch
        self.arcface.update_epoch(epoch)

    def get_arcface_stats(self):
        stats = self.arcface.get_margin_stats()
        stats.update(grad_norm=self.last_grad_norm, max_grad_norm=self.max_grad_norm, phase=self.phase,
                     backbone_frozen=self.backbone_frozen)
        return stats

    def get_training_phase(self):
        return {'phase': self.phase, 'backbone_frozen': self.backbone_frozen, 'epoch': self.current_epoch}


# --------------------------------------------------------------------------------------------
# a7  HybridNet (+ TransformerBlock)
# --------------------------------------------------------------------------------------------
class TransformerBlock(nn.Module):
    """`face_models.py:618-648` (parameter container)."""

    def __init__(self, embed_dim, num_heads=4, ff_dim=2048, dropout=0.1):
        super().__init__()
        self.attention = nn.MultiheadAttention(embed_dim, num_heads, dropout=dropout)
        self.norm1 = nn.LayerNorm(embed_dim)
        self.norm2 = nn.LayerNorm(embed_dim)
        self.ff = nn.Sequential(nn.Linear(embed_dim, ff_dim), nn.GELU(), nn.Dropout(dropout),
                                nn.Linear(ff_dim, embed_dim), nn.Dropout(dropout))

    def forward(self, x):
        raise RuntimeError("TransformerBlock is a parameter container; inference runs through HybridNet")


class _HybridHandlePlan(_TrunkPlan):
    def embedding(self, x: torch.Tensor) -> torch.Tensor:
        try:
            return super().embedding(x)
        except ValueError as e:   # (the handle rejects maps that are not 49 tokens with the same message)
            raise ValueError(str(e).split(": ", 1)[-1]) from None


class _PyHybridPlan(_PerOpPlan):
    def __init__(self, m: "HybridNet", dtype: torch.dtype):
        tr = m.transformer
        f32 = lambda t: t.detach().float().contiguous()
        super().__init__(
            m, m.fc, trunk=_trunk_plan(m.cnn, dtype, m.input_mean, m.input_std, owner=m), pos=f32(m.pos_encoding).view(m.seq_len, m.fdim),
            n1=(f32(tr.norm1.weight), f32(tr.norm1.bias)), n2=(f32(tr.norm2.weight), f32(tr.norm2.bias)), nf=(f32(m.norm.weight), f32(m.norm.bias)),
            qkv=_PackedLinearAsConv(tr.attention.in_proj_weight, tr.attention.in_proj_bias, None, dtype),
            proj=_PackedLinearAsConv(tr.attention.out_proj.weight, tr.attention.out_proj.bias, None, dtype),
            ff1=_PackedLinearAsConv(tr.ff[0].weight, tr.ff[0].bias, None, dtype), ff2=_PackedLinearAsConv(tr.ff[3].weight, tr.ff[3].bias, None, dtype))

    def embedding(self, x: torch.Tensor, rec=None) -> torch.Tensor:
        """`face_models.py:705-721`: trunk (no pool) → +pos → pre-LN transformer block → token mean → LN."""
        f = self["trunk"].features(x, rec)               # NHWC B×7×7×512 == tokens [B][49][512]
        B, Hh, Ww, D = f.shape
        L = Hh * Ww
        if L != self.m.seq_len:
            raise ValueError(f"HybridNet expects a {self.m.seq_len}-token feature map (224×224 input), got {L}")
        t, n1 = ops.add_pos_layernorm(f.view(B, L, D), self["pos"], *self["n1"], want_sum=True)
        qkv = self["qkv"](n1.view(B * L, D), relu=0)
        att = ops.mha_tokens(qkv.view(B, L, 3 * D), self.m.transformer.attention.num_heads)
        t2 = self["proj"](att.view(B * L, D), relu=0, residual=t.view(B * L, D))          # x + attn_out
        _, n2 = ops.add_pos_layernorm(t2.view(B, L, D), None, *self["n2"])
        hdn = self["ff1"](n2.view(B * L, D), relu=2)                                       # Linear → GELU
        t3 = self["ff2"](hdn, relu=0, residual=t2)                                          # x + ff_out
        y = ops.mean_layernorm(t3.view(B, L, D), *self["nf"])
        if rec is not None:
            for step in (("tokens+pos", t, ops.add_pos_layernorm, (f,)), ("norm1", n1, ops.add_pos_layernorm, (f,)),
                         ("in_proj", qkv, self["qkv"], (n1.view(B * L, D),)), ("mha", att, ops.mha_tokens, (qkv,)),
                         ("out_proj+res", t2, self["proj"], (att.view(B * L, D), t)), ("norm2", n2, ops.add_pos_layernorm, (t2,)),
                         ("ff.0+gelu", hdn, self["ff1"], (n2.view(B * L, D),)), ("ff.3+res", t3, self["ff2"], (hdn, t2)),
                         ("mean+norm", y, ops.mean_layernorm, (t3,))):
                rec(*step)
        return y


class HybridNet(_HipModule):
    """`face_models.py:650-721`."""

    def __init__(self, num_classes=18):
        super().__init__()
        self.cnn = ResNet18()
        self.features = nn.Sequential(*list(self.cnn.children())[:-2])
        self.fdim = 512
        self.seq_len = 49
        self.pos_encoding = nn.Parameter(torch.zeros(self.seq_len, 1, self.fdim))
        nn.init.normal_(self.pos_encoding, mean=0, std=0.02)
        self.transformer = TransformerBlock(self.fdim)
        self.dropout = nn.Dropout(0.1)
        self.norm = nn.LayerNorm(self.fdim)
        self.fc = nn.Linear(self.fdim, num_classes)

    def _build_plan(self, dtype, per_op=False):
        if per_op or _PY_PLAN:
            return _PyHybridPlan(self, dtype)
        return _HybridHandlePlan("hybrid", dict(self.state_dict()), self.fc.out_features, dtype, self.input_mean, self.input_std, owner=self)

    def forward(self, x):
        return self._get_plan().logits(self._check_input(x))


# --------------------------------------------------------------------------------------------
# §8(f) AttentionNet (face_models.py:194-295) and EnsembleModel (face_models.py:843-959)
# --------------------------------------------------------------------------------------------
class SpatialAttention(nn.Module):
    """Parameter container, `face_models.py:194-211` (the gate itself runs inside ``frmap_cnn_attention``)."""

    def __init__(self, kernel_size=7):
        super().__init__()
        self.conv = nn.Conv2d(2, 1, kernel_size=kernel_size, padding=kernel_size // 2)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        raise RuntimeError("SpatialAttention is a parameter container here; run AttentionNet on the GPU")


class AttentionModule(nn.Module):
    """Parameter container, `face_models.py:213-262`."""

    def __init__(self, in_channels, reduction_ratio=8):
        super().__init__()
        self.query = nn.Conv2d(in_channels, in_channels // reduction_ratio, kernel_size=1)
        self.key = nn.Conv2d(in_channels, in_channels // reduction_ratio, kernel_size=1)
        self.value = nn.Conv2d(in_channels, in_channels, kernel_size=1)
        self.gamma = nn.Parameter(torch.zeros(1))
        self.gamma_value = 0.0
        self.num_heads = 2
        self.head_dim = in_channels // (reduction_ratio * self.num_heads)
        self.spatial_attention = SpatialAttention()

    def forward(self, x):
        raise RuntimeError("AttentionModule is a parameter container here; run AttentionNet on the GPU")


class _PyAttentionPlan(_PerOpPlan):
    def __init__(self, m: "AttentionNet", dtype: torch.dtype):
        a = m.attention
        w = torch.cat([a.query.weight, a.key.weight, a.value.weight], dim=0).detach().float()
        bias = torch.cat([a.query.bias, a.key.bias, a.value.bias], dim=0).detach().float()
        super().__init__(m, m.fc, trunk=_trunk_plan(m.backbone, dtype, m.input_mean, m.input_std, owner=m),
                         qkv=ops.pack_conv_weight(w.contiguous(), dtype), qkv_bias=bias.contiguous(), cq=a.query.weight.shape[0], cqkv=w.shape[0],
                         gamma=a.gamma.detach().float().contiguous(), sw=a.spatial_attention.conv.weight.detach().float().contiguous(),
                         sb=a.spatial_attention.conv.bias.detach().float().contiguous())

    def attend(self, x: torch.Tensor, want_map: bool, rec=None):
        """-> (the attended map or None, its global average pool)."""
        f = self["trunk"].features(x, rec)                                                    # NHWC B×H×W×512
        qkv = ops.conv_igemm(f, self["qkv"], self["qkv_bias"], self["cqkv"], 1, 1, 0, 0)        # q | k | v  (+bias)
        out = ops.cnn_attention(qkv, f, self["gamma"], self["sw"], self["sb"], self["cq"], want_map=want_map, want_pool=True)
        if rec is not None:
            rec("attention.qkv", qkv, ops.conv_igemm, (f,))
            rec("attention.pool", out[1], ops.cnn_attention, (qkv, f))
        return out

    def embedding(self, x: torch.Tensor, rec=None) -> torch.Tensor:
        return self.attend(x, False, rec)[1]


class AttentionNet(_HipModule):
    """`face_models.py:264-295`: ResNet-18 trunk (no pool) → AttentionModule → global average pool → fc.
    q/k/v are ONE 1x1 conv (the three weight matrices stacked along Cout, biases as its shift); everything after it
    up to and including the pooling is ``frmap_cnn_attention``."""

    def __init__(self, num_classes=18, dropout_rate=0.25):
        super().__init__()
        self.backbone = ResNet18()
        self.features = nn.Sequential(*list(self.backbone.children())[:-2])
        self.attention = AttentionModule(512)
        self.gap = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(512, num_classes)

    def _build_plan(self, dtype, per_op=False):   # (no 'attention' handle family: the trunk on a handle, the head per-op)
        return _PyAttentionPlan(self, dtype)

    def forward(self, x):
        """`face_models.py:276-282` (``get_embedding``: `:284-288`)."""
        x = self._check_input(x)
        return self._get_plan().logits(x)

    def attention_map(self, x):
        """The attended map the module hands to the pooling, NCHW-logical (stored NHWC): B×H×W×512."""
        x = self._check_input(x)
        return self._get_plan().attend(x, True)[0]

    def get_attention_params(self):
        self.attention.gamma_value = float(self.attention.gamma.detach().cpu().item())
        return {"gamma": self.attention.gamma_value}


class EnsembleModel(nn.Module):
    """`face_models.py:843-941`: runs every member on the GPU and merges their logits on the device.
    ArcFace members contribute cosine logits against their class centres (`:889-893`), Siamese members are
    skipped (`:894-897`); 'average' / 'weighted' / 'max' as in the reference, anything else raises ValueError
    at call time (`:919-920` — the constructor accepts 'attention' but ``forward`` has no branch for it)."""

    def __init__(self, models, ensemble_method: str = 'weighted'):
        super().__init__()
        self.models = nn.ModuleList(models)
        self.ensemble_method = ensemble_method
        self.weights = nn.Parameter(torch.ones(len(models)) / len(models),
                                    requires_grad=(ensemble_method in ['weighted', 'attention']))
        if ensemble_method == 'attention':
            self.attention_net = nn.Sequential(nn.Linear(len(models), 64), nn.ReLU(inplace=True),
                                               nn.Linear(64, len(models)), nn.Softmax(dim=0))

    def forward(self, x):
        outputs = []
        for model in self.models:
            if hasattr(model, 'training') and model.training:
                model.eval()
            if isinstance(model, ArcFaceNet):
                emb = model(x)                                                            # unit-norm embedding
                outputs.append(ops.cosine_logits(emb, model.arcface.weight.detach().float(), want_argmax=False)[0])
            elif isinstance(model, SiameseNet):
                continue
            else:
                outputs.append(model(x))
        if len(outputs) == 1:
            return outputs[0]
        if self.ensemble_method == 'average':
            return torch.mean(torch.stack(outputs), dim=0)
        elif self.ensemble_method == 'weighted':
            w = torch.softmax(self.weights.detach().float(), dim=0)
            return torch.sum(torch.stack([w[i] * outputs[i] for i in range(len(outputs))]), dim=0)
        elif self.ensemble_method == 'max':
            probs = [torch.softmax(o, dim=1) for o in outputs]
            return torch.log(torch.max(torch.stack(probs), dim=0)[0])
        raise ValueError(f"Unknown ensemble method: {self.ensemble_method}")

    def get_embedding(self, x):
        """`face_models.py:922-941`: the members' embeddings concatenated along the feature axis."""
        embs = [m.get_embedding(x) for m in self.models if hasattr(m, 'get_embedding')]
        embs = [e.unsqueeze(0) if e.dim() == 1 else e for e in embs]
        if len(embs) > 1:
            return torch.cat(embs, dim=1)
        return embs[0] if embs else None


def create_ensemble(model_types, num_classes: int, ensemble_method: str = 'average') -> EnsembleModel:
    """`face_models.py:943-959`."""
    return EnsembleModel([get_model(t, num_classes=num_classes) for t in model_types], ensemble_method=ensemble_method)


# --------------------------------------------------------------------------------------------
# a1  factory
# --------------------------------------------------------------------------------------------
def get_model(model_type: str, num_classes: int = 18, input_size: Tuple[int, int] = (224, 224)) -> nn.Module:
    """`face_models.py:785-813`: same type strings; unknown → ``ValueError``.  Returns a train-mode
    module on the CPU with fp32 parameters, as the reference does; ``.to('cuda').eval()`` before
    inference."""
    if model_type == 'baseline':
        return BaselineNet(num_classes=num_classes, input_size=input_size)
    elif model_type == 'cnn':
        return ResNetTransfer(num_classes=num_classes, freeze_backbone=False)
    elif model_type == 'siamese':
        return SiameseNet()
    elif model_type == 'arcface':
        return ArcFaceNet(num_classes=num_classes, dropout_rate=0.2)
    elif model_type == 'hybrid':
        return HybridNet(num_classes=num_classes)
    elif model_type == 'attention':
        return AttentionNet(num_classes=num_classes, dropout_rate=0.25)
    elif model_type == 'ensemble':
        return create_ensemble(['cnn', 'attention', 'arcface'], num_classes=num_classes)
    elif isinstance(model_type, list):
        return create_ensemble(model_type, num_classes=num_classes)
    else:
        raise ValueError(f"Invalid model type: {model_type}")
