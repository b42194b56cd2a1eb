"""What every wrapper of `ops` does with the tensors it is handed: helpers of `test_operands_cpu.py` and `test_operands_gpu.py`.

A plain helper module like `guard.py` and `place_cases.py` (no fixture, no setting).  Four things live here.

THE TABLE (`ROWS`).  One `Row` per public callable of `ops` that takes a tensor: the smallest valid call (the shapes of that
wrapper's case in `test_guard_ops_gpu.py` / `test_guard_conv_gpu.py` / `place_cases.REJECT_CALLS`, or smaller), the names of its tensor
operands, which of them the call WRITES, and for every DEPENDENT operand - one whose extent the library takes from another operand's
shape or from a scalar argument, so that the library cannot see how long it really is - the `Rule` its shape must meet.  Every other
tensor operand is FREE: the call's extents are read from its own shape and handed to the library, which refuses what it cannot take.
`Row.own` lists extents the library itself receives and refuses ("library's own"), each with the `FRMAP_REQUIRE` that does it
(source file, a fragment of the line); such an extent may reach the library and is not a case here.
`census()` asserts that the table covers every public tensor-taking callable of `ops` and classifies every tensor parameter.

DEFECTS (`defects`).  For a dependent operand, one bad tensor per defect: too short by one along each ruled axis, too long by one,
wrong rank (same elements), wrong dtype, and on the CPU; with the exception the wrapper owes (`_dev`'s convention: ValueError for a
shape, TypeError for a dtype, RuntimeError for a CPU tensor).

THE STUB (`StubLibrary`, `install`).  Stands in for the library behind `_lib.load`: entry points that take no pointer (found from
`_lib.PROTOTYPES`: sizes, `*_supported`, `frmap_last_error`, ...) go to the real library; every other entry point records its name
and arguments and raises `ReachedLibrary`.  Nothing is ever launched through it: a wrapper that fails to refuse a bad operand is
reported, never run out of bounds.

STRIDED PLACEMENT (`strided_view`, `expanded_view`, `permuted_view`).  An operand as a view the binding has to copy.
"""
import collections
import ctypes
import inspect
import os
import re

import torch

from frmap_amd import _lib, ops

F16 = torch.float16
CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")


# ---------------------------------------------------------------------------------------------------------------------------------
# strided placement
# ---------------------------------------------------------------------------------------------------------------------------------
def _poisoned(shape, dtype, device):
    """An uninitialised-looking buffer: every byte 0x5A, so an element the view skips is never a plausible neighbour."""
    t = torch.empty(shape, dtype=dtype, device=device)
    if t.numel():
        t.view(-1).view(torch.uint8).fill_(0x5A)
    return t


def strided_view(t_cpu, device="cuda"):
    """`t_cpu` on the device as `wide[..., ::2]` of a tensor twice as wide in the last axis (stride 2 for a 1-D operand): the same
    values, starting where the allocation starts (so aligned), and not contiguous.  Empty, 0-d and one-element tensors are plain copies."""
    t = t_cpu.detach()
    if t.dim() == 0 or t.numel() == 0:
        return t.to(device, copy=True)
    wide = _poisoned(tuple(t.shape[:-1]) + (2 * t.shape[-1],), t.dtype, device)
    v = wide[..., ::2]
    v.copy_(t)
    assert tuple(v.shape) == tuple(t.shape) and v.data_ptr() == wide.data_ptr()
    if v.is_contiguous():               # (one element, or [1, .., 1, n] of n = 1: torch ignores the stride of an axis of size 1)
        return t.to(device, copy=True)
    return v


def expanded_view(t_cpu, device="cuda"):
    """`t_cpu` on the device as a stride-0 `expand` along the first axis over which its values are constant (a per-channel vector of
    one repeated value from a one-element source, a `pos` of one repeated row from a one-row source); None where the values do not
    allow it."""
    t = t_cpu.detach()
    for ax in range(t.dim()):
        if t.shape[ax] > 1 and bool((t == t.narrow(ax, 0, 1)).all()):
            v = t.narrow(ax, 0, 1).to(device, copy=True).expand(t.shape)
            assert v.stride(ax) == 0 and not v.is_contiguous()
            return v
    return None


def permuted_view(t_cpu, device="cuda"):
    """A 4-D `t_cpu` [B, H, W, C] on the device as the `permute(0, 2, 3, 1)` view of a standard contiguous [B, C, H, W] tensor: the
    NHWC map a torch user has in hand."""
    t = t_cpu.detach()
    assert t.dim() == 4
    base = _poisoned((t.shape[0], t.shape[3], t.shape[1], t.shape[2]), t.dtype, device)
    v = base.permute(0, 2, 3, 1)
    v.copy_(t)
    assert tuple(v.shape) == tuple(t.shape) and base.is_contiguous()
    return t.to(device, copy=True) if v.is_contiguous() else v          # (H = W = 1: the same memory either way)


# ---------------------------------------------------------------------------------------------------------------------------------
# the stub
# ---------------------------------------------------------------------------------------------------------------------------------
class ReachedLibrary(Exception):
    """A wrapper got as far as an entry point that takes pointers."""

    def __init__(self, entry, args):
        super().__init__("reached %s" % entry)
        self.entry, self.args_ = entry, args


def _is_pointer(ctype):
    return ctype in (ctypes.c_void_p, ctypes.c_char_p, ctypes.c_wchar_p) or (inspect.isclass(ctype) and issubclass(ctype, ctypes._Pointer))


def pointer_free():
    """The entry points that take no pointer argument, from `_lib.PROTOTYPES` (sizes, capability queries, the error text, tuning
    hooks): all a wrapper can learn from the library without handing it memory."""
    return sorted(name for name, (_, args) in _lib.PROTOTYPES.items() if not any(_is_pointer(a) for a in args))


class StubLibrary:
    def __init__(self, real):
        self._real, self._free, self.calls = real, set(pointer_free()), []

    def __getattr__(self, name):
        if name not in _lib.PROTOTYPES:
            raise AttributeError(name)
        if name in self._free:
            return getattr(self._real, name)

        def reached(*args):
            self.calls.append((name, args))
            raise ReachedLibrary(name, args)
        reached.__name__ = name
        return reached


def install(monkeypatch):
    """Put a `StubLibrary` behind `_lib.load` with the stock `monkeypatch` fixture (undone when the test ends) and return it."""
    stub = StubLibrary(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: stub)
    return stub


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------
class Rule:
    """The shape a dependent operand must have IS the shape it has in the row's valid call; `text` says where the library takes it
    from.  `axes`: the axes whose extent is the dependent one (a defect is made along each).  `at_least`: the wrapper's contract is
    "at least this many" (a state buffer: `ops.track_state` itself rounds up), so one element too many is no defect."""

    def __init__(self, text, axes=(-1,), at_least=False):
        self.text, self.axes, self.at_least = text, tuple(axes), at_least


class Row:
    def __init__(self, name, build, free=(), dependent=None, writes=(), own=None, extra=()):
        self.name, self.build, self.free, self.dependent, self.writes = name, build, tuple(free), dict(dependent or {}), tuple(writes)
        self.own, self.extra = dict(own or {}), tuple(extra)

    @property
    def tensors(self):
        return self.free + tuple(self.dependent)

    def target(self):
        return getattr(ops, self.name)

    def signature(self):
        fn = self.target()
        return inspect.signature(getattr(fn, "__wrapped__", fn))


def _r(seed, *shape, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


def _i32(*values):
    return torch.tensor(values, dtype=torch.int32)


def _kpad(k):
    return int(_lib.load().frmap_small_cin_kpad(k, k))


def _od(**kw):
    return collections.OrderedDict(kw)


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_SHIFT = Rule("[Cout] from the scalar Cout")
_WPK = Rule("a flat packed weight of Cout * Cin * k * k elements (pack_conv_weight) in the activations' dtype")
_WPK3 = Rule("a flat packed weight of Cout * frmap_small_cin_kpad(k, k) elements (pack_conv_weight_c3) in the compute dtype")
_OUT = Rule("the output's shape [B, Ho, Wo, Cout]")
_LABELS = Rule("one label per row of the matrix it labels", axes=(0,))
_GALLERY = Rule("[G, D] with the probes' D", axes=(1,))
_PACKED = Rule("int32 [B, 2], one record per probe", axes=(0, 1))
_REQ_TOP1 = ("head_match.hip", '"match_top1: bad shape B=%d G=%d D=%d"')
_REQ_MATCH_D = {"D % 4 (emb)": _REQ_TOP1}


def _track_step_call():
    S, M = 2, 3
    boxes = torch.zeros((S, M, 4))
    boxes[:, 0] = torch.tensor([10.0, 12.0, 50.0, 60.0])
    return _od(state=torch.zeros((ops.track_state_bytes(S, M),), dtype=torch.uint8), boxes=boxes, probs=torch.full((S, M), 0.99),
               counts=_i32(1, 1), frame_hw=_i32([240, 320], [240, 320]))


def _track_fuse_call():
    S, M, D = 2, 3, 8
    return _od(state=torch.zeros((ops.track_fuse_state_bytes(S, M, D),), dtype=torch.uint8), ids=_i32([0, -1, -1], [0, -1, -1]),
               counts=_i32(1, 1), emb=_r(71, 2, D), rows=_i32([0, 0], [1, 0]), decay=0.9)


def _tally_call():
    return _od(logits=_r(72, 3, 5), labels=_i32(0, 4, 2), state=torch.zeros((ops.classify_tally_words(5, 6, 10, True),), dtype=torch.int64))


ROWS = [
    Row("pack_input", lambda: _od(x=_r(1, 2, 3, 6, 5), dtype=F16), free=["x"]),
    Row("pack_conv_weight", lambda: _od(w_folded=_r(2, 64, 32, 1, 1), dtype=F16), free=["w_folded"]),
    Row("pack_conv_weight_c3", lambda: _od(w_folded=_r(3, 32, 3, 3, 3), dtype=F16), free=["w_folded"]),
    Row("conv_small_cin", lambda: _od(x4=_r(4, 1, 8, 8, 4, dtype=F16), wpk=_r(5, 32 * _kpad(3), dtype=F16), shift=_r(6, 32), Cout=32, k=3,
                                      stride=1, pad=1, relu=True),
        free=["x4"], dependent={"wpk": _WPK3, "shift": _SHIFT}),
    Row("conv_small_cin_pool2", lambda: _od(x4=_r(4, 1, 8, 8, 4, dtype=F16), wpk=_r(5, 32 * _kpad(3), dtype=F16), shift=_r(6, 32), Cout=32,
                                            relu=True),
        free=["x4"], dependent={"wpk": _WPK3, "shift": _SHIFT}),
    Row("stem7x7_maxpool", lambda: _od(x=_r(7, 1, 3, 8, 8), wpk=_r(8, 64 * _kpad(7), dtype=F16) * 0.1, shift=_r(9, 64), dtype=F16),
        free=["x"], dependent={"wpk": _WPK3, "shift": _SHIFT}),
    Row("stem7x7_maxpool_u8", lambda: _od(x_u8=(_r(10, 1, 8, 8, 3).abs() * 60).clamp(0, 255).to(torch.uint8),
                                          wpk=_r(8, 64 * _kpad(7), dtype=F16) * 0.1, shift=_r(9, 64), mean=MEAN, std=STD, dtype=F16),
        free=["x_u8"], dependent={"wpk": _WPK3, "shift": _SHIFT}),
    Row("conv_igemm", lambda: _od(x=_r(11, 1, 2, 2, 32, dtype=F16), wpk=_r(12, 64 * 32 * 9, dtype=F16) * 0.1, shift=_r(13, 64), Cout=64, k=3,
                                  stride=1, pad=1, relu=True, residual=_r(14, 1, 2, 2, 64, dtype=F16)),
        free=["x"], dependent={"wpk": _WPK, "shift": _SHIFT, "residual": _OUT},
        own={"Cin % 32": ("conv_igemm.hip", '"conv_igemm: Cin=%d must be a multiple of 32"')}),
    Row("conv_igemm_pool2", lambda: _od(x=_r(11, 1, 2, 2, 32, dtype=F16), wpk=_r(12, 64 * 32 * 9, dtype=F16) * 0.1, shift=_r(13, 64), Cout=64,
                                        relu=True),
        free=["x"], dependent={"wpk": _WPK, "shift": _SHIFT}),
    Row("conv_igemm_ds", lambda: _od(x=_r(15, 1, 2, 2, 64, dtype=F16), wpk=_r(16, 64 * 64 * 9, dtype=F16) * 0.1, shift=_r(13, 64), Cout=64,
                                     x_ds=_r(17, 1, 4, 4, 32, dtype=F16), wpk_ds=_r(18, 64 * 32, dtype=F16) * 0.1, ds_stride=2, relu=True),
        free=["x"], dependent={"wpk": _WPK, "shift": _SHIFT, "x_ds": Rule("x's batch (its H, W, C go to the library)", axes=(0,)),
                               "wpk_ds": Rule("a flat packed 1x1 weight of Cout * x_ds's channels")}),
    Row("linear_mfma", lambda: _od(x2d=_r(19, 1, 32, dtype=F16), wpk=_r(20, 64 * 32, dtype=F16) * 0.1, shift=_r(21, 64), N=64, act=0,
                                   residual=_r(22, 1, 64, dtype=F16)),
        free=["x2d"], dependent={"wpk": Rule("a flat packed weight of N * K elements"), "shift": Rule("[N] from the scalar N"),
                                 "residual": Rule("the output's shape [M, N]")},
        own={"K % 32, N % 64": ("conv_igemm.hip", '"linear_mfma: need K %% 32 == 0 and N %% 64 == 0')}),
    Row("maxpool", lambda: _od(x=_r(23, 1, 2, 2, 8, dtype=F16), k=2, stride=2, pad=0), free=["x"]),
    Row("avgpool_global", lambda: _od(x=_r(24, 1, 1, 1, 8, dtype=F16)), free=["x"]),
    Row("avgpool_adaptive", lambda: _od(x=_r(25, 1, 2, 2, 8, dtype=F16), OH=1, OW=1), free=["x"]),
    Row("linear_f32", lambda: _od(x=_r(26, 2, 4), w=_r(27, 3, 4), scale=_r(28, 3).abs() + 0.5, shift=_r(29, 3), relu=True),
        free=["x"], dependent={"w": Rule("[N, K] with x's K", axes=(1,)), "scale": Rule("[N] from w's rows"), "shift": Rule("[N] from w's rows")},
        own={"K % 4": ("head_match.hip", '"linear_f32: bad shape B=%d K=%d N=%d (K %% 4 == 0)"')}),
    Row("l2_normalize", lambda: _od(x=_r(30, 2, 4)), free=["x"]),
    Row("cast_to_f32", lambda: _od(x=_r(31, 5, dtype=F16)), free=["x"]),
    Row("cast_from_f32", lambda: _od(x=_r(32, 5), dtype=F16), free=["x"]),
    Row("add_pos_layernorm", lambda: _od(x=_r(33, 2, 5, 64, dtype=F16), pos=_r(34, 5, 64) * 0.1, gamma=_r(35, 64).abs() + 0.5,
                                         beta=_r(36, 64) * 0.1, want_sum=True),
        free=["x"], dependent={"pos": Rule("[L, D] of x [B, L, D]", axes=(0, 1)), "gamma": Rule("[D] of x"), "beta": Rule("[D] of x")},
        own={"D % 64, D <= 1024": ("transformer.hip", '"add_pos_layernorm: bad shape (D %% 64 == 0, D <= 1024)"')}),
    Row("mha_tokens", lambda: _od(qkv=_r(37, 1, 1, 384, dtype=F16), H=1), free=["qkv"],
        own={"D % H (D == 128 H)": ("transformer.hip", '"mha_tokens: need L <= 64 and head dim 128 (D=%d H=%d L=%d)"')},
        extra=[("qkv-last-axis-not-3D", "qkv", lambda t: torch.cat([t, t[..., :1]], dim=-1), ValueError),
               ("qkv-wrong-rank", "qkv", lambda t: t.reshape(1, -1), ValueError)]),
    Row("mean_layernorm", lambda: _od(t=_r(38, 2, 5, 64, dtype=F16), gamma=_r(35, 64).abs() + 0.5, beta=_r(36, 64) * 0.1),
        free=["t"], dependent={"gamma": Rule("[D] of t [B, L, D]"), "beta": Rule("[D] of t")},
        own={"D <= 1024": ("transformer.hip", '"mean_layernorm: bad shape (D <= 1024)"')}),
    Row("cnn_attention", lambda: _od(qkv=_r(39, 1, 1, 1, 2 * 8 + 256, dtype=F16), x=_r(40, 1, 1, 1, 256, dtype=F16), gamma=torch.tensor([0.7]),
                                     spatial_w=_r(41, 1, 2, 1, 1), spatial_b=torch.tensor([-0.3]), Cq=8, want_map=True, want_pool=True),
        free=["x", "spatial_w"],
        dependent={"qkv": Rule("[B, H, W, 2 Cq + C] of x [B, H, W, C] and the scalar Cq"), "gamma": Rule("one value: [1]"),
                   "spatial_b": Rule("one value: [1]")},
        own={"C in (256, 512)": ("transformer.hip", '"cnn_attention: C=%d must be 256 or 512"'),
             "KS odd, <= 15": ("transformer.hip", '"cnn_attention: odd spatial kernel size <= 15 expected (got %d)"')}),
    Row("normalize_u8", lambda: _od(img=(_r(42, 2, 7, 5, 3).abs() * 60).clamp(0, 255).to(torch.uint8), mean=MEAN, std=STD, want_nchw=True,
                                    nhwc4_dtype=F16), free=["img"]),
    Row("softmax_argmax", lambda: _od(logits=_r(43, 2, 3)), free=["logits"]),
    Row("pairwise_distance", lambda: _od(a=_r(44, 2, 4), b=_r(45, 2, 4), thresh=2.0), free=["a"],
        dependent={"b": Rule("a's shape [B, D]", axes=(0, 1))}),
    Row("classify_tally", lambda: dict(_tally_call(), ranks=6, n_bins=10, confusion=True, want_rows=True), free=["logits"],
        dependent={"labels": Rule("[B] of logits [B, C]", axes=(0,)),
                   "state": Rule("classify_tally_words(C, ranks, n_bins, confusion) words", axes=(0,))}, writes=["state"]),
    Row("ovr_append", lambda: _od(scores=_r(46, 2, 3), labels=_i32(0, 2), store=torch.zeros((3, 4)), store_labels=torch.full((4,), -1, dtype=torch.int32),
                                  first=1),
        free=["store"], dependent={"scores": Rule("[B, C] with the store's C", axes=(1,)), "labels": Rule("[B] of scores", axes=(0,)),
                                   "store_labels": Rule("[capacity] of store [C, capacity]", axes=(0,))},
        writes=["store", "store_labels"]),
    Row("ovr_rank_counts", lambda: _od(store=_r(47, 3, 4), store_labels=_i32(0, 2, 1, 0), n=4), free=["store"],
        dependent={"store_labels": Rule("[capacity] of store [C, capacity]", axes=(0,))}),
    Row("MatchPack", lambda: _od(gallery=_r(48, 7, 64)), free=["gallery"]),
    Row("match_prepare", lambda: _od(gallery=_r(48, 7, 64)), free=["gallery"]),
    Row("match_top1", lambda: _od(emb=_r(49, 2, 64), gallery=_r(48, 7, 64), thresh=9.0, packed=torch.full((2, 2), -7, dtype=torch.int32)),
        free=["emb"], dependent={"gallery": _GALLERY, "packed": _PACKED}, writes=["packed"], own=_REQ_MATCH_D,
        extra=[("emb-wrong-rank", "emb", lambda t: t.reshape(-1), ValueError)]),
    Row("match_topk", lambda: _od(emb=_r(49, 2, 64), gallery=_r(48, 7, 64), k=2, labels=_i32(0, 1, 2, 0, 1, 2, 3)),
        free=["emb"], dependent={"gallery": _GALLERY, "labels": Rule("[G] of gallery [G, D]", axes=(0,))}),
    Row("verify_counts", lambda: _od(a=_r(50, 2, 64), labels_a=_i32(0, 1), thresholds=torch.tensor([0.5, 9.0, 12.0]), b=_r(48, 7, 64),
                                     labels_b=_i32(0, 1, 2, 0, 1, 2, 3)),
        free=["a", "thresholds"], dependent={"labels_a": _LABELS, "b": Rule("[Q, D] with a's D", axes=(1,)), "labels_b": _LABELS}),
    Row("match_radius", lambda: _od(a=_r(50, 2, 64), thresh=11.0, b=_r(48, 7, 64), labels_a=_i32(0, 1), labels_b=_i32(0, 1, 2, 0, 1, 2, 3),
                                    which="same"),
        free=["a"], dependent={"labels_a": _LABELS, "b": Rule("[Q, D] with a's D", axes=(1,)), "labels_b": _LABELS}),
    Row("gap_linear_norm", lambda: _od(fmap=_r(51, 1, 1, 1, 8, dtype=F16), wt=_r(52, 8, 256), scale=_r(53, 256).abs() + 0.5, shift=_r(54, 256),
                                       want_pre=True),
        free=["fmap"], dependent={"wt": Rule("[K, N] with the map's K channels", axes=(0,)), "scale": Rule("[N] of wt"), "shift": Rule("[N] of wt")},
        own={"N in (256, 512)": ("head_match.hip", '"gap_linear_norm: N=%d not supported (256 or 512)"')}),
    Row("gap_norm_match", lambda: _od(fmap=_r(55, 2, 1, 1, 8, dtype=F16), gallery=_r(56, 3, 8), thresh=9.0, normalize=True, want_emb=True,
                                      packed=torch.full((2, 2), -7, dtype=torch.int32)),
        free=["fmap"], dependent={"gallery": Rule("[G, C] with the map's C channels", axes=(1,)), "packed": _PACKED}, writes=["packed"],
        own={"G <= 64": ("head_match.hip", '"gap_norm_match: gallery of 0..64 rows expected (got %d)"')}),
    Row("cosine_logits", lambda: _od(x=_r(57, 2, 4), w=_r(58, 3, 4), s=32.0), free=["x"], dependent={"w": Rule("[C, D] with x's D", axes=(1,))},
        own={"D % 4": ("head_match.hip", '"cosine_logits: bad shape"')}),
    Row("arcmargin_eval", lambda: _od(x=_r(57, 2, 4), w=_r(58, 3, 4), label=torch.tensor([2, 0], dtype=torch.int64), s=30.0, m=0.5,
                                      want_minmax=True),
        free=["x"], dependent={"w": Rule("[C, D] with x's D", axes=(1,)), "label": Rule("[B] of x [B, D]", axes=(0,))},
        own={"D % 4": ("head_match.hip", '"arcmargin_eval: bad shape"')}),
    Row("track_step", _track_step_call, free=["boxes"],
        dependent={"state": Rule("at least track_state_bytes(S, max_boxes) bytes", axes=(0,), at_least=True),
                   "probs": Rule("[S, max_boxes] of boxes", axes=(0, 1)), "counts": Rule("[S] of boxes", axes=(0,)),
                   "frame_hw": Rule("[S, 2] of boxes", axes=(0, 1))}, writes=["state"]),
    Row("track_fuse", _track_fuse_call, free=["ids", "emb"],
        dependent={"state": Rule("at least track_fuse_state_bytes(S, max_boxes, D) bytes", axes=(0,), at_least=True),
                   "counts": Rule("[S] of ids [S, max_boxes]", axes=(0,)), "rows": Rule("[N, 2] of emb [N, D]", axes=(0, 1))},
        writes=["state"]),
]
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)


def tensor_callables():
    """name -> the annotated tensor parameters of every public callable defined in `ops` that has one."""
    out = {}
    for name, obj in sorted(vars(ops).items()):
        if name.startswith("_") or not callable(obj) or getattr(obj, "__module__", None) != ops.__name__:
            continue
        try:
            sig = inspect.signature(getattr(obj, "__wrapped__", obj))
        except (TypeError, ValueError):
            continue
        params = [p.name for p in sig.parameters.values() if "torch.Tensor" in str(p.annotation)]
        if params:
            out[name] = params
    return out


def census():
    """The table covers every public tensor-taking callable of `ops`; every tensor parameter of every row is classified (free or
    dependent, never both), what a row writes is one of its tensors, and its valid call binds to the signature."""
    found = tensor_callables()
    assert sorted(found) == sorted(BY_NAME), ("wrappers without a row", sorted(set(found) - set(BY_NAME)), "rows without a wrapper",
                                              sorted(set(BY_NAME) - set(found)))
    for row in ROWS:
        params = list(row.signature().parameters)
        assert not set(row.free) & set(row.dependent), (row.name, "free and dependent")
        assert set(found[row.name]) <= set(row.tensors), (row.name, "unclassified tensor parameters", sorted(set(found[row.name]) - set(row.tensors)))
        assert set(row.tensors) <= set(params), (row.name, "operands that are no parameter", sorted(set(row.tensors) - set(params)))
        assert set(row.writes) <= set(row.tensors), (row.name, row.writes)
        for _, operand, _, exc in row.extra:
            assert operand in row.tensors and issubclass(exc, Exception), (row.name, operand)
    return found


def own_citations():
    """[(wrapper, extent, file, fragment)] of every "library's own" extent of the table."""
    return [(row.name, extent, f, frag) for row in ROWS for extent, (f, frag) in sorted(row.own.items())]


def citation_line(file, fragment):
    """The line of csrc/`file` that holds `fragment`, or None."""
    with open(os.path.join(CSRC, file)) as fh:
        for line in fh:
            if fragment in line:
                return line
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# calls and defects
# ---------------------------------------------------------------------------------------------------------------------------------
def invoke(row, values, place):
    """The row's call: tensors of `values` moved by `place` (CPU tensor -> device tensor; a tensor already on a device is passed as it
    is), parameters without a default passed by position, the others by keyword."""
    args, kwargs = [], {}
    for name, p in row.signature().parameters.items():
        if name not in values:
            continue
        v = values[name]
        if isinstance(v, _OnCpu):
            v = v.t
        elif isinstance(v, torch.Tensor) and v.device.type == "cpu":
            v = place(v)
        if p.default is inspect.Parameter.empty:
            args.append(v)
        else:
            kwargs[name] = v
    return row.target()(*args, **kwargs)


class _OnCpu:
    """Marks the one operand of a case that is meant to reach the wrapper as a CPU tensor."""

    def __init__(self, t):
        self.t = t


def wrong_dtype(dtype):
    return torch.float64 if dtype == torch.float32 else torch.float32


def defects(row, operand, valid):
    """[(label, bad tensor (CPU; `_OnCpu` for the one that stays there), exception)] for a dependent operand of `row`."""
    rule, out = row.dependent[operand], []
    for ax in rule.axes:
        tag = "" if len(rule.axes) == 1 else "-axis%d" % ax
        ax = ax % valid.dim()
        n = valid.shape[ax]
        out.append(("short" + tag, valid.narrow(ax, 0, n - 1).contiguous(), ValueError))
        if not rule.at_least:
            out.append(("long" + tag, torch.cat([valid, valid.narrow(ax, 0, 1)], dim=ax).contiguous(), ValueError))
    out.append(("rank", valid[None].contiguous() if valid.dim() == 1 else valid.reshape(-1).contiguous(), ValueError))
    out.append(("dtype", valid.to(wrong_dtype(valid.dtype)), TypeError))
    out.append(("cpu", _OnCpu(valid.clone()), RuntimeError))
    return out


DEFECT_LABELS = {}          # (row, operand) -> labels, without building a tensor: the parametrisation's ids


def dependent_cases():
    """[(row, operand, defect label)] for every (wrapper, dependent operand) of the table and every defect of that operand."""
    out = []
    for row in ROWS:
        for operand, rule in row.dependent.items():
            labels = []
            for ax in rule.axes:
                tag = "" if len(rule.axes) == 1 else "-axis%d" % ax
                labels.append("short" + tag)
                if not rule.at_least:
                    labels.append("long" + tag)
            DEFECT_LABELS[(row.name, operand)] = labels + ["rank", "dtype", "cpu"]
            out += [(row, operand, lab) for lab in DEFECT_LABELS[(row.name, operand)]]
    return out


def dependent_pairs():
    return [(row, operand) for row in ROWS for operand in row.dependent]


def names_operand(message, operand):
    """Whether an error text names the operand as a word of its own (`shift`, `conv_igemm.shift`, `labels_a`)."""
    return re.search(r"(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])" % re.escape(operand), message) is not None
