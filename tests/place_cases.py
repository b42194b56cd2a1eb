"""Where a buffer starts: helpers of the pointer-alignment tests (`test_place_cpu.py`, `test_place_*_gpu.py`).

A plain helper module like `conv_cases.py` and `guard.py` (no fixture, no setting).  Four things live here.

THE REQUIREMENT (`requirement`).  `guard.shifted` places every buffer "aligned to A and not to 2 A"; A comes from this function of
an allocation's dtype, kind and caller.  The guard sees a tensor, not the C argument it will become, so A is the LARGEST alignment
`_lib.ALIGNMENT` asks of any argument a tensor of that dtype and origin can become - never less than the kernel behind it needs
(include/frmap_hip.h, Conventions, "pointer alignment"), and for most buffers exactly what it needs:
  * operands (`Guard.place`), by dtype: fp16 / bf16 16 (tensors in `dtype`), fp32 16 (matrices and per-channel vectors of the MFMA
    kernels; the element-wise fp32 operands are then at 16 as well), float64 8 (mats), int64 8 (labels of arcmargin_eval), int32 8
    (rows; labels, counts and ids then at 8), uint8 4 (the uint8 stem input; frames and images then at 4);
  * outputs and workspaces the wrappers allocate (`Guard.empty` through the patched `torch`), by the function that asked and the
    dtype (`WRAPPER`), else by dtype: fp16 / bf16 16, fp32 16, int32 16 (rois_out), int64 16 (the match and head workspaces are
    int64 buffers), uint8 256 (the byte workspaces the header declares 256-byte aligned: top-k, verify, radius, model); the
    uint8 gallery pack of `MatchPack` and the tracker states are named in `WRAPPER` at 16, the uint8 images of resize.py at 1.
  A packed weight or gallery that a wrapper allocates is placed at 16: the packers write it element by element and would take 2,
  but the kernels that read it afterwards are the ones worth moving.  What the binding does with an operand BELOW its requirement (it
  copies it) is the business of the offset-view tests in `test_place_ops_gpu.py`, not of this placement.

THE RULE ON EXISTING CASES (`at_minimum_alignment`, `mirror`).  The guard tests (`test_guard_*_gpu.py`) hand their closures to
`guard.two_fills`.  Inside `at_minimum_alignment()` that name is `guard.shifted` with the requirement above, so a guard test's own
body - its case table, its `place=` closure, its path assertions and its float64 reference where it has one - runs under the second
rule.  `mirror(module, name)` wraps one such test function, parametrisation and fixtures included, for a `test_place_*` file:
nothing is pasted, and a case added to a guard test is a case of the placement test.

REJECTIONS (`misaligned_calls`).  For every entry point and every pointer argument whose requirement exceeds its element size,
the smallest valid call with that one pointer moved by half the requirement (`REJECT_CALLS` builds the argument lists; a test
supplies the memory).  CPU and GPU files share the table: with host dummy pointers the call must be refused all the same, because
the refusal comes before any HIP call.

VIEWS (`offset_rule` / `mirror_offset`, `strided_rule` / `mirror_strided`).  The guard tests once more with every placed operand a
contiguous view one element into its allocation (`test_place_*_gpu.py`), or a strided view of a wider tensor (`test_operands_gpu.py`;
the views themselves are `operand_cases.strided_view` / `permuted_view`): the binding copies what it cannot pass on, and the result
holds the bits of the call on clones.
"""
import contextlib
import inspect

import torch

import guard
from frmap_amd import _lib

OPERAND = {torch.float16: 16, torch.bfloat16: 16, torch.float32: 16, torch.float64: 8, torch.int64: 8, torch.int32: 8, torch.uint8: 4,
           torch.int8: 1, torch.bool: 1, torch.int16: 2}
EMPTY = {torch.float16: 16, torch.bfloat16: 16, torch.float32: 16, torch.float64: 8, torch.int64: 16, torch.int32: 16, torch.uint8: 256,
         torch.int8: 1, torch.bool: 1, torch.int16: 2}
# (function that asked, dtype) -> bytes, where the wrapper's buffer is of a class that needs less than its dtype's default
_F32_ELEMENT = ["avgpool_global", "linear_f32", "l2_normalize", "cast_to_f32", "mean_layernorm", "softmax_argmax", "pairwise_distance",
                "gap_linear_norm", "gap_norm_match", "cosine_logits", "arcmargin_eval", "cnn_attention", "match_top1", "match_topk",
                "normalize_u8", "forward", "call"]
_I32_ELEMENT = ["softmax_argmax", "pairwise_distance", "gap_norm_match", "cosine_logits", "match_top1", "match_topk", "match_radius",
                "embed_and_match", "embed_and_search"]
WRAPPER = {("ops." + f, torch.float32): 4 for f in _F32_ELEMENT}
WRAPPER.update({("ops." + f, torch.int32): 4 for f in _I32_ELEMENT})
WRAPPER.update({("ops.call", torch.int32): 8,                 # match_radius' pair list: int32 pairs
                ("ops.verify_counts", torch.int64): 8, ("ops.match_radius", torch.int64): 8,       # uint64 counters
                ("ops.cast_from_f32", torch.float16): 2, ("ops.cast_from_f32", torch.bfloat16): 2,
                ("ops.normalize_u8", torch.float16): 8, ("ops.normalize_u8", torch.bfloat16): 8,
                ("ops.cnn_attention", torch.float16): 4, ("ops.cnn_attention", torch.bfloat16): 4,
                ("ops.pack_input", torch.float16): 8, ("ops.pack_input", torch.bfloat16): 8,       # (then the one-pixel path)
                # uint8 buffers that are NOT 256-byte workspaces: the gallery pack the match GEMM fetches by LDS-DMA
                # (`MatchPack.__init__`) and the two tracker states, 16 each
                ("ops.__init__", torch.uint8): 16, ("ops.track_state", torch.uint8): 16, ("ops.track_fuse_state", torch.uint8): 16})


def requirement(dtype, kind, who):
    """Bytes the buffer of this allocation must be aligned to (module docstring)."""
    if kind == "operand":
        return OPERAND[dtype]
    if dtype == torch.uint8 and who.split(".")[0] in ("resize", "frames"):
        return 1                                                   # crops and resized images: byte-addressed outputs
    return WRAPPER.get((who, dtype), EMPTY[dtype])


CALLS = {"shifted": 0, "offset": 0, "strided": 0}      # how often a substituted rule ran: a mirrored test that never reaches it tests nothing


def shifted_rule(run, modules=(), device="cuda", band=guard.BAND, canon=None, what=""):
    """`guard.shifted` under `requirement`, with the signature of `guard.two_fills`."""
    CALLS["shifted"] += 1
    return guard.shifted(run, modules, device=device, band=band, canon=canon, what=what, requirement=requirement)


@contextlib.contextmanager
def at_minimum_alignment():
    """Inside the block `guard.two_fills` IS the second rule: a guard test called here runs its own closure with every buffer at
    its minimum alignment and compares with the aligned call (and goes on to its own reference checks)."""
    saved, before = guard.two_fills, CALLS["shifted"]
    guard.two_fills = shifted_rule
    try:
        yield
    finally:
        guard.two_fills = saved
    assert CALLS["shifted"] > before, "the guard test never called guard.two_fills: nothing was placed"


def mirror(module, name):
    """The guard test `module.name` as a placement test: same parameters, same fixtures, same body, the second rule."""
    fn = getattr(module, name)

    def test(*args, **kwargs):
        with at_minimum_alignment():
            return fn(*args, **kwargs)
    test.__name__ = test.__qualname__ = name
    test.__doc__ = "`%s.%s` with every buffer at its minimum alignment (`guard.shifted`)." % (module.__name__, name)
    test.__signature__ = inspect.signature(fn)
    test.pytestmark = list(getattr(fn, "pytestmark", []))
    return test


# ---------------------------------------------------------------------------------------------------------------------------------
# rejections
# ---------------------------------------------------------------------------------------------------------------------------------
F16 = 1          # FRMAP_F16


def element_size(entry, arg):
    """Bytes of one element behind a pointer argument: what `_lib.ALIGNMENT` gives an "element" its size from, by class otherwise."""
    cls, need = _lib.ALIGNMENT[entry][arg]
    if cls in ("tensor",):
        return 2
    if cls in ("vector", "matrix"):
        return 4
    if cls == "workspace":
        return 1
    if cls == "record":
        return 8 if arg in ("mats", "frames", "items") else 4
    if arg == "x" and entry.startswith("frmap_model_"):
        return 1                                                   # (void*: uint8 or fp32)
    return {"x_nchw": 4, "x_u8_hwc": 1}.get(arg, need)


def needs_rejection_test(entry, arg):
    return _lib.ALIGNMENT[entry][arg][1] > element_size(entry, arg)


# entry point -> (pointer arguments in declaration order, the remaining arguments in declaration order with '*' where the pointers go).
# Shapes are the smallest the launcher takes; every pointer gets `buf` (one 256-byte aligned buffer large enough for any of them),
# the argument under test `buf + need / 2`.  `stream` is NULL.  Host-side float triples are built by the caller ("mean", "std").
REJECT_CALLS = {
    "frmap_pack_input_nchw_f32": ["x_nchw", "out_nhwc4", 1, 2, 2, F16],
    "frmap_normalize_u8_hwc": ["img_u8", "out_nchw_f32", "out_nhwc4", 1, 2, 2, "mean", "std", F16],
    "frmap_conv_small_cin": ["in_nhwc4", "w_packed", "shift", "out", 1, 8, 8, 32, 3, 3, 1, 1, 1, F16],
    "frmap_conv_small_cin_pool2": ["in_nhwc4", "w_packed", "shift", "out", 1, 8, 8, 32, 1, F16],
    "frmap_stem7x7_maxpool": ["x_nchw", "w_packed_c3", "shift", "out", 1, 8, 8, F16],
    "frmap_stem7x7_maxpool2": ["x_nchw", "w_packed_c3", "shift", "out", 1, 8, 8, F16],
    "frmap_stem7x7_maxpool_u8": ["x_u8_hwc", "mean", "std", "w_packed_c3", "shift", "out", 1, 8, 8, 1, F16],
    "frmap_conv_igemm": ["in", "w_packed", "shift", "residual", "out", 1, 2, 2, 32, 64, 3, 1, 1, 1, F16],
    "frmap_conv_igemm_pool2": ["in", "w_packed", "shift", "out", 1, 2, 2, 32, 64, 1, F16],
    "frmap_conv_igemm_ds": ["in", "w_packed", "shift", "ds_in", "ds_w_packed", "out", 1, 2, 2, 64, 64, 4, 4, 32, 2, 1, F16],
    "frmap_linear_mfma": ["x", "w_packed", "shift", "residual", "out", "workspace", 1, 32, 64, 0, F16],
    "frmap_maxpool": ["in", "out", 1, 2, 2, 8, 2, 2, 0, F16],
    "frmap_avgpool_global": ["in", "out_f32", 1, 1, 8, F16],
    "frmap_avgpool_adaptive": ["in", "out", 1, 2, 2, 8, 1, 1, F16],
    "frmap_linear_f32": ["x", "w", "scale", "shift", "out", 1, 4, 1, 0],
    "frmap_add_pos_layernorm": ["x", "pos", "gamma", "beta", "t_out", "y_out", 1, 1, 512, 1e-5, F16],
    "frmap_mha_tokens": ["qkv", "out", 1, 1, 128, 1, F16],
    "frmap_mean_layernorm": ["t", "gamma", "beta", "out_f32", 1, 1, 8, 1e-5, F16],
    "frmap_cnn_attention": ["qkv", "x", "gamma", "spatial_w", "spatial_b", "out_map", "out_pool", 1, 1, 1, 8, 256, 1, F16],
    "frmap_match_top1": ["emb", "gallery", "idx_out", "dist_out", "id_or_unknown_out", "packed_out", 1.0, "workspace", 1, 1, 4],
    "frmap_match_top1_packed": ["emb", "gallery", "gallery_packed", "stat_w", "idx_out", "dist_out", "id_or_unknown_out", "packed_out", 1.0,
                                "workspace", "probe_split", 1, 1, 32],
    "frmap_match_topk": ["emb", "gallery", "labels", "idx_out", "dist_out", "label_out", "workspace", 1, 1, 4, 2],
    "frmap_match_topk_packed": ["emb", "gallery", "gallery_packed", "stat_w", "labels", "idx_out", "dist_out", "label_out", "workspace",
                                1, 1, 32, 2],
    "frmap_verify_counts": ["a", "label_a", 1, "b", "label_b", 1, 4, -1, "thresholds", 1, "accepted_out", "rescored_out", "workspace"],
    "frmap_verify_counts_packed": ["a", "label_a", 1, "b", "b_packed", "stat_w", "label_b", 1, 32, -1, "thresholds", 1, "accepted_out",
                                   "rescored_out", "workspace"],
    "frmap_match_radius": ["a", "label_a", 1, "b", "label_b", 1, 4, -1, 1.0, 0, "count_out", "total_out", "pair_out", "dist_out", 1,
                           "rescored_out", "workspace"],
    "frmap_match_radius_packed": ["a", "label_a", 1, "b", "b_packed", "stat_w", "label_b", 1, 32, -1, 1.0, 0, "count_out", "total_out",
                                  "pair_out", "dist_out", 1, "rescored_out", "workspace"],
    "frmap_gap_norm_match": ["map", "gallery", "emb_out", "idx_out", "dist_out", "id_or_unknown_out", "packed_out", 1.0, 0, 1e-12, 1, 1, 8, 1,
                             F16],
    "frmap_gap_linear_norm": ["map", "wt", "scale", "shift", "pre_out", "emb_out", 1e-12, 1, 1, 8, 256, 0, F16],
    "frmap_cosine_logits": ["x", "w", "logits_out", "argmax_out", "workspace", 1, 1, 4, 1.0],
    "frmap_arcmargin_eval": ["x", "w", "label", "logits_out", "minmax_out", "workspace", 1, 1, 4, 1.0, 0.5, 0],
    "frmap_resize_bilinear_u8": ["src_pool", "items", "tables", "out", 1, 1, 1, 1, 1],
    "frmap_crop_resize_u8": ["frames", 1, "rois", "out", 1, 1, 1, 1, 1, 0],
    "frmap_align_crop_resize_u8": ["frames", 1, "rois", "mats", "out", 1, 1, 1, 1, 1, 0],
    "frmap_crop_resize_yuv": ["frames", 1, "rois", "out", 1, 1, 1, 1, 1],
    "frmap_align_crop_resize_yuv": ["frames", 1, "rois", "mats", "out", 1, 1, 1, 1, 1],
    "frmap_track_step": ["state", "boxes", "probs", "counts", "frame_hw", 1, 1, 0.9, 0.5, "ids_out", "rois_out"],
    "frmap_track_fuse": ["state", "ids", "counts", "emb", "rows", 1, 1, 1, 4, 1.0, "fused", "frames_out"],
}
REJECT_BYTES = 1 << 16          # every operand of every call above fits (the largest: 64 x 64 fp16 weights, 8 KiB)
# the word a refusal must carry for an argument whose launcher words the check itself (the checks that were there before the macro)
OWN_WORDING = {("frmap_track_step", "state"), ("frmap_track_step", "boxes"), ("frmap_track_step", "rois_out"),
               ("frmap_track_fuse", "state"), ("frmap_track_fuse", "emb"), ("frmap_track_fuse", "fused"), ("frmap_track_fuse", "rows")}


def misaligned_calls():
    """[(entry, argument, requirement)] of every rejection the header promises beyond the element size, model handles aside (they
    need a finalised model: `test_place_model_gpu.py`)."""
    out = []
    for entry, args in _lib.ALIGNMENT.items():
        if entry.startswith("frmap_model_"):
            continue
        for arg, (_, need) in args.items():
            if needs_rejection_test(entry, arg):
                out.append((entry, arg, need))
    return out


def reject_args(entry, moved, bufs, mean, std):
    """The argument list of `REJECT_CALLS[entry]` with pointer `moved` taken from `bufs[arg] + need / 2` and every other pointer
    from `bufs[arg]` (`bufs`: argument name -> address of an aligned buffer of `REJECT_BYTES`), then the NULL stream."""
    need = _lib.ALIGNMENT[entry][moved][1]
    args = []
    for a in REJECT_CALLS[entry]:
        if a == "mean":
            args.append(mean)
        elif a == "std":
            args.append(std)
        elif isinstance(a, str):
            args.append(bufs[a] + (max(need // 2, element_size(entry, a)) if a == moved else 0))
        else:
            args.append(a)
    return args + [None]


# ---------------------------------------------------------------------------------------------------------------------------------
# the binding: operands that are contiguous views with a storage offset
# ---------------------------------------------------------------------------------------------------------------------------------
def offset_view(t_cpu, device="cuda"):
    """`t_cpu` on the device as `flat[1:1 + n].view(shape)`: contiguous, one element past the start of its allocation."""
    t = t_cpu.detach().contiguous()
    flat = torch.empty((t.numel() + 1,), dtype=t.dtype, device=device)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == 1
    return v


def offset_rule(run, modules=(), device="cuda", band=None, canon=None, what=""):
    """With the signature of `guard.two_fills`: `run` on plain copies (the call on `.clone()`s) and on one-element-offset views of
    the same operands; the results hold the same bits.  Nothing is guarded: what the wrapper allocates is the allocator's."""
    CALLS["offset"] += 1
    canon = canon or (lambda r: r)
    dev = torch.device(device)
    ref = canon(guard._flat(run(lambda t: t.to(dev, copy=True))))
    got = canon(guard._flat(run(lambda t: offset_view(t, dev))))
    guard.Guard(0, 1, dev)._sync()
    assert len(got) == len(ref), (what, len(got), len(ref))
    for k in range(len(ref)):
        d = guard.first_difference(got[k], ref[k])
        assert d is None, "%s: result %d on one-element-offset views differs from the call on their clones: %s" % (what, k, d)
    return ref


@contextlib.contextmanager
def on_offset_views():
    """Inside the block `guard.two_fills` is `offset_rule`; the block must have reached it at least once."""
    saved, before = guard.two_fills, CALLS["offset"]
    guard.two_fills = offset_rule
    try:
        yield
    finally:
        guard.two_fills = saved
    assert CALLS["offset"] > before, "the guard test never called guard.two_fills: no operand was a view"


def mirror_offset(module, name):
    """The guard test `module.name` with every placed operand a one-element-offset view (`offset_rule`)."""
    fn = getattr(module, name)

    def test(*args, **kwargs):
        with on_offset_views():
            return fn(*args, **kwargs)
    test.__name__ = test.__qualname__ = name
    test.__doc__ = "`%s.%s` with every tensor input a contiguous view one element into its allocation." % (module.__name__, name)
    test.__signature__ = inspect.signature(fn)
    test.pytestmark = list(getattr(fn, "pytestmark", []))
    return test


# ---------------------------------------------------------------------------------------------------------------------------------
# the binding: operands that are strided views (`operand_cases.strided_view`, `permuted_view`)
# ---------------------------------------------------------------------------------------------------------------------------------
def strided_rule(run, modules=(), device="cuda", band=None, canon=None, what=""):
    """With the signature of `guard.two_fills`: `run` on plain copies (the call on `.clone()`s) and with EVERY placed operand a strided
    view of a wider tensor (`wide[..., ::2]`: the binding copies each, and all the copies of one call are alive at once); where `run`
    placed a 4-D operand, once more with every 4-D operand the `permute(0, 2, 3, 1)` view of a tensor laid out the other way round
    (what a torch user has in hand for an NHWC map) and the others strided.  The results hold the same bits.  An operand the call
    WRITES is not placed by any guard test (the states come from `ops.track_state` / `ops.track_fuse_state` inside `run`), so it keeps
    its own form.  Nothing is guarded: what the wrapper allocates is the allocator's."""
    import operand_cases as oc
    CALLS["strided"] += 1
    canon = canon or (lambda r: r)
    dev = torch.device(device)
    seen = {"n": 0, "4d": 0}

    def strided(t):
        seen["n"] += 1
        seen["4d"] += t.dim() == 4
        return oc.strided_view(t, dev)

    def permuted(t):
        return oc.permuted_view(t, dev) if t.dim() == 4 else oc.strided_view(t, dev)
    ref = canon(guard._flat(run(lambda t: t.to(dev, copy=True))))
    forms = [("strided views (wide[..., ::2])", strided)]
    got = [canon(guard._flat(run(strided)))]
    assert seen["n"] > 0, "%s: the case placed no operand: nothing was strided" % what
    if seen["4d"]:
        forms.append(("permute(0, 2, 3, 1) views of its 4-D operands", permuted))
        got.append(canon(guard._flat(run(permuted))))
    guard.Guard(0, 1, dev)._sync()
    for (form, _), res in zip(forms, got):
        assert len(res) == len(ref), (what, form, len(res), len(ref))
        for k in range(len(ref)):
            d = guard.first_difference(res[k], ref[k])
            assert d is None, "%s: result %d on %s differs from the call on their clones: %s" % (what, k, form, d)
    return ref


@contextlib.contextmanager
def on_strided_views():
    """Inside the block `guard.two_fills` is `strided_rule`; the block must have reached it at least once."""
    saved, before = guard.two_fills, CALLS["strided"]
    guard.two_fills = strided_rule
    try:
        yield
    finally:
        guard.two_fills = saved
    assert CALLS["strided"] > before, "the guard test never called guard.two_fills: no operand was strided"


def mirror_strided(module, name):
    """The guard test `module.name` with every placed operand a strided view (`strided_rule`)."""
    fn = getattr(module, name)

    def test(*args, **kwargs):
        with on_strided_views():
            return fn(*args, **kwargs)
    test.__name__ = test.__qualname__ = name
    test.__doc__ = "`%s.%s` with every tensor input a strided view of a wider tensor." % (module.__name__, name)
    test.__signature__ = inspect.signature(fn)
    test.pytestmark = list(getattr(fn, "pytestmark", []))
    return test
