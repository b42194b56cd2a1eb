"""ctypes binding of ``libfrmap_hip.so`` (C ABI declared in ``include/frmap_hip.h``).

There is deliberately no fallback: if the shared library has not been built
(``python -c "import __graft_entry__ as g; g.build()"`` or ``csrc/build.sh``) every compute entry
point raises ``RuntimeError`` — the product path never routes through PyTorch eager or the CPU
oracle.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# FRMAP_LIB: load another build of the library (A/B variants made by tools; must have the same ABI) instead of the in-tree one
LIB_PATH = os.environ.get("FRMAP_LIB") or os.path.join(_PKG_DIR, "libfrmap_hip.so")
ABI_VERSION = 10

_lock = threading.Lock()
_lib = None

_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t

# name -> (restype, argtypes); mirrors include/frmap_hip.h one to one
PROTOTYPES = {
    "frmap_abi_version": (_i, []),
    "frmap_set_batch_invariant": (_i, [_i]),
    "frmap_last_error": (C.c_char_p, []),
    "frmap_pack_input_nchw_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "frmap_pack_conv_weight": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "frmap_small_cin_kpad": (_i, [_i, _i]),
    "frmap_pack_conv_weight_c3": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "frmap_conv_small_cin": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "frmap_match_gallery_pack_bytes": (_sz, [_i, _i]),
    "frmap_match_pack_gallery": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "frmap_match_pack_gallery_rows": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "frmap_match_top1_packed": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i, _i, _i, _vp]),
    "frmap_resize_bilinear_u8": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "frmap_crop_resize_u8": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "frmap_resize_coeffs_host": (_i, [_i, _i, _vp, _vp, _vp]),
    "frmap_align_crop_resize_u8": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "frmap_align_warp_host": (_i, [_vp, _i, _i, C.c_longlong, _vp, _i, _i, _i, _i, _i, _vp]),
    "frmap_crop_resize_yuv": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "frmap_align_crop_resize_yuv": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "frmap_yuv_to_rgb_host": (_i, [_vp, _vp, _vp, _i, _i, C.c_longlong, C.c_longlong, _i, _i, _vp]),
    "frmap_yuv_align_warp_host": (_i, [_vp, _vp, _vp, _i, _i, C.c_longlong, C.c_longlong, _i, _i, _vp, _i, _i, _i, _i, _vp]),
    "frmap_track_state_bytes": (_sz, [_i, _i]),
    "frmap_track_step": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, C.c_double, C.c_double, _vp, _vp, _vp]),
    "frmap_track_step_host": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, C.c_double, C.c_double, _vp, _vp]),
    "frmap_track_fuse_state_bytes": (_sz, [_i, _i, _i]),
    "frmap_track_fuse": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp]),
    "frmap_track_fuse_host": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp]),
    "frmap_gap_linear_norm": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i, _i, _i, _i, _i, _vp]),
    "frmap_conv_small_cin_pool2": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "frmap_conv_igemm_pool2_supported": (_i, [_i, _i, _i, _i, _i]),
    "frmap_conv_igemm_pool2_form": (_i, [_i, _i, _i, _i, _i]),
    "frmap_conv3x3_pp_pool_layout": (_i, [_i, _i, _i, _i, _i]),
    "frmap_conv_igemm_pool2": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "frmap_stem7x7_maxpool": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "frmap_stem7x7_maxpool2": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "frmap_stem7x7_maxpool_u8": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "frmap_conv_igemm": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "frmap_conv_pp_tuning": (_i, [_i, _i, _i]),
    "frmap_conv_pp_ri": (_i, [_i]),
    "frmap_conv_pp_pitch": (_i, [_i]),
    "frmap_conv_pp_ds": (_i, [_i]),
    "frmap_conv_pp_im": (_i, [_i]),
    "frmap_conv_wave_start": (_i, [_i]),
    "frmap_conv1x1_pp_layout": (_i, [_i, _i, _i, _i, _i, _i]),
    "frmap_conv3x3_pp_layout": (_i, [_i, _i, _i, _i, _i]),
    "frmap_conv3x3s2_pp_layout": (_i, [_i, _i, _i, _i, _i]),
    "frmap_conv3x3_pp_ds_layout": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "frmap_conv3x3_pp_tile_px": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "frmap_conv_plan_key": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.c_char_p, _i]),
    "frmap_conv_plan_keys": (_i, [_i, C.c_char_p, _i]),
    "frmap_conv_plan_selfcheck": (_i, []),
    "frmap_conv_igemm_ds_supported": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "frmap_conv_igemm_ds": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "frmap_linear_mfma_workspace_bytes": (_sz, [_i, _i, _i]),
    "frmap_linear_mfma": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "frmap_maxpool": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "frmap_avgpool_global": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "frmap_avgpool_adaptive": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "frmap_linear_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "frmap_l2_normalize_f32": (_i, [_vp, _vp, _i, _i, _f, _vp]),
    "frmap_cast_to_f32": (_i, [_vp, _vp, _sz, _i, _vp]),
    "frmap_cast_from_f32": (_i, [_vp, _vp, _sz, _i, _vp]),
    "frmap_add_pos_layernorm": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp]),
    "frmap_mha_tokens": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "frmap_mean_layernorm": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp]),
    "frmap_cnn_attention": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "frmap_normalize_u8_hwc": (_i, [_vp, _vp, _vp, _i, _i, _i, C.POINTER(C.c_float), C.POINTER(C.c_float), _i, _vp]),
    "frmap_softmax_argmax": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "frmap_pairwise_distance": (_i, [_vp, _vp, _vp, _vp, _f, _i, _i, _vp]),
    "frmap_classify_tally_words": (_sz, [_i, _i, _i, _i]),
    "frmap_classify_tally": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "frmap_classify_tally_host": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "frmap_ovr_append": (_i, [_vp, _vp, _i, _i, _vp, _vp, C.c_longlong, C.c_longlong, _vp]),
    "frmap_ovr_rank_counts": (_i, [_vp, _vp, C.c_longlong, C.c_longlong, _i, _vp, _vp, _vp, _vp]),
    "frmap_ovr_rank_counts_host": (_i, [_vp, _vp, C.c_longlong, C.c_longlong, _i, _vp, _vp, _vp]),
    "frmap_head_fit_state_bytes": (_sz, [_i, _i, _i]),
    "frmap_head_fit_workspace_bytes": (_sz, [_i, _i, _i]),
    "frmap_head_fit_step": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _i, _vp]),
    "frmap_head_fit_step_host": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _i, _i]),
    "frmap_head_fit_group_state_stride": (_sz, [_i, _i, _i]),
    "frmap_head_fit_group_state_bytes": (_sz, [_i, _i, _i, _i]),
    "frmap_head_fit_group_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "frmap_head_fit_group_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "frmap_head_fit_group_step_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i]),
    "frmap_head_fit_hidden_state_bytes": (_sz, [_i, _i, _i, _i]),
    "frmap_head_fit_hidden_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "frmap_head_fit_hidden_step": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f,
                                        _i, _vp]),
    "frmap_head_fit_hidden_step_host": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f,
                                             _f, _i, _i]),
    "frmap_head_fit_pair_state_bytes": (_sz, [_i, _i, _i]),
    "frmap_head_fit_pair_workspace_bytes": (_sz, [_i, _i, _i]),
    "frmap_head_fit_pair_step": (_i, [_vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _i, _vp]),
    "frmap_head_fit_pair_step_host": (_i, [_vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _i,
                                           _i]),
    "frmap_head_fit_margin_state_bytes": (_sz, [_i, _i, _i]),
    "frmap_head_fit_margin_workspace_bytes": (_sz, [_i, _i, _i]),
    "frmap_head_fit_margin_step": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _i, _vp]),
    "frmap_head_fit_margin_step_host": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _i, _i]),
    "frmap_head_fit_embed_state_bytes": (_sz, [_i, _i, _i, _i]),
    "frmap_head_fit_embed_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "frmap_head_fit_embed_step": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f,
                                       _f, _f, _f, _f, _i, _vp]),
    "frmap_head_fit_embed_step_host": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f,
                                            _f, _f, _f, _f, _f, _i, _i]),
    "frmap_head_workspace_bytes": (_sz, [_i, _i]),
    "frmap_match_workspace_bytes": (_sz, [_i, _i]),
    "frmap_match_top1": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _i, _i, _i, _vp]),
    "frmap_match_topk_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "frmap_match_topk": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "frmap_match_topk_packed": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "frmap_verify_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "frmap_verify_counts": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "frmap_verify_counts_packed": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "frmap_match_radius_workspace_bytes": (_sz, [_i, _i, _i]),
    "frmap_match_radius": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp, C.c_longlong, _vp, _vp, _vp]),
    "frmap_match_radius_packed": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp, C.c_longlong, _vp,
                                       _vp, _vp]),
    "frmap_gap_norm_match": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _f, _i, _i, _i, _i, _i, _vp]),
    "frmap_cosine_logits": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "frmap_arcmargin_eval": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _i, _vp]),
    # model handles
    "frmap_model_create": (_i, [C.POINTER(_vp), C.c_char_p, _i, _i]),
    "frmap_model_load_tensor": (_i, [_vp, C.c_char_p, _vp, _sz, _i]),
    "frmap_model_set_input_normalization": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "frmap_model_finalize": (_i, [_vp, _vp]),
    "frmap_model_embedding_dim": (_i, [_vp]),
    "frmap_model_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "frmap_model_match_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i]),
    "frmap_model_forward": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "frmap_model_embed_and_match": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "frmap_model_search_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i, _i]),
    "frmap_model_embed_and_search": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "frmap_model_trace": (_i, [_vp, _i]),
    "frmap_model_trace_read": (_i, [_vp, _vp, _i]),
    "frmap_model_destroy": (None, [_vp]),
}

# Pointer alignment of every device-pointer argument of every launching entry point (include/frmap_hip.h, Conventions, "pointer
# alignment"): entry point -> {argument: (class, bytes)}.  `bytes` is what the launcher rejects below - the widest access a kernel
# behind it makes through the pointer; where the launcher picks a narrower path for some shapes (odd H * W, D % 512 != 0, ...) this is
# the widest of them, so a tensor that meets it is accepted whatever the shape.  A class's default is in ALIGN_CLASS (None: the
# element size); an argument that departs from it has its own note in the header.  tests/test_place_cpu.py compares both with the header.
ALIGN_CLASS = {
    "tensor": 16,      # activations, residuals, packed weights / galleries, fp16 splits and outputs in `dtype`
    "vector": 16,      # fp32 per-channel vectors of the MFMA kernels (shift; pos / gamma / beta of add_pos_layernorm)
    "matrix": 16,      # fp32 matrices a GEMM, the exact re-score or the tracker reads in float4 pieces (rows are multiples of 4)
    "element": None,   # everything walked element by element
    "record": 8,       # records with 8-byte fields or int32 pairs
    "workspace": 16,   # scratch and state buffers
}
_T, _V, _M, _R, _W = ("tensor", 16), ("vector", 16), ("matrix", 16), ("record", 8), ("workspace", 16)
_W256 = ("workspace", 256)
_E1, _E2, _E4, _E8 = (("element", n) for n in (1, 2, 4, 8))
_TOP1_OUT = {"idx_out": _E4, "dist_out": _E4, "id_or_unknown_out": _E4, "packed_out": _E4}
_PAIRS = {"a": _M, "label_a": _E4, "b": _M, "label_b": _E4}
_CROP = {"frames": _R, "rois": _E4, "out": _E1}
_STEM = {"w_packed_c3": _T, "shift": _V, "out": _T}
ALIGNMENT = {
    "frmap_pack_input_nchw_f32": {"x_nchw": _E4, "out_nhwc4": ("tensor", 8)},
    "frmap_normalize_u8_hwc": {"img_u8": _E1, "out_nchw_f32": _E4, "out_nhwc4": ("tensor", 8)},
    "frmap_resize_bilinear_u8": {"src_pool": _E1, "items": _R, "tables": _E4, "out": _E1},
    "frmap_crop_resize_u8": _CROP,
    "frmap_align_crop_resize_u8": {"frames": _R, "rois": _E4, "mats": _R, "out": _E1},
    "frmap_crop_resize_yuv": _CROP,
    "frmap_align_crop_resize_yuv": {"frames": _R, "rois": _E4, "mats": _R, "out": _E1},
    "frmap_track_step": {"state": _W, "boxes": _M, "probs": _E4, "counts": _E4, "frame_hw": _E4, "ids_out": _E4, "rois_out": ("record", 16)},
    "frmap_track_fuse": {"state": _W, "ids": _E4, "counts": _E4, "emb": _M, "rows": _R, "fused": _M, "frames_out": _E4},
    "frmap_pack_conv_weight": {"w_oihw": _E4, "w_packed": ("tensor", 2)},
    "frmap_pack_conv_weight_c3": {"w_oihw": _E4, "w_packed": ("tensor", 2)},
    "frmap_conv_small_cin": {"in_nhwc4": ("tensor", 8), "w_packed": _T, "shift": _V, "out": _T},
    "frmap_conv_small_cin_pool2": {"in_nhwc4": ("tensor", 8), "w_packed": _T, "shift": _V, "out": _T},
    "frmap_stem7x7_maxpool": {"x_nchw": _E4, **_STEM},
    "frmap_stem7x7_maxpool2": {"x_nchw": _E4, **_STEM},
    "frmap_stem7x7_maxpool_u8": {"x_u8_hwc": ("element", 4), **_STEM},
    "frmap_conv_igemm": {"in": _T, "w_packed": _T, "shift": _V, "residual": _T, "out": _T},
    "frmap_conv_igemm_pool2": {"in": _T, "w_packed": _T, "shift": _V, "out": _T},
    "frmap_conv_igemm_ds": {"in": _T, "w_packed": _T, "shift": _V, "ds_in": _T, "ds_w_packed": _T, "out": _T},
    "frmap_linear_mfma": {"x": _T, "w_packed": _T, "shift": _V, "residual": _T, "out": _T, "workspace": _W},
    "frmap_maxpool": {"in": _T, "out": _T},
    "frmap_avgpool_global": {"in": _T, "out_f32": _E4},
    "frmap_avgpool_adaptive": {"in": _T, "out": _T},
    "frmap_linear_f32": {"x": _M, "w": _M, "scale": _E4, "shift": _E4, "out": _E4},
    "frmap_l2_normalize_f32": {"x": _E4, "out": _E4},
    "frmap_cast_to_f32": {"in": _E2, "out": _E4},
    "frmap_cast_from_f32": {"in": _E4, "out": _E2},
    "frmap_add_pos_layernorm": {"x": _T, "pos": _V, "gamma": _V, "beta": _V, "t_out": _T, "y_out": _T},
    "frmap_mha_tokens": {"qkv": _T, "out": _T},
    "frmap_mean_layernorm": {"t": _T, "gamma": _E4, "beta": _E4, "out_f32": _E4},
    "frmap_cnn_attention": {"qkv": _T, "x": _T, "gamma": _E4, "spatial_w": _E4, "spatial_b": _E4, "out_map": ("tensor", 4), "out_pool": _E4},
    "frmap_softmax_argmax": {"logits": _E4, "probs_out": _E4, "pred_out": _E4},
    "frmap_pairwise_distance": {"a": _E4, "b": _E4, "dist_out": _E4, "same_out": _E4},
    "frmap_classify_tally": {"logits": _E4, "labels": _E4, "state": _E8, "row_pred_out": _E4, "row_rank_out": _E4, "row_conf_out": _E4,
                             "row_loss_out": _E4},
    "frmap_ovr_append": {"scores": _E4, "labels": _E4, "store": _E4, "store_labels": _E4},
    "frmap_ovr_rank_counts": {"store": _E4, "store_labels": _E4, "ge_same_out": _E8, "ge_other_out": _E8, "eq_other_out": _E8},
    "frmap_head_fit_step": {"x": _E4, "labels": _E4, "rows": _E4, "keep": _E1, "w": _E4, "b": _E4, "state": _E8, "workspace": _E4},
    "frmap_head_fit_group_step": {"x": _E4, "labels": _E4, "rows": _E4, "keep": _E1, "hyper": _E4, "w": _E4, "b": _E4, "state": _E8,
                                  "workspace": _E4},
    "frmap_head_fit_hidden_step": {"x": _E4, "labels": _E4, "rows": _E4, "keep1": _E1, "keep2": _E1, "w1": _E4, "b1": _E4, "w2": _E4, "b2": _E4,
                                   "state": _E8, "workspace": _E4},
    "frmap_head_fit_pair_step": {"x": _E4, "left": _E4, "right": _E4, "differ": _E4, "keep": _E1, "w": _E4, "b": _E4, "state": _E8,
                                 "workspace": _E4},
    "frmap_head_fit_margin_step": {"x": _E4, "labels": _E4, "rows": _E4, "keep": _E1, "w": _E4, "state": _E8, "workspace": _E4},
    "frmap_head_fit_embed_step": {"x": _E4, "labels": _E4, "rows": _E4, "keep": _E1, "w1": _E4, "gamma": _E4, "beta": _E4, "running_mean": _E4,
                                  "running_var": _E4, "wc": _E4, "state": _E8, "workspace": _E4},
    "frmap_match_top1": {"emb": _M, "gallery": _M, **_TOP1_OUT, "workspace": _W},
    "frmap_match_pack_gallery": {"gallery": _E4, "packed_out": ("tensor", 2), "stat_w_out": _E4},
    "frmap_match_pack_gallery_rows": {"gallery": _E4, "packed_out": ("tensor", 2), "stat_w_out": _E4},
    "frmap_match_top1_packed": {"emb": _M, "gallery": _M, "gallery_packed": _T, "stat_w": _M, **_TOP1_OUT, "workspace": _W, "probe_split": _T},
    "frmap_match_topk": {"emb": _M, "gallery": _M, "labels": _E4, "idx_out": _E4, "dist_out": _E4, "label_out": _E4, "workspace": _W256},
    "frmap_match_topk_packed": {"emb": _M, "gallery": _M, "gallery_packed": _T, "stat_w": _M, "labels": _E4, "idx_out": _E4, "dist_out": _E4,
                                "label_out": _E4, "workspace": _W256},
    "frmap_verify_counts": {**_PAIRS, "thresholds": _E4, "accepted_out": _E8, "rescored_out": _E8, "workspace": _W256},
    "frmap_verify_counts_packed": {"a": _M, "label_a": _E4, "b": _M, "b_packed": _T, "stat_w": _M, "label_b": _E4, "thresholds": _E4,
                                   "accepted_out": _E8, "rescored_out": _E8, "workspace": _W256},
    "frmap_match_radius": {**_PAIRS, "count_out": _E4, "total_out": _E8, "pair_out": _R, "dist_out": _E4, "rescored_out": _E8,
                           "workspace": _W256},
    "frmap_match_radius_packed": {"a": _M, "label_a": _E4, "b": _M, "b_packed": _T, "stat_w": _M, "label_b": _E4, "count_out": _E4,
                                  "total_out": _E8, "pair_out": _R, "dist_out": _E4, "rescored_out": _E8, "workspace": _W256},
    "frmap_gap_norm_match": {"map": _T, "gallery": _M, "emb_out": _E4, **_TOP1_OUT},
    "frmap_gap_linear_norm": {"map": _T, "wt": _E4, "scale": _E4, "shift": _E4, "pre_out": _E4, "emb_out": _E4},
    "frmap_cosine_logits": {"x": _M, "w": _M, "logits_out": _E4, "argmax_out": _E4, "workspace": _W},
    "frmap_arcmargin_eval": {"x": _M, "w": _M, "label": _E8, "logits_out": _E4, "minmax_out": _E4, "workspace": _W},
    "frmap_model_forward": {"x": ("element", 4), "out": _T, "workspace": _W256},
    "frmap_model_embed_and_match": {"x": ("element", 4), "gallery": _M, "gallery_packed": _T, "gallery_stat": _M, **_TOP1_OUT, "emb_out": _M,
                                    "workspace": _W256},
    "frmap_model_embed_and_search": {"x": ("element", 4), "gallery": _M, "gallery_packed": _T, "gallery_stat": _M, "labels": _E4, "idx_out": _E4,
                                     "dist_out": _E4, "label_out": _E4, "emb_out": _M, "workspace": _W256},
}


def align_of(entry: str, arg: str) -> int:
    """Bytes a tensor handed to `entry` as `arg` must be aligned to (KeyError for a name the header does not have)."""
    return ALIGNMENT[entry][arg][1]


def lib_available() -> bool:
    return os.path.isfile(LIB_PATH)


def load() -> C.CDLL:
    """Load (once) and return the library; raise loudly if it is missing or has the wrong ABI."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not lib_available():
            raise RuntimeError(
                f"HIP extension not built: {LIB_PATH} is missing. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
                "There is no CPU / PyTorch fallback for this path.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if lib.frmap_abi_version() != ABI_VERSION:
            raise RuntimeError(f"libfrmap_hip.so ABI {lib.frmap_abi_version()} != expected {ABI_VERSION}; rebuild")
        _lib = lib
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().frmap_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError(f"{what}: {msg}")
        raise RuntimeError(f"{what}: {msg} (rc={rc})")
