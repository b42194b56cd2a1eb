"""No GPU: the tables and the host-side helpers of the stream tests (`stream_cases.py`)."""
import ast
import os

import pytest
import torch

import stream_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
# the guard modules the stream files mirror, and the tests of each that do NOT hand a closure to `guard.two_fills`
SOURCES = {"test_guard_ops_gpu.py": {"test_positive_control_one_element_too_many"},
           "test_guard_conv_gpu.py": {"test_conv_case_is_guarded", "test_gelu_case_is_guarded", "test_linear_case_is_guarded"},
           "test_guard_model_gpu.py": set(),
           "test_guard_frames_gpu.py": {"test_a_record_that_breaks_the_contract_leaves_its_rows_at_the_fill"},
           "test_guard_yuv_gpu.py": {"test_a_record_that_breaks_the_contract_leaves_its_rows_at_the_fill"}}
REQUIRED_TRUE = ["test_pack_input", "test_normalize_u8", "test_maxpool", "test_avgpool_global", "test_avgpool_adaptive", "test_casts",
                 "test_linear_f32_and_l2_normalize", "test_softmax_argmax_and_pairwise_distance", "test_gap_linear_norm",
                 "test_gap_norm_match", "test_cosine_logits_and_arcmargin", "test_match_top1", "test_match_top1_empty_gallery",
                 "test_match_topk", "test_layernorm_kernels", "test_mha_tokens", "test_cnn_attention", "test_track_step",
                 "test_guard_bands_and_placement", "test_pack_conv_weight_is_guarded", "test_pack_conv_weight_c3_is_guarded",
                 "test_resnet_handle_forward", "test_resnet_handle_forward_bf16", "test_family_handle_forward",
                 "test_siamese_u8_unfused_stem", "test_embed_and_match_and_search"]


def _tests_of(filename):
    with open(os.path.join(HERE, filename)) as f:
        tree = ast.parse(f.read())
    return {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def _uses_two_fills(filename, name):
    with open(os.path.join(HERE, filename)) as f:
        tree = ast.parse(f.read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name][0]
    return any(isinstance(n, ast.Attribute) and n.attr == "two_fills" for n in ast.walk(fn)) or \
        any(isinstance(n, ast.Name) and n.id == "_rule" for n in ast.walk(fn))


def test_capturable_names_every_mirrored_test_and_nothing_else():
    mirrored = {"test_guard_bands_and_placement"}                   # test_tally_gpu.py and test_ovr_gpu.py
    for filename, left_out in SOURCES.items():
        names = _tests_of(filename)
        assert left_out <= names, (filename, left_out - names)
        for n in names - left_out:
            assert _uses_two_fills(filename, n), (filename, n, "does not reach guard.two_fills: it cannot be mirrored")
        mirrored |= names - left_out
    for filename in ("test_tally_gpu.py", "test_ovr_gpu.py"):
        assert _uses_two_fills(filename, "test_guard_bands_and_placement")
    assert set(sc.CAPTURABLE) == mirrored, (sorted(set(sc.CAPTURABLE) - mirrored), sorted(mirrored - set(sc.CAPTURABLE)))


def test_what_the_header_or_the_graphed_step_relies_on_is_capturable():
    for name in REQUIRED_TRUE:
        assert sc.CAPTURABLE[name] is True, (name, sc.CAPTURABLE[name])
    for name, why in sc.CAPTURABLE.items():
        assert why is True or (isinstance(why, str) and ("ops." in why or "resize.py:" in why)), (name, why)
    assert set(sc.SYNCS) == {n for n, why in sc.CAPTURABLE.items() if why is not True}


def test_blind_names_only_mirrored_tests():
    for key, why in sc.BLIND.items():
        assert key.split("[")[0].split(":")[0] in sc.CAPTURABLE and isinstance(why, str) and why, key
    assert "test_match_top1_empty_gallery" in sc.BLIND
    assert set(sc.VARIANT) <= set(sc.CAPTURABLE)


def _operands():
    g = torch.Generator().manual_seed(3)
    return [torch.randn((5, 7), generator=g), torch.randn((1, 7), generator=g), torch.randn((1,), generator=g),
            torch.randn((1, 3, 4, 6), generator=g).to(torch.float16), torch.randn((4, 3), generator=g).to(torch.bfloat16),
            torch.randint(0, 9, (6,), generator=g).to(torch.int32), torch.randint(0, 9, (1,), generator=g),
            torch.randint(0, 256, (2, 3, 3), generator=g).to(torch.uint8), torch.randint(0, 256, (1, 3, 3), generator=g).to(torch.uint8),
            torch.zeros((0, 4)), torch.randint(0, 5, (3, 2), generator=g).to(torch.int64)]


@pytest.mark.parametrize("test", [None, "test_verify_counts", "test_track_step"])
def test_variant_is_deterministic_and_keeps_shape_dtype_and_integer_values(test):
    for k, t in enumerate(_operands()):
        keep = t.clone()
        a, b = sc.variant(t, k, test or "no such test"), sc.variant(t, k, test or "no such test")
        assert torch.equal(t, keep), "the operand itself was changed"
        assert a.shape == t.shape and a.dtype == t.dtype and (t.numel() == 0 or a.data_ptr() != t.data_ptr())
        assert torch.equal(a, b)
        if not t.is_floating_point() and t.dtype != torch.uint8:
            assert sorted(a.reshape(-1).tolist()) == sorted(t.reshape(-1).tolist())
        if t.numel() and (t.is_floating_point() or t.dtype == torch.uint8):
            assert not torch.equal(a, t), (k, "the variant of a float or image operand must differ")
        if t.is_floating_point():
            assert bool(torch.isfinite(a.float()).all())


def test_ascending_thresholds_stay_ascending_and_boxes_stay_boxes():
    thr = torch.tensor([1e-4, 0.5, 1.0, 1.3, 1.5, 2.5])
    v = sc.variant(thr, 2, "test_verify_counts")
    assert torch.equal(v, thr * 0.5) and bool((v[1:] > v[:-1]).all()) and bool((v >= 0).all())
    boxes = torch.tensor([[[10.0, 20.0, 30.0, 50.0], [1.0, 2.0, 3.0, 4.0]]])
    for b in (boxes, boxes.repeat(3, 1, 1) + torch.arange(3.0).view(3, 1, 1)):
        v = sc.variant(b, 0, "test_track_step")
        assert bool((v[..., 2] >= v[..., 0]).all()) and bool((v[..., 3] >= v[..., 1]).all())


@pytest.mark.parametrize("ms", [250.001, 1000.0, 0.0, -1.0, float("inf")])
def test_delay_rejects_a_request_outside_its_bounds(ms):
    with pytest.raises(ValueError, match="bounded spin"):
        sc.delay(None, ms)
    assert sc.CAP_MS == 250.0
