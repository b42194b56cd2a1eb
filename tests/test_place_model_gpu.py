"""GPU: the model handles where their buffers start.

1. The two-fill tests of `test_guard_model_gpu.py` - `frmap_model_forward` of every family and selector at the sizes that take the
   second-generation fused stem, the other fused stem and the unfused one, fp32 and uint8 input; `frmap_model_embed_and_match` /
   `_embed_and_search` with scanned and packed galleries - run again under `guard.shifted`: x aligned to 16 bytes and not to 32
   (fp32) or to 4 and not to 8 (uint8), the gallery, its pack and emb_out to 16, the per-probe results to 4, the workspace (which the
   header wants 256-byte aligned) where it was, the uint8 gallery pack (`MatchPack`, fetched by LDS-DMA) to 16.  Bands untouched, bits those of the aligned call.  Taken: every case of
   `test_resnet_handle_forward` for B = 3, `test_resnet_handle_forward_bf16`, `test_family_handle_forward` for B = 3 fp32 and B = 1
   uint8, `test_siamese_u8_unfused_stem`, `test_embed_and_match_and_search` without the normalise step (G = 36 and 600); left out:
   their B = 1 twins and the normalise twins, which launch the same kernels on fewer rows.
2. The stem a forward takes follows the POINTER: on a 64 x 64 fp32 batch `frmap_model_trace` names `stem_s2d_kernel` for x at 16
   bytes and `stem_pool_kernel` for the same image at 4 (where `frmap_stem_s2d` declines it); each embedding holds the bits of
   the unguarded call at the same alignment (the two stems sum in different orders: `test_place_conv_gpu.py`, the exception).
3. The second half of a batch of an odd-sized image (`x[B/2:]` of 4 x 3 x 225 x 231 floats starts 8 bytes past a multiple of 16)
   gives the bits of the call on its clone, for every output selector (what those bits ARE against the float64 twin is
   `test_model_twin_gpu.py`'s business, on aligned tensors; equal bits carry its verdict over).
4. The selection of 1 once more on one-element-offset views (x, gallery, labels), and x at exactly its documented alignment handed
   to `frmap_model_forward` itself: fp32 at 4 bytes for the baseline family and the wide-input trunk (the layout kernel's one-pixel
   path, even H * W included), uint8 at 1 byte where the byte-wise normalise kernel reads it.
5. The handle's own refusals: x, out, gallery, gallery_packed, gallery_stat, emb_out and workspace of the three calls, each moved
   by half its requirement inside device memory the test owns: -1, a text that names the argument, a clean device, nothing written.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import place_cases as pc  # noqa: E402
import test_guard_model_gpu as tm  # noqa: E402
from frmap_amd import _lib, ops, synth  # noqa: E402

DEV = "cuda"


def _shifted(fn, *args):
    with pc.at_minimum_alignment():
        return fn(*args)


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("H,W", [(64, 64), (61, 37), (16, 232)], ids=["64x64-s2d-stem", "61x37-other-fused-stem", "16x232-unfused-stem"])
@pytest.mark.parametrize("mt", ["cnn", "arcface"])
def test_resnet_handle_forward_at_minimum_alignment(calibrated_sd, mt, H, W, u8):
    _shifted(tm.test_resnet_handle_forward, calibrated_sd, mt, 3, H, W, u8)


def test_resnet_handle_forward_bf16_at_minimum_alignment(calibrated_sd):
    _shifted(tm.test_resnet_handle_forward_bf16, calibrated_sd)


@pytest.mark.parametrize("B,u8", [(3, False), (1, True)], ids=["B3-fp32", "B1-u8"])
@pytest.mark.parametrize("mt", ["baseline", "siamese", "hybrid"])
def test_family_handle_forward_at_minimum_alignment(calibrated_sd, mt, B, u8):
    _shifted(tm.test_family_handle_forward, calibrated_sd, mt, B, u8)


def test_siamese_u8_unfused_stem_at_minimum_alignment(calibrated_sd):
    _shifted(tm.test_siamese_u8_unfused_stem, calibrated_sd)


@pytest.mark.parametrize("G", [36, 600])
@pytest.mark.parametrize("mt,B,HW", tm.MATCH_MODELS, ids=[m[0] for m in tm.MATCH_MODELS])
def test_embed_and_match_and_search_at_minimum_alignment(calibrated_sd, mt, B, HW, G):
    _shifted(tm.test_embed_and_match_and_search, calibrated_sd, mt, B, HW, G, False)


# ---------------------------------------------------------------------------------------------------------------------------------
# the same selection with every placed operand (x, the gallery, the labels) a view one element into its allocation: an fp32 x is
# then 4- and not 8-byte aligned and goes to the library as it is, a uint8 x is one byte in (copied where the fused uint8 stem
# would take it), the gallery is copied for the matcher while its pack is still recognised by the caller's tensor
# ---------------------------------------------------------------------------------------------------------------------------------
# NOT taken here: an fp32 image with W % 4 == 0 in front of the 3x3-pool ResNet stem (cnn / arcface at 64 x 64, hybrid at 224 x 224,
# the fp32 cnn match).  At 4 bytes that stem runs its other kernel, whose sums differ in the last place from the aligned call's
# (the one exception, `test_place_conv_gpu.py`); `test_the_stem_follows_the_pointer` below holds that case to the call at the same alignment.
def _offset(fn, *args):
    with pc.on_offset_views():
        return fn(*args)


RESNET_OFFSET = [(H, W, u8) for (H, W) in ((64, 64), (61, 37), (16, 232)) for u8 in (False, True) if (H, W, u8) != (64, 64, False)]


@pytest.mark.parametrize("H,W,u8", RESNET_OFFSET, ids=["%dx%d-%s" % (h, w, "u8" if u else "fp32") for h, w, u in RESNET_OFFSET])
@pytest.mark.parametrize("mt", ["cnn", "arcface"])
def test_resnet_handle_forward_on_offset_views(calibrated_sd, mt, H, W, u8):
    _offset(tm.test_resnet_handle_forward, calibrated_sd, mt, 3, H, W, u8)


FAMILY_OFFSET = [("baseline", 3, False), ("siamese", 3, False), ("baseline", 1, True), ("siamese", 1, True), ("hybrid", 1, True)]


@pytest.mark.parametrize("mt,B,u8", FAMILY_OFFSET, ids=["%s-B%d-%s" % (m, b, "u8" if u else "fp32") for m, b, u in FAMILY_OFFSET])
def test_family_handle_forward_on_offset_views(calibrated_sd, mt, B, u8):
    _offset(tm.test_family_handle_forward, calibrated_sd, mt, B, u8)


def test_siamese_u8_unfused_stem_on_offset_views(calibrated_sd):
    _offset(tm.test_siamese_u8_unfused_stem, calibrated_sd)


@pytest.mark.parametrize("G", [36, 600])
@pytest.mark.parametrize("mt,B,HW", tm.MATCH_MODELS[1:4], ids=[m[0] for m in tm.MATCH_MODELS[1:4]])
def test_embed_and_match_and_search_on_offset_views(calibrated_sd, mt, B, HW, G):
    _offset(tm.test_embed_and_match_and_search, calibrated_sd, mt, B, HW, G, False)


FOUR_BYTE_CASES = [("baseline", 64, 64, False), ("baseline", 61, 37, False), ("baseline", 64, 64, True), ("cnn", 16, 232, False),
                   ("cnn", 16, 232, True), ("siamese", 64, 520, False), ("siamese", 64, 520, True)]


@pytest.mark.parametrize("mt,H,W,u8", FOUR_BYTE_CASES, ids=["%s-%dx%d-%s" % (m, h, w, "u8" if u else "fp32") for m, h, w, u in FOUR_BYTE_CASES])
def test_x_at_its_documented_alignment_is_taken_as_it_is(calibrated_sd, mt, H, W, u8):
    """x exactly as loose as the header allows, between guard bands, handed to the C entry point itself (no copy can hide a refusal):
    fp32 at 4 bytes and not 8 - the layout kernel of a baseline forward and of the wide-input trunk then takes its one-pixel path,
    an even H * W included; uint8 at 1 byte and not 2 where the byte-wise normalise kernel reads it (baseline, inputs wider than the
    fused stems) .  Every selector: rc 0, bands untouched, the bits of the aligned call."""
    h = tm._handle(calibrated_sd, mt)
    B = 2
    x = tm._input(300 + H + W, B, H, W, u8)
    need = 1 if u8 else 4
    for what in tm.SELECTORS[mt]:
        want = h.forward(x.to(DEV), what).cpu()
        for fill in guard.FILLS:
            g = guard.Guard(fill, shift=guard.min_placement(lambda d, kind, who: need if kind == "operand" else pc.requirement(d, kind, who)))
            xd = g.place(x)
            assert xd.data_ptr() % (2 * need) == need
            with g.patch(ops):
                out = torch.empty_like(want, device=DEV)
                ws = torch.empty((h._lib.frmap_model_workspace_bytes(h._h, B, H, W),), dtype=torch.uint8, device=DEV)
                rc = h._lib.frmap_model_forward(h._h, xd.data_ptr(), ops.IN_U8_HWC if u8 else ops.IN_F32_NCHW, B, H, W, what, out.data_ptr(),
                                                ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, (mt, what, h._lib.frmap_last_error().decode())
            g.check()
            assert guard.first_difference(out.cpu(), want) is None, (mt, what, fill, guard.first_difference(out.cpu(), want))


# ---------------------------------------------------------------------------------------------------------------------------------
def _at(x_cpu, need):
    """(guard, x on the device aligned to `need` and not to 2 `need`)"""
    g = guard.Guard(0x5A, shift=guard.min_placement(need))
    xd = g.place(x_cpu)
    assert xd.data_ptr() % (2 * need) == need
    return g, xd


def test_the_stem_follows_the_pointer(calibrated_sd):
    h = tm._handle(calibrated_sd, "cnn")
    x = synth.randn(171, (3, 3, 64, 64), "g.x")
    # (the two stems sum in different orders - `test_place_conv_gpu.py`, the exception: each placement meets the bits of the
    #  unguarded call at the same alignment)
    want = {16: h.forward(x.to(DEV), ops.OUT_EMBEDDING).cpu(), 4: h.forward(pc.offset_view(x, DEV), ops.OUT_EMBEDDING).cpu()}
    assert torch.allclose(want[4], want[16], atol=2e-2, rtol=2e-2)       # (a smoke bound only: the stems' own bound is tested on the stems)
    for need, kernel in ((16, "stem_s2d_kernel"), (4, "stem_pool_kernel")):
        g, xd = _at(x, need)
        h.trace(True)
        try:
            got = h.forward(xd, ops.OUT_EMBEDDING).cpu()
            labels = [r[0] for r in h.trace_read()]
        finally:
            h.trace(False)
        g.check()
        assert labels and labels[0].startswith(kernel), (need, labels[:2])
        assert guard.first_difference(got, want[need]) is None, (need, guard.first_difference(got, want[need]))


def test_second_half_of_a_batch_of_odd_sized_images(calibrated_sd):
    h = tm._handle(calibrated_sd, "cnn")
    B, H, W = 4, 225, 231
    x = synth.randn(5000 + H, (B, 3, H, W), "sz").to(DEV)
    half = x[B // 2:]
    assert half.is_contiguous() and half.data_ptr() % 16 == 8
    for what in tm.SELECTORS["cnn"]:
        a, b = h.forward(half, what), h.forward(half.clone(), what)
        assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all()), what


# ---------------------------------------------------------------------------------------------------------------------------------
MODEL_REJECTS = [(e, a, n) for e in ("frmap_model_forward", "frmap_model_embed_and_match", "frmap_model_embed_and_search")
                 for a, (_, n) in _lib.ALIGNMENT[e].items() if pc.needs_rejection_test(e, a)]


@pytest.mark.parametrize("entry,arg,need", MODEL_REJECTS, ids=["%s-%s" % (e[12:], a) for e, a, _ in MODEL_REJECTS])
def test_the_handle_refuses_a_pointer_below_its_requirement(calibrated_sd, entry, arg, need):
    h = tm._handle(calibrated_sd, "cnn")
    B, H, W, G = 1, 64, 64, 600
    nbytes = max(h._lib.frmap_model_search_workspace_bytes(h._h, B, H, W, G, 2), G * 512 * 4 * 2) + 512
    g = guard.Guard(0x5A, band=4096)
    p = {a: g.empty((nbytes,), torch.uint8).data_ptr() for a in _lib.ALIGNMENT[entry]}
    p[arg] += max(need // 2, pc.element_size(entry, arg))
    st = torch.cuda.current_stream().cuda_stream
    if entry == "frmap_model_forward":
        rc = h._lib.frmap_model_forward(h._h, p["x"], ops.IN_F32_NCHW, B, H, W, ops.OUT_TRUNK_MAP, p["out"], p["workspace"], st)
    elif entry == "frmap_model_embed_and_match":
        rc = h._lib.frmap_model_embed_and_match(h._h, p["x"], ops.IN_F32_NCHW, B, H, W, p["gallery"], p["gallery_packed"], p["gallery_stat"], G,
                                                1.0, 0, p["idx_out"], p["dist_out"], p["id_or_unknown_out"], p["packed_out"], p["emb_out"],
                                                p["workspace"], st)
    else:
        rc = h._lib.frmap_model_embed_and_search(h._h, p["x"], ops.IN_F32_NCHW, B, H, W, p["gallery"], p["gallery_packed"], p["gallery_stat"],
                                                 p["labels"], G, 2, 0, p["idx_out"], p["dist_out"], p["label_out"], p["emb_out"],
                                                 p["workspace"], st)
    msg = h._lib.frmap_last_error().decode()
    assert rc == -1 and (" %s must be %d-byte aligned" % (arg, need)) in msg and msg.startswith(entry[6:] + ": "), (rc, msg)
    torch.cuda.synchronize()
    g.check()
    for a in g.allocs:
        assert bool((a.raw == 0x5A).all()), (entry, arg, a.describe())
