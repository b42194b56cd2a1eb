"""GPU: the model handles (`frmap_model_forward`, `_embed_and_match`, `_embed_and_search`) between guard bands (`guard.py`),
reached through `ops.ModelHandle`, so that the workspace is exactly `frmap_model_workspace_bytes` (`_match_` / `_search_`) with
the rear band at its last byte.  Expected values are the unguarded call's bits (the two-fill rule); model parity is tested in
`test_models_gpu.py` / `test_model_cabi_gpu.py`.  Weights live in memory the library allocates for itself (not guarded).

The workspace is cut as `ModelWs` in `model_api.cpp` states it (one struct, filled by `model_ws`, read by the three
`*_workspace_bytes` functions and by every forward).  Which launch first writes and first reads each field:
  slot 0..2     ResNet trunks.  slot 0: the fused stem (or the max-pool of the unfused one) writes it; slot 1: `pack_input` /
                `normalize_u8_hwc` (NHWC4 input); slot 2: the 7x7 conv of the unfused stem.  Each block reads `buf[cur]` and
                writes the other two; every later map is at most half of the 7x7 conv's.
  tokens        hybrid: the last trunk block writes it (`final_out`) / `add_pos_layernorm` reads it
  arena         `Arena::take`: every buffer is an output of the launch that follows its `take` and an input of later launches
                only; `linear` takes its split-K slab from the arena at `frmap_linear_mfma_workspace_bytes`.  Sized by the same
                code run dry for both input kinds: a siamese tower takes uint8 rows of W % 4 != 0 through the unfused stem,
                through more buffers than the fp32 call of the same size (`test_siamese_u8_unfused_stem`).
  scratch0, 1   cnn logits: `avgpool_global` writes scratch0 / `linear_f32` reads; arcface logits: `gap_linear_norm` writes /
                `linear_f32` reads; match: scratch1 = the pooled row or the family's own embedding, scratch0 = its unit-norm copy
  match, split  the matcher's fields as `test_guard_ops_gpu.py` lists them; the split is written by the packed top-1's first launch
No field is read before it is written.  A baseline / siamese trunk map is [B, 28, 28, 128] / [B, 14, 14, 512] at 224 x 224, not a
ResNet's [B, 7, 7, 512] (`ops.ModelHandle.forward` sizes it).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
from frmap_amd import evaluate, ops, synth  # noqa: E402

IMAGENET_MEAN, IMAGENET_STD = evaluate.IMAGENET_MEAN, evaluate.IMAGENET_STD

DEV = "cuda"
NUM_CLASSES = 36
_handles = {}


def _handle(calibrated_sd, mt, dtype=torch.float16):
    if (mt, dtype) not in _handles:
        sd = {k: v.to(DEV) for k, v in calibrated_sd(mt).items()}
        _handles[(mt, dtype)] = ops.ModelHandle(mt, sd, NUM_CLASSES, dtype, IMAGENET_MEAN, IMAGENET_STD)
        torch.cuda.synchronize()
    return _handles[(mt, dtype)]


def _input(seed, B, H, W, u8):
    if u8:
        g = torch.Generator().manual_seed(seed)
        return torch.randint(0, 256, (B, H, W, 3), generator=g).to(torch.uint8)
    return synth.randn(seed, (B, 3, H, W), "g.x")


def _rule(run, what):
    return guard.two_fills(run, [ops], what=what)


def _workspace_allocs(run, want_bytes, who):
    """Run once more under a guard and return the sizes the wrapper asked for: the workspace must be `want_bytes` exactly."""
    g = guard.Guard(0x5A)
    with g.patch(ops):
        run(g.place)
    g.check()
    sizes = [a.nbytes for a in g.allocs if a.who == who and a.dtype == torch.uint8 and a.kind == "empty"]
    assert want_bytes in sizes, (who, want_bytes, sizes)


SELECTORS = {"cnn": (ops.OUT_TRUNK_MAP, ops.OUT_POOLED, ops.OUT_EMBEDDING, ops.OUT_LOGITS),
             "arcface": (ops.OUT_TRUNK_MAP, ops.OUT_POOLED, ops.OUT_EMBEDDING, ops.OUT_LOGITS),
             "baseline": (ops.OUT_TRUNK_MAP, ops.OUT_EMBEDDING, ops.OUT_LOGITS),
             "siamese": (ops.OUT_TRUNK_MAP, ops.OUT_EMBEDDING),
             "hybrid": (ops.OUT_TRUNK_MAP, ops.OUT_POOLED, ops.OUT_EMBEDDING, ops.OUT_LOGITS)}


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("H,W", [(64, 64), (61, 37), (16, 232)], ids=["64x64-s2d-stem", "61x37-other-fused-stem", "16x232-unfused-stem"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("mt", ["cnn", "arcface"])
def test_resnet_handle_forward(calibrated_sd, mt, B, H, W, u8):
    h = _handle(calibrated_sd, mt)
    x = _input(70 + B, B, H, W, u8)
    for what in SELECTORS[mt]:
        _rule(lambda place: h.forward(place(x), what), f"{mt} forward what={what}")
    ws = h._lib.frmap_model_workspace_bytes(h._h, B, H, W)
    _workspace_allocs(lambda place: h.forward(place(x), ops.OUT_LOGITS), ws, "ops.forward")


def test_resnet_handle_forward_bf16(calibrated_sd):
    h = _handle(calibrated_sd, "arcface", torch.bfloat16)
    x = _input(75, 3, 61, 37, False)
    for what in SELECTORS["arcface"]:
        _rule(lambda place: h.forward(place(x), what), f"arcface bf16 forward what={what}")


@pytest.mark.parametrize("B,u8", [(1, False), (3, False), (1, True)], ids=["B1-fp32", "B3-fp32", "B1-u8"])
@pytest.mark.parametrize("mt", ["baseline", "siamese", "hybrid"])
def test_family_handle_forward(calibrated_sd, mt, B, u8):
    h = _handle(calibrated_sd, mt)
    x = _input(80 + B, B, 224, 224, u8)
    for what in SELECTORS[mt]:
        out, = _rule(lambda place: h.forward(place(x), what), f"{mt} forward what={what}")
        if what == ops.OUT_TRUNK_MAP:
            assert tuple(out.shape) == {"baseline": (B, 28, 28, 128), "siamese": (B, 14, 14, 512), "hybrid": (B, 7, 7, 512)}[mt]
    ws = h._lib.frmap_model_workspace_bytes(h._h, B, 224, 224)
    _workspace_allocs(lambda place: h.forward(place(x), ops.OUT_EMBEDDING), ws, "ops.forward")


def test_siamese_u8_unfused_stem(calibrated_sd):
    """uint8 rows of W % 4 != 0 take the unfused stem, through more arena than the fp32 call of the same size."""
    h = _handle(calibrated_sd, "siamese")
    x = _input(85, 2, 64, 62, True)
    _rule(lambda place: h.forward(place(x), ops.OUT_EMBEDDING), "siamese u8 64x62")
    assert h._lib.frmap_model_workspace_bytes(h._h, 2, 64, 62) > h._lib.frmap_model_workspace_bytes(h._h, 2, 64, 64)


MATCH_MODELS = [("cnn", 3, 64), ("arcface", 3, 64), ("baseline", 1, 224), ("siamese", 1, 224), ("hybrid", 1, 224)]


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalize"])
@pytest.mark.parametrize("G", [36, 600])
@pytest.mark.parametrize("mt,B,HW", MATCH_MODELS, ids=[m[0] for m in MATCH_MODELS])
def test_embed_and_match_and_search(calibrated_sd, mt, B, HW, G, normalize):
    h = _handle(calibrated_sd, mt)
    D = h.embedding_dim
    x = _input(90 + G, B, HW, HW, mt == "arcface")
    gal = synth.unit_rows(91, G, D, "g.gal")
    labels = (torch.arange(G, dtype=torch.int32) * 7) % 12

    def prepared(g):
        return ops.match_prepare(g) if ops.wants_pack(G, D) else None

    def match(place):
        g = place(gal)
        return h.embed_and_match(place(x), g, prepared(g), 1.1, normalize, packed=True, want_emb=True)

    def search(place):
        g = place(gal)
        return h.embed_and_search(place(x), g, prepared(g), 5, place(labels), normalize, want_emb=True)

    def search1(place):
        g = place(gal)
        return h.embed_and_search(place(x), g, prepared(g), 1, None, normalize)
    m = _rule(match, f"{mt} embed_and_match G={G}")
    _rule(search, f"{mt} embed_and_search G={G}")
    s1 = _rule(search1, f"{mt} embed_and_search k=1 G={G}")
    assert guard.first_difference(m[0], s1[0][:, 0].contiguous()) is None                  # k = 1 is the top-1 step itself
    _workspace_allocs(match, h._lib.frmap_model_match_workspace_bytes(h._h, B, HW, HW, G), "ops.embed_and_match")
    _workspace_allocs(search, h._lib.frmap_model_search_workspace_bytes(h._h, B, HW, HW, G, 5), "ops.embed_and_search")
