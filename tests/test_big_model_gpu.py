"""GPU: the `cnn` model (the `frmap_model` handle behind `face_models`' `get_embedding`, `frmap_model_forward`) at the smallest batch
whose first activation (112 x 112 x 64 two-byte elements a face: 1.6 MB) passes 4 GiB by two periods: 2,689 faces of 224 x 224.
Each of the arena's three activation slots then passes 2^32 bytes and 2^31 elements, and `frmap_model_workspace_bytes` - what the
Python side allocates, a `size_t` in `_lib.py` - passes 2^33.

Inputs of period 7 (`big_cases.tile_on_device`), batch-invariant planning on (every layer's kernel and layout follow from the
per-image geometry, so a face's embedding does not depend on the batch it is in): the embeddings are periodic bit for bit and the
first 7 are the bits of the B = 7 run, whose accuracy against the oracle is the business of test_models_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import big_cases as bc  # noqa: E402
import frmap_amd  # noqa: E402
import guard  # noqa: E402
from frmap_amd import _lib, ops  # noqa: E402
from oracle import weights  # noqa: E402

DEV = "cuda"
K = bc.K
H = W = 224
ACT = bc.Operand("first activation", 112 * 112 * 64 * 2, 2)
X = bc.Operand("x", 3 * H * W * 4, 4)


@pytest.mark.parametrize("dtype", [torch.float16], ids=["fp16"])
def test_cnn_embeddings_are_periodic_past_4gib(dtype, calibrated_sd):
    B = bc.smallest_batch([ACT])
    assert B == 2 ** 32 // ACT.item_bytes + 15 == 2689 and bc.crosses(B, ACT)
    bc.assert_period(ACT.item_bytes, 2)
    bc.assert_period(X.item_bytes, 4)
    lib = _lib.load()
    ops.set_batch_invariant(True)
    try:
        m = frmap_amd.get_model("cnn", 36)
        m.load_state_dict(calibrated_sd("cnn"))
        m = m.to(DEV).eval().set_compute_dtype(dtype)
        handle = m.model_handle()
        assert handle is not None
        ws_bytes = lib.frmap_model_workspace_bytes(handle._h, B, H, W)
        assert ws_bytes > 2 ** 33 and ws_bytes >= 3 * B * ACT.item_bytes, ws_bytes     # three slots, each past 2^32
        bc.need_memory(bc.estimate_bytes([ws_bytes, B * X.item_bytes, B * 512 * 4]), "cnn model")
        x7 = weights.golden_inputs("cnn", K).to(DEV)
        with torch.no_grad():
            emb7 = m.get_embedding(x7)
            assert tuple(emb7.shape) == (K, 512) and bool(torch.isfinite(emb7).all())
            xbig = bc.tile_on_device(x7, B)
            g = guard.Guard(0xFF)
            with g.patch(ops):                  # the output and the arena between bands
                emb = m.get_embedding(xbig)
            g.check()
        assert sorted(a.nbytes for a in g.allocs)[-1] == ws_bytes, "the arena is not what the size query answers"
        print(f"\ncnn {str(dtype)[6:]} B={B}: x {B * X.item_bytes / 2 ** 30:.2f} GiB, arena {ws_bytes / 2 ** 30:.2f} GiB, "
              f"peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
        assert tuple(emb.shape) == (B, 512)
        assert torch.equal(emb[:K].view(torch.int32), emb7.view(torch.int32)), "the first period differs from the B = 7 run"
        bc.assert_periodic(emb, K, what="cnn embeddings")
        bc.assert_operand_intact(xbig, x7, what="cnn input")
    finally:
        ops.set_batch_invariant(None)
        emb = xbig = g = None
        torch.cuda.empty_cache()
