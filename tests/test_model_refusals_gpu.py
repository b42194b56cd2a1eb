"""GPU: what the three model-handle entry points refuse, with the exact text of each refusal.

`frmap_model_forward`, `_embed_and_match` and `_embed_and_search` on a finalized fp16 handle (B = 1 at 64 x 64: every case is
refused before a launch), every buffer from `guard.Guard(0x5A)` as `test_the_handle_refuses_a_pointer_below_its_requirement`
(`test_place_model_gpu.py`) has them.  Each case: the return code, the whole text of `frmap_last_error`, a clean device after
`torch.cuda.synchronize()`, every guarded byte still 0x5A.  With two faults in one call the header promises nothing about which
is reported; these cases have one fault each, except where a case says otherwise.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import test_guard_model_gpu as tm  # noqa: E402
from frmap_amd import _lib, ops  # noqa: E402

FORWARD, MATCH, SEARCH = "frmap_model_forward", "frmap_model_embed_and_match", "frmap_model_embed_and_search"
B, H, W, G = 1, 64, 64, 36
UNFINALIZED, NULL = "unfinalized", "null"
TOKENS = "HybridNet expects a 49-token feature map (224x224 input), got 4"        # 64 x 64 -> a 2 x 2 trunk map


def _trunk_handle(calibrated_sd):
    if ("resnet18_trunk", torch.float16) not in tm._handles:
        sd = {k: v.to(tm.DEV) for k, v in calibrated_sd("cnn").items()}
        tm._handles[("resnet18_trunk", torch.float16)] = ops.ModelHandle("resnet18_trunk", sd, 0, torch.float16, tm.IMAGENET_MEAN, tm.IMAGENET_STD)
        torch.cuda.synchronize()
    return tm._handles[("resnet18_trunk", torch.float16)]


def _shape(entry, **kw):
    """The text of the entry point's shape refusal for the case's B, H, W (and G)."""
    a = {"B": B, "H": H, "W": W, "G": G, **kw}
    return ("bad shape B=%d H=%d W=%d" % (a["B"], a["H"], a["W"])) + ("" if entry == FORWARD else " G=%d" % a["G"])


# (entry, model | NULL | UNFINALIZED, arguments changed from the good call, the text after "<entry without frmap_>: ")
CASES = []
for e in (FORWARD, MATCH, SEARCH):
    CASES += [(e, NULL, {}, "null model"),
              (e, UNFINALIZED, {}, "frmap_model_finalize has not run"),
              (e, "cnn", {"x": 0}, "null pointer"),
              (e, "cnn", {"workspace": 0}, "null pointer"),
              (e, "cnn", {"B": 0}, _shape(e, B=0)),
              (e, "cnn", {"H": 6}, _shape(e, H=6)),
              (e, "cnn", {"x_kind": 2}, "bad input kind 2"),
              (e, "hybrid", {}, TOKENS)]
CASES += [(FORWARD, "cnn", {"out": 0}, "null pointer"),
          (FORWARD, "cnn", {"what": 4}, "bad output selector 4"),
          (FORWARD, "cnn", {"what": -1}, "bad output selector -1"),
          (FORWARD, "resnet18_trunk", {"what": ops.OUT_EMBEDDING}, "a bare trunk has no embedding / logits head"),
          (FORWARD, "baseline", {"what": ops.OUT_POOLED}, "'baseline' has no pooled-trunk output"),
          (FORWARD, "siamese", {"what": ops.OUT_POOLED}, "'siamese' has no pooled-trunk output"),
          (FORWARD, "siamese", {"what": ops.OUT_LOGITS}, "'siamese' has no classifier head (forward(x1, x2) = two embeddings)")]
for e in (MATCH, SEARCH):
    CASES += [(e, "cnn", {"idx_out": 0}, "null pointer"),
              (e, "cnn", {"dist_out": 0}, "null pointer"),
              (e, "resnet18_trunk", {}, "a bare trunk has no embedding"),
              (e, "cnn", {"G": -1}, _shape(e, G=-1)),
              (e, "cnn", {"gallery": 0}, _shape(e))]
CASES += [(SEARCH, "cnn", {"k": 0}, "k=0 out of range (1 <= k <= 64)"),
          (SEARCH, "cnn", {"k": 65}, "k=65 out of range (1 <= k <= 64)"),
          # k = 1 without labels is the top-1 step itself: the call is handed on, and the refusal carries that entry point's name
          (SEARCH, "hybrid", {"k": 1, "labels": 0}, "model_embed_and_match: " + TOKENS)]


def _id(c):
    return "%s-%s-%s" % (c[0][12:], c[1], "-".join("%s=%s" % kv for kv in c[2].items()) or "as-it-is")


@pytest.mark.parametrize("entry,mt,changed,text", CASES, ids=[_id(c) for c in CASES])
def test_the_handle_refuses_a_bad_request(calibrated_sd, entry, mt, changed, text):
    lib = _lib.load()
    fresh = C.c_void_p()
    if mt == NULL:
        hptr = None
    elif mt == UNFINALIZED:
        assert lib.frmap_model_create(C.byref(fresh), b"cnn", tm.NUM_CLASSES, ops.dt_code(torch.float16)) == 0
        hptr = fresh
    else:
        hptr = (_trunk_handle(calibrated_sd) if mt == "resnet18_trunk" else tm._handle(calibrated_sd, mt))._h
    any_h = tm._handle(calibrated_sd, "cnn")
    nbytes = max(lib.frmap_model_search_workspace_bytes(any_h._h, B, H, W, G, 5), lib.frmap_model_search_workspace_bytes(hptr, B, H, W, G, 5),
                 G * 512 * 4, B * 3 * H * W * 4) + 512
    g = guard.Guard(0x5A, band=4096)
    a = {n: g.empty((nbytes,), torch.uint8).data_ptr() for n in _lib.ALIGNMENT[entry]}
    a.update(x_kind=ops.IN_F32_NCHW, B=B, H=H, W=W, G=G, k=5, what=ops.OUT_EMBEDDING)
    a.update(changed)
    st = torch.cuda.current_stream().cuda_stream
    try:
        if entry == FORWARD:
            rc = lib.frmap_model_forward(hptr, a["x"], a["x_kind"], a["B"], a["H"], a["W"], a["what"], a["out"], a["workspace"], st)
        elif entry == MATCH:
            rc = lib.frmap_model_embed_and_match(hptr, a["x"], a["x_kind"], a["B"], a["H"], a["W"], a["gallery"], a["gallery_packed"],
                                                 a["gallery_stat"], a["G"], 1.0, 0, a["idx_out"], a["dist_out"], a["id_or_unknown_out"],
                                                 a["packed_out"], a["emb_out"], a["workspace"], st)
        else:
            rc = lib.frmap_model_embed_and_search(hptr, a["x"], a["x_kind"], a["B"], a["H"], a["W"], a["gallery"], a["gallery_packed"],
                                                  a["gallery_stat"], a["labels"], a["G"], a["k"], 0, a["idx_out"], a["dist_out"],
                                                  a["label_out"], a["emb_out"], a["workspace"], st)
        msg = lib.frmap_last_error().decode()
    finally:
        if fresh:
            lib.frmap_model_destroy(fresh)
    want = text if text.startswith("model_") else entry[6:] + ": " + text
    print(rc, msg)
    assert rc == -1 and msg == want, (rc, msg, want)
    torch.cuda.synchronize()
    g.check()
    for al in g.allocs:
        assert bool((al.raw == 0x5A).all()), (entry, mt, changed, al.describe())
