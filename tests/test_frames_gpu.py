"""GPU: the frame front end - `resize.crop_resize_u8` (ROI crop + BGR -> RGB + Pillow-exact resize in one launch, filter taps
computed on the device) bit for bit against Pillow on the sliced array, and `matching.embed_boxes` / `identify_boxes` against the
per-box `get_embedding` + `compare_faces` loop of the reference's frame loop (`src/app.py:224-241`)."""
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import frmap_amd  # noqa: E402
from frmap_amd import _lib, frames, matching, ops, resize, synth  # noqa: E402
from align_cases import pil_crop as _pil  # noqa: E402
from test_configs_gpu import DIST_BOUND  # noqa: E402  (the project's gate on a distance's error per compute dtype)

DEV = "cuda"
_rng = np.random.default_rng(20240611)
# 720p: 16-pixel blocks of random colour under pixel noise - every pixel differs from its neighbours (a one-pixel slip of a window or
# a tap shows) and crops of different places differ as images (their embeddings are distinct).  1080p: noise, one channel a ramp.
F720 = (0.75 * np.kron(_rng.integers(0, 256, (45, 80, 3)), np.ones((16, 16, 1))) + 0.25 * _rng.integers(0, 256, (720, 1280, 3))).astype(np.uint8)
F1080 = _rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
F1080[:, :, 0] = (np.add.outer(np.arange(1080), np.arange(1920)) // 9 % 256).astype(np.uint8)


def _edge_rois(out_h, out_w):
    """[frame, x1, y1, x2, y2] over (F720, F1080): every path of the kernel at the smallest sizes that reach it."""
    return [
        [0, 100, 50, 101, 51],                       # 1 x 1
        [0, 300, 200, 337, 201],                     # 1 row x k columns
        [1, 5, 7, 6, 48],                            # k rows x 1 column (not "tall": 41 <= 100)
        [0, 0, 0, 1280, 720],                        # the full frames (all four edges)
        [1, 0, 0, 1920, 1080],
        [0, 0, 0, 97, 120],                          # top-left corner
        [0, 1280 - 213, 720 - 388, 1280, 720],       # bottom-right corner
        [1, 0, 1080 - 61, 75, 1080],                 # bottom-left
        [1, 1920 - 64, 0, 1920, 59],                 # top-right
        [0, 400, 300, 420, 330],                     # upscale on both axes
        [0, 400, 300, 400 + out_w, 300 + 91],        # width unchanged: horizontal copy
        [1, 900, 500, 900 + 233, 500 + out_h],       # height unchanged: vertical copy
        [1, 11, 13, 11 + out_w, 13 + out_h],         # both unchanged: plain copy (+ channel swap)
        [0, 500, 100, 500 + 2 * out_w, 100 + 2 * out_h],       # exact 2x
        [0, 600, 150, 600 + 388, 150 + 401],         # overlapping boxes of one face ...
        [0, 601, 151, 601 + 388, 151 + 400],         # ... a pixel apart, as in consecutive video frames
        [0, 640, 200, 640 + 250, 200 + 260],
        [1, 200, 100, 200 + 1080, 100 + 901],        # large box in the second frame
    ]


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("size", [(160, 160), (224, 224), (96, 200)])
def test_crop_resize_is_bit_exact_with_pillow(size, bgr):
    out_h, out_w = size
    rois = np.array(_edge_rois(out_h, out_w), dtype=np.int64)
    got = resize.crop_resize_u8([F720, F1080], rois, size, bgr=bgr, device=DEV)     # two host frames of different sizes, one call
    assert got.shape == (len(rois), out_h, out_w, 3) and got.dtype == torch.uint8 and got.is_cuda
    got = got.cpu().numpy()
    fr = (F720, F1080)
    for i, (f, *roi) in enumerate(rois.tolist()):
        assert np.array_equal(got[i], _pil(fr[f], roi, out_h, out_w, bgr)), (i, f, roi)


def test_crop_resize_heaviest_reduction_and_rejection():
    """32x per axis is the largest reduction the header promises for any output up to 224 wide: 1920 -> 60 columns (32x) with
    1080 -> 34 rows (31.8x), and 1088 -> 34 rows would be 32x as well; a reduction whose window cannot fit LDS is rejected."""
    for size, roi in (((34, 60), [0, 0, 1920, 1080]), ((5, 224), [3, 10, 3 + 1800, 10 + 160])):
        got = resize.crop_resize_u8(F1080, np.array([roi]), size, device=DEV).cpu().numpy()
        assert np.array_equal(got[0], _pil(F1080, roi, size[0], size[1], False)), size
    with pytest.raises(ValueError, match="LDS"):
        resize.crop_resize_u8(F1080, np.array([[0, 0, 1920, 1080]]), (2, 1200), device=DEV)   # 540x vertically at 1200 columns


def test_crop_resize_500_rois_of_a_padded_device_frame_and_the_existing_resize():
    """N = 500 ROIs of one device-resident frame whose rows are padded (a view of a wider buffer: pitch > 3 W), BGR; equal to
    Pillow and to `resize_bilinear_u8` on the same slices, bit for bit.  Then [F, H, W, 3] stacks, [N, 5] ROIs and N = 0."""
    buf = torch.full((720, 1280 + 24, 3), 255, dtype=torch.uint8, device=DEV)
    frame = buf[:, 8:8 + 1280]
    frame.copy_(torch.from_numpy(F720).to(DEV))
    assert frame.stride(0) == 3 * (1280 + 24) and frame.data_ptr() != buf.data_ptr()
    rng = np.random.default_rng(7)
    w, h = rng.integers(1, 140, 500), rng.integers(1, 140, 500)
    x1, y1 = rng.integers(0, 1280 - w + 1), rng.integers(0, 720 - h + 1)
    rois = np.stack([x1, y1, x1 + w, y1 + h], 1)
    rois[:4] = [[0, 0, 139, 3], [1280 - 5, 0, 1280, 139], [0, 720 - 139, 2, 720], [1280 - 77, 720 - 90, 1280, 720]]
    got = resize.crop_resize_u8(frame, rois, (160, 160), bgr=True).cpu().numpy()
    assert got.shape == (500, 160, 160, 3)
    for i, roi in enumerate(rois.tolist()):
        assert np.array_equal(got[i], _pil(F720, roi, 160, 160, True)), (i, roi)
    slices = [np.ascontiguousarray(F720[b:d, a:c, ::-1]) for a, b, c, d in rois[:64].tolist()]
    assert torch.equal(resize.resize_bilinear_u8(slices, (160, 160), DEV).cpu(), torch.from_numpy(got[:64]))
    # a stack of frames (host array, device tensor), ROIs with a frame index
    stack = np.stack([F720, F720[::-1].copy(), F720[:, ::-1].copy()])
    r5 = np.array([[2, 10, 20, 110, 150], [0, 10, 20, 110, 150], [1, 1000, 500, 1280, 720]])
    want = np.stack([_pil(stack[f], roi, 112, 112, False) for f, *roi in r5.tolist()])
    assert np.array_equal(resize.crop_resize_u8(stack, r5, (112, 112), device=DEV).cpu().numpy(), want)
    assert np.array_equal(resize.crop_resize_u8(torch.from_numpy(stack).to(DEV), r5, (112, 112)).cpu().numpy(), want)
    # N = 0
    for empty in (np.zeros((0, 4), np.int64), np.zeros((0, 5), np.int32), []):
        e = resize.crop_resize_u8(frame, empty, (224, 160))
        assert e.shape == (0, 224, 160, 3) and e.dtype == torch.uint8 and e.is_cuda


def test_crop_resize_tall_roi_takes_pillows_other_pass_order():
    """A ROI more than 100x taller than wide whose height shrinks: Pillow resizes it in height first; the wrapper routes it through
    `resize_bilinear_u8` on the slice, between ROIs that take the kernel."""
    rois = np.array([[50, 10, 150, 210], [300, 100, 302, 500], [700, 0, 701, 720], [60, 20, 160, 220]])
    assert rois[1][3] - rois[1][1] > 100 * (rois[1][2] - rois[1][0])
    for bgr in (False, True):
        got = resize.crop_resize_u8(F720, rois, (160, 160), bgr=bgr, device=DEV).cpu().numpy()
        for i, roi in enumerate(rois.tolist()):
            assert np.array_equal(got[i], _pil(F720, roi, 160, 160, bgr)), (bgr, i)


def test_crop_resize_rejects_bad_rois_and_frames():
    ok = [10, 10, 50, 50]
    for bad in ([10, 10, 10, 50], [10, 50, 60, 50], [60, 10, 50, 50], [-1, 10, 50, 50], [10, -1, 50, 50], [10, 10, 1281, 50],
                [10, 10, 50, 721]):
        with pytest.raises(ValueError, match="empty or leaves"):
            resize.crop_resize_u8(F720, np.array([ok, bad]), (160, 160), device=DEV)
    with pytest.raises(ValueError, match="frame index"):
        resize.crop_resize_u8(F720, np.array([[1] + ok]), (160, 160), device=DEV)
    with pytest.raises(ValueError):
        resize.crop_resize_u8(F720, np.array([[10.0, 10.0, 50.0, 50.0]]), (160, 160), device=DEV)      # not integers
    with pytest.raises(ValueError):
        resize.crop_resize_u8(F720[:, :, 0], np.array([ok]), (160, 160), device=DEV)                    # not H x W x 3
    with pytest.raises(ValueError):
        resize.crop_resize_u8(F720.astype(np.float32), np.array([ok]), (160, 160), device=DEV)


def test_crop_resize_c_entry_point_rejects_before_any_launch():
    lib = _lib.load()
    frame = torch.from_numpy(F720).to(DEV)
    desc = np.zeros(1, resize.FRAME_DTYPE)
    desc[0] = (frame.data_ptr(), 720, 1280, 3 * 1280)
    fr = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    rois = torch.tensor([[0, 10, 10, 50, 50]], dtype=torch.int32, device=DEV)
    out = torch.zeros((1, 160, 160, 3), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    call = lib.frmap_crop_resize_u8
    good = (fr.data_ptr(), 1, rois.data_ptr(), out.data_ptr(), 1, 160, 160, 720, 1280, 0, st)
    for pos in (0, 2, 3):                                                  # null frames / rois / out
        args = list(good)
        args[pos] = None
        assert call(*args) == -1 and b"null pointer" in lib.frmap_last_error()
    assert call(fr.data_ptr(), 1, rois.data_ptr(), out.data_ptr(), -1, 160, 160, 720, 1280, 0, st) == -1
    assert call(fr.data_ptr(), 0, rois.data_ptr(), out.data_ptr(), 1, 160, 160, 720, 1280, 0, st) == -1
    assert call(fr.data_ptr(), 1, rois.data_ptr(), out.data_ptr(), 1, 160, 160, 1 << 20, 1280, 0, st) == -1
    assert b"LDS" in lib.frmap_last_error()
    assert call(None, 0, None, None, 0, 160, 160, 720, 1280, 0, st) == 0   # N = 0: nothing to do, nothing launched
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                                             # none of the rejected calls wrote anything
    assert call(*good) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), _pil(F720, [10, 10, 50, 50], 160, 160, False))
    # device records the host never sees: one that leaves its frame is skipped by the kernel (nothing read out of bounds)
    rois2 = torch.tensor([[0, 10, 10, 50, 50], [0, 1270, 10, 1290, 50], [3, 0, 0, 5, 5]], dtype=torch.int32, device=DEV)
    out2 = torch.full((3, 160, 160, 3), 7, dtype=torch.uint8, device=DEV)
    assert call(fr.data_ptr(), 1, rois2.data_ptr(), out2.data_ptr(), 3, 160, 160, 720, 1280, 0, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out2[0], out[0]) and bool((out2[1:] == 7).all())


# --------------------------------------------------------------------------------------------------------------------------------
# boxes -> embeddings -> names
# --------------------------------------------------------------------------------------------------------------------------------
BOXES = np.array([
    [100.3, 50.9, 300.2, 400.7],
    [-20.5, -3.2, 90.9, 80.1],             # clipped at the top-left corner
    [640.0, 200.0, 890.0, 460.0],
    [1200.0, 600.0, 1400.0, 900.0],        # clipped at the bottom-right corner
    [700.0, 100.0, 760.0, 161.0],          # below the detection threshold
    [500.0, 300.0, 500.4, 380.0],          # empty after truncation
    [641.0, 201.0, 891.0, 461.0],          # overlaps box 2, one pixel on
    [900.5, 20.5, 1060.5, 180.5],          # 160 x 160: the copy path
    [30.0, 500.0, 127.0, 640.0],
    [1000.0, 300.0, 1388.0, 700.0],
], dtype=np.float64)
PROBS = np.array([0.99, 0.95, 0.999, 0.93, 0.5, 0.99, 0.97, 0.92, 0.9, 0.98])
KEPT = [0, 1, 2, 3, 6, 7, 8, 9]


def _model(mt, sd, dtype):
    m = frmap_amd.get_model(mt, 36)
    m.load_state_dict(sd)
    return m.to(DEV).eval().set_compute_dtype(dtype)


def _crops(frame):
    rois, kept = frames.clip_boxes(BOXES, PROBS, frame.shape)
    assert kept.tolist() == KEPT
    return [frame[y1:y2, x1:x2] for x1, y1, x2, y2 in rois.tolist()]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("mt", ["cnn", "arcface"])
def test_embed_boxes_equals_the_per_box_get_embedding_bit_for_bit(mt, dtype, calibrated_sd):
    """Under batch-invariant planning a face's bits do not depend on its batch, so the one-launch crop + one `model(x)` of
    `embed_boxes` must reproduce the reference loop's `get_embedding(frame[y1:y2, x1:x2], model)` exactly, from a host frame and
    from a device-resident one."""
    m = _model(mt, calibrated_sd(mt), dtype)
    ops.set_batch_invariant(True)
    try:
        singles = [matching.get_embedding(c, m) for c in _crops(F720)]
        assert all(e is not None for e in singles)
        want = torch.cat([e.reshape(1, -1) for e in singles])
        for frame in (F720, torch.from_numpy(F720).to(DEV)):
            emb, kept = matching.embed_boxes(m, frame, BOXES, PROBS)
            assert kept.tolist() == KEPT and emb.shape == want.shape
            assert torch.equal(emb, want)
        emb0, kept0 = matching.embed_boxes(m, F720, BOXES[4:6], PROBS[4:6])          # nothing survives the clipping
        assert emb0.shape[0] == 0 and kept0.shape == (0,)
    finally:
        ops.set_batch_invariant(None)


def _loop_answers(embs, refs, thresh):
    return [matching.compare_faces(e, refs, thresh) for e in embs]


def _gallery_and_threshold(singles, seed, dtype):
    """refs = unrelated unit rows around the loop's own embeddings of every second crop; thresh = half the smallest distance an
    un-enrolled crop has to any entry.  Enrolled crops then have a name to find (distance ~ 0), the others are "Unknown", and no
    answer hangs on an error the size of the gate: asserted, so that a disagreement below is the code's and not a coin flip."""
    other = synth.unit_rows(seed, 13, 512)
    enrolled = list(range(1, len(singles), 2))
    refs = [{"name": f"other{i}", "embedding": other[i:i + 1]} for i in range(6)]
    refs += [{"name": f"face{KEPT[i]}", "embedding": singles[i].detach().cpu()} for i in enrolled]
    refs += [{"name": f"other{i}", "embedding": other[i:i + 1]} for i in range(6, 13)]
    d = torch.cdist(torch.cat(singles).cpu().double(), torch.cat([r["embedding"] for r in refs]).double())
    best = d.min(dim=1).values
    far = float(best[[i for i in range(len(singles)) if i not in enrolled]].min())
    assert float(best[enrolled].max()) < 1e-4 and far > 16 * DIST_BOUND[dtype], (best.tolist(), far)
    thresh = far / 2
    want = _loop_answers(singles, refs, thresh)
    assert [w[0] for w in want] == [f"face{KEPT[i]}" if i in enrolled else "Unknown" for i in range(len(singles))]
    return refs, thresh, want


def _check_identify(got, kept, want, dtype, label):
    assert kept.tolist() == KEPT and len(got) == len(want)
    err = max(abs(g[1] - w[1]) for g, w in zip(got, want))
    print(f"identify_boxes {label} {dtype}: max |dist - per-box loop| = {err:.3e} (gate {DIST_BOUND[dtype]:.1e}); names "
          f"{[g[0] for g in got]}")
    assert [(g[0], g[2]) for g in got] == [(w[0], w[2]) for w in want]
    assert err < DIST_BOUND[dtype], err


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_identify_boxes_equals_the_per_box_loop_arcface(dtype, calibrated_sd):
    """Default planning (bits may depend on the batch size): same `(name, ref_idx)` as the per-box `get_embedding` + `compare_faces`
    loop for every kept box, distances within the project's gate for the dtype.  'arcface' returns unit-norm embeddings from
    `model(x)`, the scale `DIST_BOUND` was stated for."""
    m = _model("arcface", calibrated_sd("arcface"), dtype)
    singles = [matching.get_embedding(c, m) for c in _crops(F720)]
    refs, thresh, want = _gallery_and_threshold(singles, 4242, dtype)
    for frame in (F720, torch.from_numpy(F720).to(DEV)):
        got, kept = matching.identify_boxes(m, frame, BOXES, refs, thresh, probs=PROBS)
        _check_identify(got, kept, want, dtype, "arcface forward")
    g = frmap_amd.Gallery([r["name"] for r in refs], torch.cat([r["embedding"] for r in refs]), DEV)
    got, kept = matching.identify_boxes(m, F720, BOXES, g, thresh, probs=PROBS)        # a Gallery instead of the refs list
    _check_identify(got, kept, want, dtype, "arcface forward, Gallery")
    # empty refs, no boxes
    for empty in ([], None):
        got, kept = matching.identify_boxes(m, F720, BOXES, empty, 1.0, probs=PROBS)
        assert kept.tolist() == KEPT and got == [("Unknown", float("inf"), None)] * len(KEPT)
    got, kept = matching.identify_boxes(m, F720, BOXES[4:6], refs, 1.0, probs=PROBS[4:6])
    assert got == [] and kept.shape == (0,)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_identify_boxes_embedding_mode_feeds_the_handle_uint8_crops(dtype, calibrated_sd):
    """`what="embedding", normalize=True` on 'cnn' (a model-handle model whose input normalisation is set to get_embedding's
    0.5 / 0.5): the uint8 crops go straight into `frmap_model_embed_and_match`.  Same names and indices as matching the
    L2-normalised `model.get_embedding` of each crop on its own; distances within the same gate (config 2's path and scale)."""
    m = _model("cnn", calibrated_sd("cnn"), dtype).set_input_normalization((.5, .5, .5), (.5, .5, .5))
    assert m.model_handle() is not None
    singles = []
    for c in _crops(F720):
        u8 = resize.resize_bilinear_u8([np.ascontiguousarray(c[:, :, ::-1])], (160, 160), DEV)
        x = ops.normalize_u8(u8, (.5, .5, .5), (.5, .5, .5))[0]
        with torch.no_grad():
            singles.append(ops.l2_normalize(m.get_embedding(x).reshape(1, -1), 1e-12))
    refs, thresh, want = _gallery_and_threshold(singles, 4243, dtype)
    got, kept = matching.identify_boxes(m, F720, BOXES, refs, thresh, probs=PROBS, what="embedding", normalize=True)
    _check_identify(got, kept, want, dtype, "cnn embedding (uint8 handle path)")
    # other normalisation than the handle's: the fp32 input path, same answer
    got, kept = matching.identify_boxes(m.set_input_normalization((.4, .5, .6), (.5, .5, .5)), F720, BOXES, refs, thresh, probs=PROBS,
                                        what="embedding", normalize=True)
    _check_identify(got, kept, want, dtype, "cnn embedding (fp32 input path)")
    with pytest.raises(ValueError):
        matching.identify_boxes(m, F720, BOXES, refs, what="logits")
