"""GPU: eye-aligned crops - `resize.align_crop_resize_u8` (rotate about a point + ROI crop + BGR -> RGB + Pillow-exact resize in one
launch, no rotated frame in memory) bit for bit against the Pillow chain `Image.rotate(angle, BILINEAR, center=c).crop(box)
.resize(size, BILINEAR)`, and `matching.embed_boxes` / `identify_boxes` with `landmarks=` / `margin=` against the per-face loop
(Pillow rotate + crop, then `get_embedding` + `compare_faces`)."""
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import align_cases as ac  # noqa: E402
import frmap_amd  # noqa: E402
from frmap_amd import _lib, frames, matching, ops, resize, synth  # noqa: E402
from test_configs_gpu import DIST_BOUND  # noqa: E402  (the project's gate on a distance's error per compute dtype)

DEV = "cuda"
_rng = np.random.default_rng(20240918)
FA = _rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)                 # noise
# 16-pixel blocks of random colour under pixel noise: every pixel differs from its neighbours, and crops of different places differ
# as images (their embeddings are distinct)
FB = (0.75 * np.kron(_rng.integers(0, 256, (23, 30, 3)), np.ones((16, 16, 1)))[:360] + 0.25 * _rng.integers(0, 256, (360, 480, 3))).astype(np.uint8)
FR = (FA, FB)
_ROT, _WANT = {}, {}


def _rotated(f, angle, center):
    """Pillow's rotation of frame f as an image, computed once per (frame, angle, centre) and shared by every test and size."""
    key = (f, angle, center)
    if key not in _ROT:
        _ROT[key] = Image.fromarray(FR[f]).rotate(angle, resample=Image.BILINEAR, center=center)
    return _ROT[key]


def _want(case, out_h, out_w):
    f, roi, angle, center = case
    key = (case, out_h, out_w)
    if key not in _WANT:
        a = np.asarray(_rotated(f, angle, center).crop(roi).resize((out_w, out_h), Image.BILINEAR))
        a.setflags(write=False)
        _WANT[key] = a
    return _WANT[key]


def _mats(cases):
    return np.stack([frames.rotation_matrix(angle, center) for _, _, angle, center in cases]) if cases else np.zeros((0, 6))


def _rois5(cases):
    return np.array([[f, *roi] for f, roi, _, _ in cases], dtype=np.int64).reshape(-1, 5)


def _cases(out_h, out_w):
    """(frame, (x1, y1, x2, y2), angle, centre) over (FA 240 x 320, FB 360 x 480): every path of the kernel and every way the
    rotated source meets the frame, at the smallest sizes that reach it."""
    c = []
    for i, angle in enumerate(ac.ANGLES):                                  # every angle class, centres inside the frame
        c.append((i % 2, (60, 40, 200, 190) if i % 2 == 0 else (150, 90, 371, 300), angle, (131.0, 117.0) if i % 3 else (160.5, 120.25)))
    w2, h2 = min(2 * out_w, 480), min(2 * out_h, 360)
    c += [
        (1, (100, 80, 300, 280), 17.0, (-40.0, 500.0)),                    # a centre outside the frame
        (0, (0, 50, 90, 200), 20.0, (160.0, 120.0)),                       # the four edges: the rotated source leaves the frame
        (0, (230, 30, 320, 180), 20.0, (160.0, 120.0)),                    # (black fill inside the crop)
        (1, (100, 0, 340, 110), -33.0, (240.0, 180.0)),
        (1, (120, 250, 330, 360), -33.0, (240.0, 180.0)),
        (0, (10, 10, 150, 130), 180.0, (-200.0, -200.0)),                  # every sample outside the frame: all zero
        (0, (100, 50, 101, 51), 12.0, (100.0, 50.0)),                      # 1 x 1
        (0, (120, 200, 157, 201), -7.5, (140.0, 200.0)),                   # 1 row x k columns
        (1, (5, 7, 6, 48), 7.5, (5.0, 30.0)),                              # k rows x 1 column (not "tall": 41 <= 100)
        (0, (0, 0, 320, 240), 9.0, (160.0, 120.0)),                        # the full frames
        (1, (0, 0, 480, 360), -171.0, (200.0, 190.0)),
        (1, (0, 0, 480, 360), 45.0, (480.0, 360.0)),                       # about a corner
        (0, (200, 100, 220, 130), 15.0, (210.0, 115.0)),                   # upscale on both axes
        (1, (40, 60, 40 + out_w, 60 + 91), 11.0, (150.0, 100.0)),          # width unchanged: horizontal copy
        (1, (100, 20, 100 + 233, 20 + out_h), -11.0, (200.0, 130.0)),      # height unchanged: vertical copy
        (1, (11, 13, 11 + out_w, 13 + out_h), 23.0, (120.0, 120.0)),       # size == ROI size: the rotated crop itself
        (1, (16, 0, 16 + w2, h2), -4.0, (240.0, 170.0)),                   # exact 2x (on each axis the frame has room for)
        (1, (140, 60, 140 + 188, 60 + 201), 14.0, (234.0, 140.0)),         # two boxes of one face a pixel apart, their angles
        (1, (141, 61, 141 + 188, 61 + 200), 14.1, (235.0, 140.0)),         # 0.1 degrees apart, as in consecutive video frames
    ]
    return c


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("size", [(160, 160), (224, 224), (37, 53)])
def test_align_crop_is_bit_exact_with_the_pillow_chain(size, bgr):
    out_h, out_w = size
    cases = _cases(out_h, out_w)
    src = [np.ascontiguousarray(f[:, :, ::-1]) for f in FR] if bgr else list(FR)       # BGR frames come out RGB
    got = resize.align_crop_resize_u8(src, _rois5(cases), _mats(cases), size, bgr=bgr, device=DEV)   # two frames, one call
    assert got.shape == (len(cases), out_h, out_w, 3) and got.dtype == torch.uint8 and got.is_cuda
    got = got.cpu().numpy()
    for i, case in enumerate(cases):
        assert np.array_equal(got[i], _want(case, out_h, out_w)), (i, case)
    # the cases are what their comments say
    zero = [i for i, c in enumerate(cases) if c[3] == (-200.0, -200.0)]
    assert len(zero) == 1 and int(got[zero[0]].max()) == 0
    for i in (len(ac.ANGLES) + 1, len(ac.ANGLES) + 2, len(ac.ANGLES) + 3, len(ac.ANGLES) + 4):            # black fill, not only black
        a = np.asarray(_rotated(cases[i][0], cases[i][2], cases[i][3]).crop(cases[i][1]))
        assert (a.max(2) == 0).any() and (a.max(2) > 0).any(), i


def test_align_crop_at_angle_zero_is_crop_resize():
    for size in ((160, 160), (37, 53)):
        cases = [(f, roi, 0.0, center) for f, roi, _, center in _cases(*size)]
        got = resize.align_crop_resize_u8(list(FR), _rois5(cases), _mats(cases), size, device=DEV)
        assert torch.equal(got, resize.crop_resize_u8(list(FR), _rois5(cases), size, device=DEV))


def test_align_crop_300_rois_of_a_padded_device_frame_stacks_and_empty():
    """N = 300 random ROIs / angles / centres of one device-resident frame whose rows are padded (a view of a wider buffer), BGR,
    one launch.  Then [F, H, W, 3] stacks with [N, 5] ROIs, and N = 0."""
    H, W = FA.shape[:2]
    buf = torch.full((H, W + 24, 3), 255, dtype=torch.uint8, device=DEV)
    frame = buf[:, 8:8 + W]
    frame.copy_(torch.from_numpy(np.ascontiguousarray(FA[:, :, ::-1])).to(DEV))
    assert frame.stride(0) == 3 * (W + 24) and frame.data_ptr() != buf.data_ptr()
    rng = np.random.default_rng(7)
    n = 300
    w, h = rng.integers(1, 140, n), rng.integers(1, 140, n)
    x1, y1 = rng.integers(0, W - w + 1), rng.integers(0, H - h + 1)
    rois = np.stack([x1, y1, x1 + w, y1 + h], 1)
    rois[:4] = [[0, 0, 139, 3], [W - 5, 0, W, 139], [0, H - 139, 2, H], [W - 77, H - 90, W, H]]
    angles = np.round(rng.uniform(-180.0, 180.0, n), 3)
    angles[:60] = np.round(rng.uniform(-30.0, 30.0, 60), 3)              # the range of a tilted head
    centers = np.round(np.stack([rng.uniform(-40.0, W + 40.0, n), rng.uniform(-40.0, H + 40.0, n)], 1) * 2) / 2
    cases = [(0, tuple(rois[i].tolist()), float(angles[i]), (float(centers[i, 0]), float(centers[i, 1]))) for i in range(n)]
    got = resize.align_crop_resize_u8(frame, rois, _mats(cases), (160, 160), bgr=True).cpu().numpy()
    assert got.shape == (n, 160, 160, 3)
    for i, case in enumerate(cases):
        assert np.array_equal(got[i], _want(case, 160, 160)), (i, case)
    # a stack of frames (host array, device tensor), ROIs with a frame index
    stack = np.stack([FA, FA[::-1].copy(), FA[:, ::-1].copy()])
    r5 = np.array([[2, 10, 20, 110, 150], [0, 10, 20, 110, 150], [1, 200, 100, 320, 240]])
    rot = [(13.0, (60.0, 80.0)), (-13.0, (60.0, 80.0)), (101.5, (250.0, 170.0))]
    m = np.stack([frames.rotation_matrix(a, c) for a, c in rot])
    want = np.stack([np.asarray(Image.fromarray(stack[f]).rotate(a, resample=Image.BILINEAR, center=c).crop(tuple(roi))
                                .resize((112, 112), Image.BILINEAR)) for (f, *roi), (a, c) in zip(r5.tolist(), rot)])
    assert np.array_equal(resize.align_crop_resize_u8(stack, r5, m, (112, 112), device=DEV).cpu().numpy(), want)
    assert np.array_equal(resize.align_crop_resize_u8(torch.from_numpy(stack).to(DEV), r5, torch.from_numpy(m), (112, 112)).cpu().numpy(), want)
    # N = 0
    for empty in (np.zeros((0, 4), np.int64), np.zeros((0, 5), np.int32), []):
        e = resize.align_crop_resize_u8(frame, empty, np.zeros((0, 6)), (224, 160))
        assert e.shape == (0, 224, 160, 3) and e.dtype == torch.uint8 and e.is_cuda


def test_align_crop_tall_roi_takes_pillows_other_pass_order():
    """A ROI more than 100x taller than wide whose height shrinks: Pillow resizes the rotated crop in height first; the wrapper
    makes the rotated crop with the kernel at its own size and routes it through `resize_bilinear_u8`, between ROIs that take the
    kernel."""
    cases = [(0, (50, 10, 150, 210), 8.0, (100.0, 110.0)), (0, (200, 5, 202, 235), -19.0, (201.0, 120.0)),
             (0, (300, 0, 301, 240), 5.0, (300.0, 120.0)), (0, (60, 20, 160, 220), -8.0, (110.0, 120.0))]
    assert all((c[1][3] - c[1][1] > 100 * (c[1][2] - c[1][0])) == (i in (1, 2)) for i, c in enumerate(cases))
    for bgr in (False, True):
        src = np.ascontiguousarray(FA[:, :, ::-1]) if bgr else FA
        got = resize.align_crop_resize_u8(src, _rois5(cases), _mats(cases), (100, 100), bgr=bgr, device=DEV).cpu().numpy()
        for i, case in enumerate(cases):
            assert np.array_equal(got[i], _want(case, 100, 100)), (bgr, i)


def test_align_crop_rejects_bad_arguments_on_the_host():
    ok, eye = [10, 10, 50, 50], frames.rotation_matrix(5.0, (30, 30))
    for bad in ([10, 10, 10, 50], [60, 10, 50, 50], [-1, 10, 50, 50], [10, -1, 50, 50], [10, 10, 321, 50], [10, 10, 50, 241]):
        with pytest.raises(ValueError, match="empty or leaves"):
            resize.align_crop_resize_u8(FA, np.array([ok, bad]), np.stack([eye, eye]), (160, 160), device=DEV)
    with pytest.raises(ValueError, match="frame index"):
        resize.align_crop_resize_u8(FA, np.array([[1] + ok]), eye[None], (160, 160), device=DEV)
    for wrong in (eye, np.stack([eye, eye]), eye[None, :5], np.zeros((0, 6))):          # [6], [2, 6], [1, 5], [0, 6] for one ROI
        with pytest.raises(ValueError, match="matrices"):
            resize.align_crop_resize_u8(FA, np.array([ok]), wrong, (160, 160), device=DEV)
    for bad in (np.nan, np.inf, -np.inf):
        m = np.stack([eye, eye])
        m[1, 2] = bad
        with pytest.raises(ValueError, match="non-finite"):
            resize.align_crop_resize_u8(FA, np.array([ok, ok]), m, (160, 160), device=DEV)
    with pytest.raises(ValueError, match="LDS"):
        resize.align_crop_resize_u8(FB, np.array([[0, 0, 480, 360]]), eye[None], (1, 200), device=DEV)   # 360x vertically at 200 columns
    with pytest.raises(ValueError):
        resize.align_crop_resize_u8(FA.astype(np.float32), np.array([ok]), eye[None], (160, 160), device=DEV)


def test_align_crop_c_entry_point_rejects_before_any_launch_and_skips_bad_records():
    lib = _lib.load()
    frame = torch.from_numpy(FA).to(DEV)
    desc = np.zeros(1, resize.FRAME_DTYPE)
    desc[0] = (frame.data_ptr(), 240, 320, 3 * 320)
    fr = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    rois = torch.tensor([[0, 10, 10, 50, 50]], dtype=torch.int32, device=DEV)
    eye = frames.rotation_matrix(5.0, (30, 30))
    mats = torch.from_numpy(eye[None].copy()).to(DEV)
    out = torch.zeros((1, 160, 160, 3), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    call = lib.frmap_align_crop_resize_u8
    good = (fr.data_ptr(), 1, rois.data_ptr(), mats.data_ptr(), out.data_ptr(), 1, 160, 160, 240, 320, 0, st)
    for pos in (0, 2, 3, 4):                                               # null frames / rois / mats / out
        args = list(good)
        args[pos] = None
        assert call(*args) == -1 and b"null pointer" in lib.frmap_last_error()
    args = list(good)
    args[3] = mats.data_ptr() + 4                                          # doubles off their alignment
    assert call(*args) == -1 and b"aligned" in lib.frmap_last_error()
    for pos, val in ((5, -1), (1, 0), (6, 0), (8, 0)):                     # N < 0, no frames, out_h = 0, max_roi_h = 0
        args = list(good)
        args[pos] = val
        assert call(*args) == -1
    args = list(good)
    args[8] = 1 << 20
    assert call(*args) == -1 and b"LDS" in lib.frmap_last_error()
    assert call(None, 0, None, None, None, 0, 160, 160, 240, 320, 0, st) == 0   # N = 0: nothing to do, nothing launched
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                                             # none of the rejected calls wrote anything
    assert call(*good) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), _want((0, (10, 10, 50, 50), 5.0, (30, 30)), 160, 160))
    # device records the host never sees: a ROI that leaves its frame, a frame index out of range and a matrix with a non-finite
    # entry are skipped by the kernel (nothing read out of bounds, the output left as it was)
    rois2 = torch.tensor([[0, 10, 10, 50, 50], [0, 310, 10, 330, 50], [3, 0, 0, 5, 5], [0, 10, 10, 50, 50], [0, 10, 10, 50, 50]],
                         dtype=torch.int32, device=DEV)
    m2 = np.stack([eye] * 5)
    m2[3, 5], m2[4, 0] = np.nan, np.inf
    mats2 = torch.from_numpy(m2).to(DEV)
    out2 = torch.full((5, 160, 160, 3), 7, dtype=torch.uint8, device=DEV)
    assert call(fr.data_ptr(), 1, rois2.data_ptr(), mats2.data_ptr(), out2.data_ptr(), 5, 160, 160, 240, 320, 0, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out2[0], out[0]) and bool((out2[1:] == 7).all())


# --------------------------------------------------------------------------------------------------------------------------------
# boxes + landmarks -> embeddings -> names
# --------------------------------------------------------------------------------------------------------------------------------
BOXES = np.array([
    [60.3, 40.9, 200.2, 210.7],
    [-20.5, -3.2, 110.9, 120.1],             # clipped at the top-left corner
    [240.0, 100.0, 400.0, 290.0],
    [380.0, 250.0, 520.0, 400.0],            # clipped at the bottom-right corner
    [300.0, 20.0, 360.0, 81.0],              # below the detection threshold
    [241.0, 101.0, 401.0, 291.0],            # overlaps box 2, one pixel on
    [30.0, 200.0, 190.0, 350.0],
], dtype=np.float64)
PROBS = np.array([0.99, 0.95, 0.999, 0.93, 0.5, 0.97, 0.98])
TILTS = [-25.0, 12.0, 20.0, -8.5, 3.0, 25.0, -17.0]
KEPT = [0, 1, 2, 3, 5, 6]


def _landmarks():
    """Five points per box as a detector gives them (eyes first): the eye line through the upper part of the box, tilted."""
    lm = np.zeros((len(BOXES), 5, 2))
    for i, ((x1, y1, x2, y2), t) in enumerate(zip(BOXES, TILTS)):
        cx, cy, d = (x1 + x2) / 2, y1 + 0.4 * (y2 - y1), 0.2 * (x2 - x1)
        u = np.array([np.cos(np.radians(t)), np.sin(np.radians(t))])
        n = np.array([-u[1], u[0]])
        c = np.array([cx, cy])
        lm[i] = [c - d * u, c + d * u, c + 0.8 * d * n, c + 1.6 * d * n - 0.7 * d * u, c + 1.6 * d * n + 0.7 * d * u]
    return lm


LANDMARKS = _landmarks()


def _loop_crops(margin):
    """The per-face loop on the host (`src/data_prep.py:69-106, 138-145` with Pillow's rotation): BGR crops, as `get_embedding`
    takes them, of the kept boxes."""
    H, W = FB.shape[:2]
    rgb = np.ascontiguousarray(FB[:, :, ::-1])                             # FB is the BGR frame of these tests
    crops = []
    for i in KEPT:
        x1, y1, x2, y2 = BOXES[i]
        mx, my = int((x2 - x1) * margin), int((y2 - y1) * margin)
        x1, y1, x2, y2 = max(0, x1 - mx), max(0, y1 - my), min(W, x2 + mx), min(H, y2 + my)
        le, re_ = LANDMARKS[i][0], LANDMARKS[i][1]
        angle = np.degrees(np.arctan2(re_[1] - le[1], re_[0] - le[0]))
        center = ((le[0] + re_[0]) // 2, (le[1] + re_[1]) // 2)
        rot = np.asarray(Image.fromarray(rgb).rotate(angle, resample=Image.BILINEAR, center=center))
        crops.append(np.ascontiguousarray(rot[int(y1):int(y2), int(x1):int(x2), ::-1]))
    return crops


def _model(mt, sd, dtype):
    m = frmap_amd.get_model(mt, 36)
    m.load_state_dict(sd)
    return m.to(DEV).eval().set_compute_dtype(dtype)


def test_landmarks_are_tilted_as_stated():
    got = [frames.eye_rotation(lm)[0] for lm in LANDMARKS]
    assert np.allclose(got, TILTS, atol=1e-9) and min(TILTS) == -25.0 and max(TILTS) == 25.0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("mt", ["cnn", "arcface"])
def test_embed_boxes_with_landmarks_equals_the_per_face_loop_bit_for_bit(mt, dtype, calibrated_sd):
    """Under batch-invariant planning a face's bits do not depend on its batch, so `embed_boxes(landmarks=, margin=)` must
    reproduce `get_embedding` of the loop's rotated crops exactly, from a host frame and from a device-resident one."""
    m = _model(mt, calibrated_sd(mt), dtype)
    ops.set_batch_invariant(True)
    try:
        for margin in (0.0, 0.2):
            singles = [matching.get_embedding(c, m) for c in _loop_crops(margin)]
            assert all(e is not None for e in singles)
            want = torch.cat([e.reshape(1, -1) for e in singles])
            for frame in (FB, torch.from_numpy(FB).to(DEV)):
                emb, kept = matching.embed_boxes(m, frame, BOXES, PROBS, landmarks=LANDMARKS, margin=margin)
                assert kept.tolist() == KEPT and emb.shape == want.shape
                assert torch.equal(emb, want), margin
        emb0, kept0 = matching.embed_boxes(m, FB, BOXES[4:5], PROBS[4:5], landmarks=LANDMARKS[4:5], margin=0.2)   # below det_thresh
        assert emb0.shape[0] == 0 and kept0.shape == (0,)
    finally:
        ops.set_batch_invariant(None)


def _gallery_and_threshold(singles, seed, dtype):
    """refs = unrelated unit rows around the loop's own embeddings of every second crop; thresh = half the smallest distance an
    un-enrolled crop has to any entry, so that no answer hangs on an error the size of the gate (asserted)."""
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
    want = [matching.compare_faces(e, refs, thresh) for e in singles]
    assert [w[0] for w in want] == [f"face{KEPT[i]}" if i in enrolled else "Unknown" for i in range(len(singles))]
    return refs, thresh, want


def _check_identify(got, kept, want, dtype, label):
    assert kept.tolist() == KEPT and len(got) == len(want)
    err = max(abs(g[1] - w[1]) for g, w in zip(got, want))
    print(f"identify_boxes {label} {dtype}: max |dist - per-face loop| = {err:.3e} (gate {DIST_BOUND[dtype]:.1e}); names "
          f"{[g[0] for g in got]}")
    assert [(g[0], g[2]) for g in got] == [(w[0], w[2]) for w in want]
    assert err < DIST_BOUND[dtype], err


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_identify_boxes_with_landmarks_equals_the_per_face_loop_arcface(dtype, calibrated_sd):
    """Default planning: same `(name, ref_idx)` as the per-face loop (Pillow rotate + crop, `get_embedding`, `compare_faces`) for
    every kept box, distances within the project's gate for the dtype; the box below `det_thresh` is absent."""
    m = _model("arcface", calibrated_sd("arcface"), dtype)
    for margin in (0.0, 0.2):
        singles = [matching.get_embedding(c, m) for c in _loop_crops(margin)]
        refs, thresh, want = _gallery_and_threshold(singles, 4242, dtype)
        for frame in (FB, torch.from_numpy(FB).to(DEV)):
            got, kept = matching.identify_boxes(m, frame, BOXES, refs, thresh, probs=PROBS, landmarks=LANDMARKS, margin=margin)
            _check_identify(got, kept, want, dtype, f"arcface forward, margin {margin}")
            emb, kept = matching.embed_boxes(m, frame, BOXES, PROBS, landmarks=LANDMARKS, margin=margin)
            err = float((emb.float() - torch.cat(singles).float()).norm(dim=1).max())
            assert kept.tolist() == KEPT and err < DIST_BOUND[dtype], err


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_identify_boxes_with_landmarks_feeds_the_handle_uint8_crops(dtype, calibrated_sd):
    """`what="embedding", normalize=True` on 'cnn' with get_embedding's normalisation: the aligned uint8 crops go straight into
    `frmap_model_embed_and_match`.  Same names and indices as matching the L2-normalised `model.get_embedding` of each of the
    loop's crops on its own; distances within the gate."""
    m = _model("cnn", calibrated_sd("cnn"), dtype).set_input_normalization((.5, .5, .5), (.5, .5, .5))
    assert m.model_handle() is not None
    for margin in (0.0, 0.2):
        singles = []
        for c in _loop_crops(margin):
            u8 = resize.resize_bilinear_u8([np.ascontiguousarray(c[:, :, ::-1])], (160, 160), DEV)
            x = ops.normalize_u8(u8, (.5, .5, .5), (.5, .5, .5))[0]
            with torch.no_grad():
                singles.append(ops.l2_normalize(m.get_embedding(x).reshape(1, -1), 1e-12))
        refs, thresh, want = _gallery_and_threshold(singles, 4243, dtype)
        got, kept = matching.identify_boxes(m, FB, BOXES, refs, thresh, probs=PROBS, what="embedding", normalize=True,
                                            landmarks=LANDMARKS, margin=margin)
        _check_identify(got, kept, want, dtype, f"cnn embedding (uint8 handle path), margin {margin}")


def test_aligned_crops_differ_from_unaligned_ones(calibrated_sd):
    """A silently ignored `landmarks=` must fail: the aligned and the unaligned crop of a box tilted by 20 degrees differ, as
    images and as embeddings; `margin=` alone moves the crop too."""
    assert TILTS[2] == 20.0
    rois, _ = frames.clip_boxes(BOXES[2:3], None, FB.shape)
    m6 = frames.rotation_matrix(*frames.eye_rotation(LANDMARKS[2]))[None]
    aligned = resize.align_crop_resize_u8(FB, rois, m6, (160, 160), bgr=True, device=DEV)
    plain = resize.crop_resize_u8(FB, rois, (160, 160), bgr=True, device=DEV)
    assert float((aligned != plain).float().mean()) > 0.5
    m = _model("arcface", calibrated_sd("arcface"), torch.float16)
    e_plain, _ = matching.embed_boxes(m, FB, BOXES, PROBS)
    e_align, _ = matching.embed_boxes(m, FB, BOXES, PROBS, landmarks=LANDMARKS)
    e_margin, _ = matching.embed_boxes(m, FB, BOXES, PROBS, margin=0.2)
    assert not torch.equal(e_plain, e_align) and not torch.equal(e_plain, e_margin)
    # (far beyond what rounding could move an embedding: the gate on a distance's error; row 2 is the box tilted by 20 degrees)
    assert KEPT[2] == 2 and float((e_plain - e_align).float().norm(dim=1)[2]) > 16 * DIST_BOUND[torch.float16]
    with pytest.raises(ValueError, match="landmarks"):
        matching.embed_boxes(m, FB, BOXES, PROBS, landmarks=LANDMARKS[:3])


def test_embed_boxes_without_the_new_keywords_is_unchanged(calibrated_sd):
    """`embed_boxes(...)` as before == `clip_boxes` + `crop_resize_u8` + `normalize_u8` + the model called directly, bit for bit;
    `margin=` alone == the same on the widened boxes."""
    m = _model("cnn", calibrated_sd("cnn"), torch.bfloat16)
    for margin in (0.0, 0.2):
        rois, kept = frames.clip_boxes(frames.margin_boxes(BOXES, margin, FB.shape) if margin else BOXES, PROBS, FB.shape)
        x = ops.normalize_u8(resize.crop_resize_u8(FB, rois, (160, 160), bgr=True, device=DEV), (.5, .5, .5), (.5, .5, .5))[0]
        with torch.no_grad():
            want = m(x)
        emb, k = matching.embed_boxes(m, FB, BOXES, PROBS, **({"margin": margin} if margin else {}))
        assert k.tolist() == kept.tolist() == KEPT and torch.equal(emb, want)
