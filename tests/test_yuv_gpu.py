"""GPU: face crops straight from 4:2:0 YUV frames - `resize.crop_resize_u8` / `align_crop_resize_u8` on `resize.YuvFrame`s (NV12,
NV21, I420; one launch, a filter tap converting the pixel it reads, no RGB frame in memory) against the SAME calls on the frame
converted by `frames.yuv_to_rgb`, and `matching.identify_streams` on NV12 frames against the same call on the converted BGR
frames.  Every comparison is on bits; there is no tolerance in this file."""
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import big_cases as bc  # noqa: E402
import frmap_amd  # noqa: E402
import yuv_cases as yc  # noqa: E402
from frmap_amd import _lib, frames, matching, resize, synth  # noqa: E402

DEV = "cuda"
_WANT = {}


def _rois5(per_frame):
    return np.array([[f, *roi] for f, rois in enumerate(per_frame) for roi in rois], dtype=np.int64)


def _want_crops(key, rgbs, r5, size):
    """The existing crop of the converted frames, computed once per (frames, size) and shared by the formats."""
    key = (key, size)
    if key not in _WANT:
        _WANT[key] = resize.crop_resize_u8([np.array(a) for a in rgbs], r5, size, device=DEV).cpu()
    return _WANT[key]


@pytest.mark.parametrize("csc", range(4))
@pytest.mark.parametrize("fmt", yc.FORMATS)
def test_plain_crops_equal_the_crops_of_the_converted_frames(fmt, csc):
    """Two frames of different sizes (37 x 53: odd both ways; 64 x 48) and DIFFERENT csc in one launch, padded pitches, on the
    device; every ROI of `yuv_cases.rois` (full frame, 1 x 1, odd x1 / y1, last row / column) at every size of `OUT_SIZES`
    (upscale, heaviest reduction, ROI-sized = copy on both axes, one axis equal)."""
    cscs = (csc, (csc + 1) % 4)
    fr = [yc.frame(fmt, H, W, c, device=DEV) for (H, W), c in zip(yc.SIZES, cscs)]
    assert all(f.device.type == "cuda" and f.y_pitch > f.shape[1] for f in fr)
    rgbs = [yc.rgb(H, W, c) for (H, W), c in zip(yc.SIZES, cscs)]
    r5 = _rois5([yc.rois(H, W) for H, W in yc.SIZES])
    for size in yc.OUT_SIZES:
        got = resize.crop_resize_u8(fr, r5, size, bgr=(csc % 2 == 1))            # bgr is ignored for YUV frames
        assert got.shape == (len(r5), size[0], size[1], 3) and got.dtype == torch.uint8 and got.is_cuda
        want = _want_crops(("plain", cscs), rgbs, r5, size)
        bad = [i for i in range(len(r5)) if not torch.equal(got[i].cpu(), want[i])]
        assert not bad, (fmt, cscs, size, [r5[i].tolist() for i in bad])
    # the sizes are what their comments say: a ROI-sized output is the converted slice itself
    i = [r.tolist() for r in r5].index([0, 3, 5, 23, 22])
    assert np.array_equal(resize.crop_resize_u8(fr, r5, (17, 20))[i].cpu().numpy(), rgbs[0][5:22, 3:23])


def test_plain_crops_equal_pillow_on_the_converted_slice():
    H, W = yc.SIZES[0]
    f = yc.frame("nv12", H, W, 0, device=DEV)
    rgb = yc.rgb(H, W, 0)
    rois = yc.rois(H, W)
    got = resize.crop_resize_u8(f, np.array(rois), (160, 160)).cpu().numpy()
    for i, (x1, y1, x2, y2) in enumerate(rois):
        want = np.asarray(Image.fromarray(np.ascontiguousarray(rgb[y1:y2, x1:x2])).resize((160, 160), Image.BILINEAR))
        assert np.array_equal(got[i], want), (i, rois[i])


def test_tall_roi_takes_pillows_other_pass_order():
    """A 404 x 4 ROI of a 404 x 8 frame to 8 x 8, between ROIs that take the kernel: the wrapper cuts the converted crop at its own
    size with the YUV kernel and resizes it with `resize_bilinear_u8`, as it does for aligned crops."""
    H, W, tall = yc.TALL
    assert tall[3] - tall[1] > 100 * (tall[2] - tall[0])
    rois = np.array([(0, 0, 8, 100), tall, (1, 3, 8, 404)])
    for fmt, csc in (("nv12", 0), ("i420", 3)):
        f = yc.frame(fmt, H, W, csc, device=DEV)
        rgb = np.array(yc.rgb(H, W, csc))
        got = resize.crop_resize_u8(f, rois, (8, 8))
        assert torch.equal(got.cpu(), resize.crop_resize_u8(rgb, rois, (8, 8), device=DEV).cpu()), fmt
        x1, y1, x2, y2 = tall
        want = np.asarray(Image.fromarray(np.ascontiguousarray(rgb[y1:y2, x1:x2])).resize((8, 8), Image.BILINEAR))
        assert np.array_equal(got[1].cpu().numpy(), want)
        m = np.stack([frames.rotation_matrix(4.0, (4.0, 200.0))] * 3)
        assert torch.equal(resize.align_crop_resize_u8(f, rois, m, (8, 8)).cpu(), resize.align_crop_resize_u8(rgb, rois, m, (8, 8), device=DEV).cpu())


@pytest.mark.parametrize("cscs", [(0, 3), (2, 1)])
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_aligned_crops_equal_the_aligned_crops_of_the_converted_frames(fmt, cscs):
    """Rotations that leave the source inside the frame, throw part or all of it outside (RGB 0) and put samples on its clamped
    edge; two frames of different csc in one launch."""
    fr = [yc.frame(fmt, H, W, c, device=DEV) for (H, W), c in zip(yc.SIZES, cscs)]
    rgbs = [np.array(yc.rgb(H, W, c)) for (H, W), c in zip(yc.SIZES, cscs)]
    cases = [(f, *case) for f, (H, W) in enumerate(yc.SIZES) for case in yc.align_cases(H, W)]
    r5 = np.array([[f, *roi] for f, roi, _, _ in cases], dtype=np.int64)
    mats = np.stack([frames.rotation_matrix(angle, center) for _, _, angle, center in cases])
    for size in yc.ALIGN_SIZES:
        got = resize.align_crop_resize_u8(fr, r5, mats, size, bgr=True)              # bgr is ignored for YUV frames
        key = (("align", cscs), size)
        if key not in _WANT:
            _WANT[key] = resize.align_crop_resize_u8(rgbs, r5, mats, size, device=DEV).cpu()
        want = _WANT[key]
        bad = [i for i in range(len(cases)) if not torch.equal(got[i].cpu(), want[i])]
        assert not bad, (fmt, cscs, size, [cases[i] for i in bad])
        # the cases are what their comments say: black fill inside some crops, one crop all black, angle 0 the plain crop
        zero = [i for i, c in enumerate(cases) if c[3] == (-200.0, -200.0)]
        assert zero and all(int(want[i].max()) == 0 for i in zero)
        plain = [i for i, c in enumerate(cases) if c[2] == 0.0]
        assert torch.equal(want[plain], resize.crop_resize_u8(rgbs, r5[plain], size, device=DEV).cpu())
    full = np.asarray(Image.fromarray(rgbs[0]).rotate(29.999, resample=Image.BILINEAR, center=(0, 0)))
    assert (full.max(2) == 0).any() and (full.max(2) > 0).any()
    i = [(c[0], c[1], c[2]) for c in cases].index((0, (0, 0, yc.SIZES[0][1], yc.SIZES[0][0]), 29.999))
    assert np.array_equal(resize.align_crop_resize_u8(fr, r5[i:i + 1], mats[i:i + 1], yc.SIZES[0]).cpu().numpy()[0], full)   # Pillow itself


def test_empty_calls_a_decoder_surface_and_host_planes():
    H, W = yc.SIZES[1]
    dev_frame = yc.frame("nv12", H, W, 2, device=DEV)
    for empty in (np.zeros((0, 4), np.int64), np.zeros((0, 5), np.int32), []):
        e = resize.crop_resize_u8(dev_frame, empty, (24, 16))
        assert e.shape == (0, 24, 16, 3) and e.dtype == torch.uint8 and e.is_cuda
        e = resize.align_crop_resize_u8(dev_frame, empty, np.zeros((0, 6)), (24, 16))
        assert e.shape == (0, 24, 16, 3) and e.dtype == torch.uint8 and e.is_cuda
    rois = np.array(yc.rois(H, W))
    mats = np.stack([frames.rotation_matrix(-9.5, (20.0, 30.0))] * len(rois))
    want = resize.crop_resize_u8(dev_frame, rois, (40, 20)).cpu()
    want_a = resize.align_crop_resize_u8(dev_frame, rois, mats, (40, 20)).cpu()
    assert torch.equal(want, _want_crops(("surface", 2), [yc.rgb(H, W, 2)], np.concatenate([np.zeros((len(rois), 1), np.int64), rois], 1), (40, 20)))
    # the decoder's single [3 H / 2, W] buffer == the two-plane form; padded pitch; host (one upload) and device
    for pad in (False, True):
        s = yc.surface(H, W, pad=pad)
        host = resize.nv12_frame(s, standard="bt709")
        up = host.to(DEV)
        assert up.device.type == "cuda" and len({t.untyped_storage().data_ptr() for t in up.planes()}) == 1
        assert up.u.data_ptr() == up.y.data_ptr() + H * up.y_pitch and up.v.data_ptr() == up.u.data_ptr() + 1
        dev_surface = torch.from_numpy(np.ascontiguousarray(s)).to(DEV)
        for f in (host, up, resize.nv12_frame(dev_surface, standard="bt709")):
            assert torch.equal(resize.crop_resize_u8(f, rois, (40, 20), device=DEV).cpu(), want), pad
            assert torch.equal(resize.align_crop_resize_u8(f, rois, mats, (40, 20), device=DEV).cpu(), want_a), pad
    # host planes of every layout == device planes
    for fmt in yc.FORMATS:
        host = yc.frame(fmt, H, W, 2)
        assert host.device.type == "cpu"
        assert torch.equal(resize.crop_resize_u8([host], rois, (40, 20), device=DEV).cpu(), want), fmt
        assert torch.equal(resize.align_crop_resize_u8(host, rois, mats, (40, 20), device=DEV).cpu(), want_a), fmt
    packed = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="cannot be mixed"):
        resize.crop_resize_u8([dev_frame, packed], rois, (40, 20))
    with pytest.raises(ValueError, match="LDS"):
        resize.crop_resize_u8(yc.frame("nv12", *yc.TALL[:2], 0, device=DEV), np.array([[0, 0, 8, 404]]), (1, 300))


def test_c_entry_points_reject_before_any_launch():
    lib = _lib.load()
    H, W = yc.SIZES[1]
    f = yc.frame("nv12", H, W, 0, device=DEV)
    desc = np.zeros(1, resize.YUV_FRAME_DTYPE)
    desc[0] = f.record()
    fr = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    rois = torch.tensor([[0, 10, 10, 40, 50]], dtype=torch.int32, device=DEV)
    eye = frames.rotation_matrix(5.0, (30, 30))
    mats = torch.from_numpy(eye[None].copy()).to(DEV)
    out = torch.zeros((1, 160, 160, 3), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    crop, align = lib.frmap_crop_resize_yuv, lib.frmap_align_crop_resize_yuv
    good = (fr.data_ptr(), 1, rois.data_ptr(), out.data_ptr(), 1, 160, 160, H, W, st)
    good_a = good[:3] + (mats.data_ptr(),) + good[3:]
    for call, base, ptrs in ((crop, good, (0, 2, 3)), (align, good_a, (0, 2, 3, 4))):
        n0 = len(base) - 10                                                  # position of n_frames' neighbours shifts by the mats argument
        for pos in ptrs:
            args = list(base)
            args[pos] = None
            assert call(*args) == -1 and b"null pointer" in lib.frmap_last_error()
        for pos, val in ((4 + n0, -1), (1, 0), (5 + n0, 0), (6 + n0, 65537), (7 + n0, 0), (8 + n0, (1 << 24) + 1)):
            args = list(base)
            args[pos] = val
            assert call(*args) == -1, (pos, val)
            assert pos == 4 + n0 or b"bad shape" in lib.frmap_last_error()
        args = list(base)
        args[7 + n0] = 1 << 20
        assert call(*args) == -1 and b"bytes of LDS for one output row" in lib.frmap_last_error()
    args = list(good_a)
    args[3] = mats.data_ptr() + 4
    assert align(*args) == -1 and b"mats must be 8-byte aligned" in lib.frmap_last_error()
    assert crop(None, 0, None, None, 0, 160, 160, H, W, st) == 0 and align(None, 0, None, None, None, 0, 160, 160, H, W, st) == 0
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                                               # none of the rejected calls wrote anything
    rgb = np.array(yc.rgb(H, W, 0))
    assert crop(*good) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), resize.crop_resize_u8(rgb, np.array([[10, 10, 40, 50]]), (160, 160), device=DEV).cpu())
    assert align(*good_a) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), resize.align_crop_resize_u8(rgb, np.array([[10, 10, 40, 50]]), eye[None], (160, 160), device=DEV).cpu())


def test_rows_past_the_2_gib_offset():
    """A 3-row frame whose luma pitch is 2^30 + 64 bytes: row 2 begins past the 2 GiB offset (a 32-bit row offset would wrap; a
    signed one turns negative).  The chroma pitch is 2^31 + 64: chroma row 1 as well.  Equal to the same rows packed tightly."""
    H, W = 3, 96
    y_pitch, c_pitch = 2 ** 30 + 64, 2 ** 31 + 64
    y, u, v = yc.planes(H, W, 5)
    bc.need_memory((H - 1) * y_pitch + c_pitch + 2 * W + 512 * 2 ** 20, "a YUV frame with rows past the 2 GiB offset")
    big_y = torch.empty((H - 1) * y_pitch + W, dtype=torch.uint8, device=DEV)
    big_c = torch.empty(c_pitch + W, dtype=torch.uint8, device=DEV)
    try:
        yv = torch.as_strided(big_y, (H, W), (y_pitch, 1))
        cv = torch.as_strided(big_c, (2, W // 2, 2), (c_pitch, 2, 1))
        yv.copy_(torch.from_numpy(np.array(y)).to(DEV))
        cv[:, :, 0].copy_(torch.from_numpy(np.array(u)).to(DEV))
        cv[:, :, 1].copy_(torch.from_numpy(np.array(v)).to(DEV))
        f = resize.nv12_frame(yv, cv, "bt709", True)
        assert f.y_pitch == y_pitch and f.c_pitch == c_pitch and (H - 1) * f.y_pitch > 2 ** 31 and f.c_pitch > 2 ** 31
        rois = np.array([(0, 0, W, H), (1, 2, 50, 3), (0, 1, W, 3), (95, 2, 96, 3)])
        mats = np.stack([frames.rotation_matrix(2.0, (48.0, 1.5))] * len(rois))
        tight = resize.nv12_frame(np.array(y), np.stack([u, v], -1), "bt709", True)
        for size in ((3, 96), (8, 40)):
            assert torch.equal(resize.crop_resize_u8(f, rois, size), resize.crop_resize_u8(tight, rois, size, device=DEV)), size
            assert torch.equal(resize.align_crop_resize_u8(f, rois, mats, size), resize.align_crop_resize_u8(tight, rois, mats, size, device=DEV)), size
        assert np.array_equal(resize.crop_resize_u8(f, rois[:1], (3, 96)).cpu().numpy()[0], frames.yuv_to_rgb(y, u, v, "bt709", True))
    finally:
        del big_y, big_c
        bc.release()


# --------------------------------------------------------------------------------------------------------------------------------
# frames -> names
# --------------------------------------------------------------------------------------------------------------------------------
_rng = np.random.default_rng(20251020)


def _picture(H, W):
    """Planes of a picture with structure (16-pixel blocks under noise, as the frames of test_frames_gpu): crops of different
    places embed differently."""
    def blocks(h, w, step):
        base = np.kron(_rng.integers(0, 256, ((h + step - 1) // step, (w + step - 1) // step)), np.ones((step, step)))[:h, :w]
        return (0.75 * base + 0.25 * _rng.integers(0, 256, (h, w))).astype(np.uint8)
    return blocks(H, W, 16), blocks((H + 1) // 2, (W + 1) // 2, 8), blocks((H + 1) // 2, (W + 1) // 2, 8)


PICTURES = [_picture(360, 480), _picture(241, 321)]                                   # the second: odd both ways
BOXES = [np.array([[30.3, 40.9, 200.2, 260.7], [-20.5, -3.2, 110.9, 120.1], [300.0, 100.0, 460.0, 330.0]], np.float32),
         np.array([[10.0, 10.0, 120.0, 150.0], [150.5, 60.5, 330.0, 250.0], [100.0, 101.0, 221.0, 231.0]], np.float32)]
PROBS = [np.array([0.99, 0.95, 0.97], np.float32), np.array([0.93, 0.98, 0.96], np.float32)]


def _landmarks(boxes, tilt):
    x1, y1, x2, y2 = boxes.T.astype(np.float64)
    w, h = x2 - x1, y2 - y1
    return np.stack([np.stack([x1 + .3 * w, y1 + .4 * h + tilt * h], 1), np.stack([x1 + .7 * w, y1 + .4 * h - tilt * h], 1),
                     np.stack([x1 + .5 * w, y1 + .6 * h], 1)], 1)


def _same(a, b):
    """Two `identify_streams` results hold the same values, floats compared by their bits."""
    assert len(a) == len(b)
    for sa, sb in zip(a, b):
        assert len(sa) == len(sb)
        for xa, xb in zip(sa, sb):
            if isinstance(xa, list):
                assert [(r[0], np.float64(r[1]).tobytes(), r[2]) for r in xa] == [(r[0], np.float64(r[1]).tobytes(), r[2]) for r in xb]
            elif xa is None:
                assert xb is None
            else:
                assert xa.dtype == xb.dtype and xa.tobytes() == xb.tobytes()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_identify_streams_on_nv12_frames_equals_identify_streams_on_the_converted_frames(dtype, calibrated_sd):
    """2 streams x 3 boxes.  The crops are bit-identical, so everything after them is: results (names, distances, indices), kept,
    face ids - plain, with `landmarks=` and `margin=`, and with `templates=`; from host frames and from device frames."""
    m = frmap_amd.get_model("arcface", 36)
    m.load_state_dict(calibrated_sd("arcface"))
    m = m.to(DEV).eval().set_compute_dtype(dtype)
    yuv_host = [resize.nv12_frame(y, np.stack([u, v], -1), "bt709") for y, u, v in PICTURES]
    yuv_dev = [f.to(DEV) for f in yuv_host]
    bgr = [np.ascontiguousarray(frames.yuv_to_rgb(y, u, v, "bt709")[:, :, ::-1]) for y, u, v in PICTURES]
    assert [f.shape for f in yuv_host] == [b.shape for b in bgr]
    emb = matching.embed_streams(m, bgr, BOXES, PROBS)[0]
    assert emb.shape[0] == 6
    other = synth.unit_rows(6161, 9, 512)
    refs = [{"name": f"other{i}", "embedding": other[i:i + 1]} for i in range(5)]
    refs += [{"name": f"face{i}", "embedding": emb[i:i + 1].detach().float().cpu()} for i in (0, 2, 5)]
    refs += [{"name": f"other{i}", "embedding": other[i:i + 1]} for i in range(5, 9)]
    lms = [_landmarks(b, 0.05 * (-1) ** s) for s, b in enumerate(BOXES)]
    assert torch.equal(matching.embed_streams(m, yuv_dev, BOXES, PROBS)[0], emb)
    e1, k1 = matching.embed_boxes(m, yuv_host[1], BOXES[1], PROBS[1], landmarks=lms[1], margin=0.2)       # one frame, not a sequence
    e2, k2 = matching.embed_boxes(m, bgr[1], BOXES[1], PROBS[1], landmarks=lms[1], margin=0.2)
    assert torch.equal(e1, e2) and k1.tolist() == k2.tolist()
    g1, g2 = (matching.identify_boxes(m, f, BOXES[0], refs, 0.5, probs=PROBS[0]) for f in (yuv_dev[0], bgr[0]))
    _same([g1], [g2])
    for kw in ({}, {"landmarks": lms, "margin": 0.3}, {"margin": 0.3}):
        want_tr = matching.StreamTracker(2, 4, DEV)
        want = [matching.identify_streams(m, bgr, BOXES, refs, want_tr, 0.5, probs=PROBS, **kw) for _ in range(2)]
        names = {r[0][:4] for res, _, _ in want[0] for r in res}
        assert kw or "face" in names                                         # the enrolled crops find their own embeddings
        for fr in (yuv_host, yuv_dev):
            tr = matching.StreamTracker(2, 4, DEV)
            for step in range(2):
                _same(matching.identify_streams(m, fr, BOXES, refs, tr, 0.5, probs=PROBS, **kw), want[step])
        _same(matching.identify_streams(m, yuv_dev, BOXES, refs, None, 0.5, probs=PROBS, **kw),
              matching.identify_streams(m, bgr, BOXES, refs, None, 0.5, probs=PROBS, **kw))
    # with templates: the fifth and sixth entries (track results, track weights) as well
    runs = []
    for fr in (bgr, yuv_dev):
        tr = matching.StreamTracker(2, 4, DEV)
        tpl = matching.TrackTemplates(tr, 512, 0.9)
        runs.append([matching.identify_streams(m, fr, BOXES, refs, tr, 0.5, probs=PROBS, templates=tpl, landmarks=lms, margin=0.3) for _ in range(2)])
    assert len(runs[0][0][0]) == 5
    for step in range(2):
        _same(runs[1][step], runs[0][step])
