"""GPU: the frame kernels (`resize.crop_resize_u8`, `align_crop_resize_u8`, the batched `resize_bilinear_u8`) between guard bands
(`guard.py`), on the ROI tables of `test_frames_gpu.py` / `test_align_gpu.py` at their smallest output sizes.  Frames are placed
operands, outputs come from the patched `resize` module; valid rows follow the two-fill rule and equal Pillow as before.  Through
the C entry points, a record that breaks the contract (leaves its frame, names no frame, carries a non-finite matrix) must leave
its output rows exactly at the fill: the kernels promise that they skip it.  These entry points take no workspace."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import test_align_gpu as tag  # noqa: E402  (its case table and cached Pillow references)
from frmap_amd import _lib, resize  # noqa: E402
from test_frames_gpu import F720, F1080, _edge_rois, _pil  # noqa: E402

DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("bgr", [False, True])
def test_crop_resize(bgr):
    out_h, out_w = 96, 200
    rois = np.array(_edge_rois(out_h, out_w), dtype=np.int64)
    got, = guard.two_fills(lambda place: resize.crop_resize_u8([place(_t(F720)), place(_t(F1080))], rois, (out_h, out_w), bgr=bgr),
                           [resize], what="crop_resize_u8")
    fr = (F720, F1080)
    for i, (f, *roi) in enumerate(rois.tolist()):
        assert np.array_equal(got[i].numpy(), _pil(fr[f], roi, out_h, out_w, bgr)), (i, f, roi)


def test_crop_resize_tall_roi_and_batched_resize():
    """The tall ROIs go through the batched `resize_bilinear_u8` (its output guarded too), between ROIs that take the kernel."""
    rois = np.array([[50, 10, 150, 210], [300, 100, 302, 500], [700, 0, 701, 720], [60, 20, 160, 220]])
    got, = guard.two_fills(lambda place: resize.crop_resize_u8(place(_t(F720)), rois, (64, 48)), [resize], what="crop_resize_u8 tall")
    for i, roi in enumerate(rois.tolist()):
        assert np.array_equal(got[i].numpy(), _pil(F720, roi, 64, 48, False)), i
    slices = [np.ascontiguousarray(F720[b:d, a:c]) for a, b, c, d in ([0, 0, 1, 1], [10, 20, 75, 21], [5, 7, 6, 48], [100, 100, 148, 164], [0, 0, 320, 200])]
    got, = guard.two_fills(lambda place: resize.resize_bilinear_u8(slices, (64, 48), DEV), [resize], what="resize_bilinear_u8")
    for i, a in enumerate(slices):
        assert np.array_equal(got[i].numpy(), _pil(a, [0, 0, a.shape[1], a.shape[0]], 64, 48, False)), i


@pytest.mark.parametrize("bgr", [False, True])
def test_align_crop(bgr):
    out_h, out_w = 37, 53
    cases = tag._cases(out_h, out_w)
    src = [np.ascontiguousarray(f[:, :, ::-1]) for f in tag.FR] if bgr else list(tag.FR)
    got, = guard.two_fills(lambda place: resize.align_crop_resize_u8([place(_t(f)) for f in src], tag._rois5(cases), tag._mats(cases),
                                                                     (out_h, out_w), bgr=bgr), [resize], what="align_crop_resize_u8")
    for i, case in enumerate(cases):
        assert np.array_equal(got[i].numpy(), tag._want(case, out_h, out_w)), (i, case)


def test_align_crop_tall_roi():
    cases = [(0, (50, 10, 150, 210), 8.0, (100.0, 110.0)), (0, (200, 5, 202, 235), -19.0, (201.0, 120.0)),
             (0, (60, 20, 160, 220), -8.0, (110.0, 120.0))]
    got, = guard.two_fills(lambda place: resize.align_crop_resize_u8(place(_t(tag.FA)), tag._rois5(cases), tag._mats(cases), (100, 100)),
                           [resize], what="align_crop_resize_u8 tall")
    for i, case in enumerate(cases):
        assert np.array_equal(got[i].numpy(), tag._want(case, 100, 100)), i


@pytest.mark.parametrize("align", [False, True], ids=["crop_resize", "align_crop"])
def test_a_record_that_breaks_the_contract_leaves_its_rows_at_the_fill(align):
    """Device records the host never saw: row 0 is valid, the others leave the frame (right, bottom), are empty, name frame 3 of 1
    and (aligned) carry a NaN matrix.  Their rows stay at the fill under both fills; row 0 is Pillow's both times."""
    lib = _lib.load()
    H, W = tag.FA.shape[:2]
    oh, ow = 37, 53
    recs = [[0, 10, 10, 50, 50], [0, W - 10, 10, W + 10, 50], [0, 10, H - 5, 50, H + 1], [0, 60, 60, 60, 90], [3, 0, 0, 5, 5], [0, 20, 20, 60, 70]]
    mats = np.stack([tag.frames.rotation_matrix(7.0, (30.0, 30.0))] * len(recs))
    if align:
        mats[5, 2] = np.nan
    want0 = tag._want((0, (10, 10, 50, 50), 7.0, (30.0, 30.0)), oh, ow) if align else _pil(tag.FA, [10, 10, 50, 50], oh, ow, False)
    want5 = None if align else _pil(tag.FA, [20, 20, 60, 70], oh, ow, False)
    st = torch.cuda.current_stream().cuda_stream
    for fill in guard.FILLS:
        g = guard.Guard(fill)
        frame = g.place(_t(tag.FA))
        desc = np.zeros(1, resize.FRAME_DTYPE)
        desc[0] = (frame.data_ptr(), H, W, 3 * W)
        fr = g.place(_t(desc.view(np.uint8)))
        rois = g.place(torch.tensor(recs, dtype=torch.int32))
        out = g.empty((len(recs), oh, ow, 3), torch.uint8)
        if align:
            m = g.place(_t(mats))
            rc = lib.frmap_align_crop_resize_u8(fr.data_ptr(), 1, rois.data_ptr(), m.data_ptr(), out.data_ptr(), len(recs), oh, ow, 50, 40, 0, st)
        else:
            rc = lib.frmap_crop_resize_u8(fr.data_ptr(), 1, rois.data_ptr(), out.data_ptr(), len(recs), oh, ow, 50, 40, 0, st)
        assert rc == 0, lib.frmap_last_error()
        g.check()
        got = out.cpu().numpy()
        assert np.array_equal(got[0], want0)
        skipped = (1, 2, 3, 4, 5) if align else (1, 2, 3, 4)
        for i in skipped:
            assert (got[i] == fill).all(), (hex(fill), i)
        if not align:
            assert np.array_equal(got[5], want5)
