"""GPU: the YUV crop kernels (`resize.crop_resize_u8` / `align_crop_resize_u8` on `resize.YuvFrame`s) between guard bands
(`guard.py`), as `test_guard_frames_gpu.py` does for the packed-frame kernels.  Planes are placed operands (their padding included:
a read outside a plane's rows lands in padding or a band, a write anywhere shows), outputs come from the patched `resize` module;
valid rows follow the two-fill rule and equal the crops of the converted frames.  Through the C entry points, records, matrices
and output are placed too, and one record of each contract-breaking kind must leave exactly its rows at the fill while its
neighbours come out right."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import yuv_cases as yc  # noqa: E402
from frmap_amd import _lib, frames, resize  # noqa: E402

DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _placed_frame(place, fmt, H, W, csc):
    """The frame of `yuv_cases.frame` with every underlying buffer (padding included) placed whole, the planes cut out of it."""
    yb, ub, vb, pairs = yc.layout(fmt, *yc.planes(H, W))
    std, full = yc.CSC[csc]

    def put(view):
        base = view
        while isinstance(base.base, np.ndarray):
            base = base.base
        off = view.__array_interface__["data"][0] - base.__array_interface__["data"][0]
        t = place(_t(base.reshape(-1)))                                      # (a guard's payload starts inside its storage)
        return torch.as_strided(t, view.shape, view.strides, t.storage_offset() + off)

    if fmt == "i420":
        return resize.i420_frame(put(yb), put(ub), put(vb), std, full)
    return (resize.nv12_frame if fmt == "nv12" else resize.nv21_frame)(put(yb), put(pairs), std, full)


def _r5():
    return np.array([[f, *roi] for f, (H, W) in enumerate(yc.SIZES) for roi in yc.rois(H, W)], dtype=np.int64)


@pytest.mark.parametrize("fmt", yc.FORMATS)
def test_crop_resize_yuv(fmt):
    cscs = (1, 2)
    r5 = _r5()
    rgbs = [np.array(yc.rgb(H, W, c)) for (H, W), c in zip(yc.SIZES, cscs)]
    for size in ((8, 8), (17, 20)):
        got, = guard.two_fills(lambda place: resize.crop_resize_u8([_placed_frame(place, fmt, H, W, c) for (H, W), c in zip(yc.SIZES, cscs)],
                                                                   r5, size), [resize], what="crop_resize_u8 on YUV frames")
        assert torch.equal(got, resize.crop_resize_u8(rgbs, r5, size, device=DEV).cpu()), (fmt, size)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_align_crop_yuv(fmt):
    cscs = (0, 3)
    cases = [(f, *case) for f, (H, W) in enumerate(yc.SIZES) for case in yc.align_cases(H, W)]
    r5 = np.array([[f, *roi] for f, roi, _, _ in cases], dtype=np.int64)
    mats = np.stack([frames.rotation_matrix(angle, center) for _, _, angle, center in cases])
    rgbs = [np.array(yc.rgb(H, W, c)) for (H, W), c in zip(yc.SIZES, cscs)]
    for size in ((8, 8), (17, 20)):
        got, = guard.two_fills(lambda place: resize.align_crop_resize_u8([_placed_frame(place, fmt, H, W, c) for (H, W), c in zip(yc.SIZES, cscs)],
                                                                         r5, mats, size), [resize], what="align_crop_resize_u8 on YUV frames")
        assert torch.equal(got, resize.align_crop_resize_u8(rgbs, r5, mats, size, device=DEV).cpu()), (fmt, size)


def test_tall_roi_of_a_yuv_frame():
    H, W, tall = yc.TALL
    rois = np.array([(0, 0, 8, 100), tall, (1, 3, 8, 404)])
    got, = guard.two_fills(lambda place: resize.crop_resize_u8(_placed_frame(place, "nv21", H, W, 2), rois, (8, 8)), [resize],
                           what="crop_resize_u8 on a YUV frame, tall")
    assert torch.equal(got, resize.crop_resize_u8(np.array(yc.rgb(H, W, 2)), rois, (8, 8), device=DEV).cpu())


@pytest.mark.parametrize("align", [False, True], ids=["crop_resize_yuv", "align_crop_yuv"])
def test_a_record_that_breaks_the_contract_leaves_its_rows_at_the_fill(align):
    """Device records the host never saw.  Frames 0 and 1 are valid (NV12 and I420); frames 2 .. 8 are frame 0 with one field broken
    each: a null y, u or v plane, c_step 3, csc 4, y_pitch < W, c_pitch < c_step * ceil(W / 2).  ROI records: valid ones of frames 0
    and 1 first and last, between them one that names frame 9 of 9, ones that leave the frame (right, bottom), an empty one, one per
    broken frame, one whose taps exceed the launch's cap (a 37-row ROI in a launch sized for 20) and - aligned - one with a NaN and
    one with an infinite matrix entry.  Their rows stay at the fill under both fills; the valid rows are right both times."""
    lib = _lib.load()
    (H0, W0), (H1, W1) = yc.SIZES
    oh, ow = 8, 8
    good = [[0, 3, 5, 23, 22], [1, 2, 4, 33, 21]]
    recs = [good[0], [9, 0, 0, 5, 5], [0, W0 - 10, 10, W0 + 10, 30], [0, 10, H0 - 5, 30, H0 + 1], [0, 20, 20, 20, 30], [-1, 0, 0, 5, 5]]
    recs += [[k, 3, 5, 23, 22] for k in range(2, 9)]
    recs += [[0, 0, 0, 20, H0]]                                                   # taller than max_roi_h: more taps than the cap
    n_bad_mats = 2 if align else 0
    recs += [good[0]] * n_bad_mats + [good[1]]
    n = len(recs)
    valid = (0, n - 1)
    mats = np.stack([frames.rotation_matrix(7.0, (12.0, 12.0))] * n)
    if align:
        mats[n - 3, 2], mats[n - 2, 4] = np.nan, np.inf
    rgbs = [np.array(yc.rgb(H, W, c)) for (H, W), c in zip(yc.SIZES, (0, 3))]
    rv = np.array([recs[i] for i in valid])
    want = (resize.align_crop_resize_u8(rgbs, rv, mats[list(valid)], (oh, ow), device=DEV) if align else
            resize.crop_resize_u8(rgbs, rv, (oh, ow), device=DEV)).cpu()
    st = torch.cuda.current_stream().cuda_stream
    for fill in guard.FILLS:
        g = guard.Guard(fill)
        fr = [_placed_frame(g.place, "nv12", H0, W0, 0), _placed_frame(g.place, "i420", H1, W1, 3)]
        desc = np.zeros(9, resize.YUV_FRAME_DTYPE)
        desc[0], desc[1] = fr[0].record(), fr[1].record()
        desc[2:] = desc[0]
        desc[2]["y"], desc[3]["u"], desc[4]["v"] = 0, 0, 0
        desc[5]["c_step"], desc[6]["csc"] = 3, 4
        desc[7]["y_pitch"], desc[8]["c_pitch"] = W0 - 1, 2 * ((W0 + 1) // 2) - 1
        d = g.place(_t(desc.view(np.uint8)))
        rois = g.place(torch.tensor(recs, dtype=torch.int32))
        out = g.empty((n, oh, ow, 3), torch.uint8)
        if align:
            m = g.place(_t(mats))
            rc = lib.frmap_align_crop_resize_yuv(d.data_ptr(), 9, rois.data_ptr(), m.data_ptr(), out.data_ptr(), n, oh, ow, 20, 40, st)
        else:
            rc = lib.frmap_crop_resize_yuv(d.data_ptr(), 9, rois.data_ptr(), out.data_ptr(), n, oh, ow, 20, 40, st)
        assert rc == 0, lib.frmap_last_error()
        g.check()
        got = out.cpu()
        for k, i in enumerate(valid):
            assert torch.equal(got[i], want[k]), (hex(fill), i)
        for i in range(n):
            if i not in valid:
                assert bool((got[i] == fill).all()), (hex(fill), i, recs[i])
