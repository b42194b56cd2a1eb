"""Device-side `transforms.Resize(size)` for PIL-style 8-bit RGB images (`src/testing.py:99-100`, `src/training.py:305-310`,
`src/app.py:39`): bit-exact with Pillow's bilinear resampler.

Pillow resizes in two passes of small integer FIR filters (libImaging/Resample.c).  The filter tables depend only on the
(input size, output size) pair; they are built here on the host, in float64 with Pillow's operation order, cached per pair
and shipped with the batch; the integer arithmetic over the pixels (`frmap_resize_bilinear_u8`) runs on the GPU, so the
decoded images cross PCIe once, at their native size, and everything after the decode is on the device.
"""
from __future__ import annotations

import functools
import math
from typing import Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import frames as _frames

PRECISION_BITS = 32 - 8 - 2
ITEM_DTYPE = np.dtype([("src_off", "<u8"), ("H", "<i4"), ("W", "<i4"), ("bx_off", "<i4"), ("kx_off", "<i4"), ("ksx", "<i4"),
                       ("by_off", "<i4"), ("ky_off", "<i4"), ("ksy", "<i4")])   # FrmapResizeItem (csrc/resize.hip), 40 bytes
FRAME_DTYPE = np.dtype([("base", "<u8"), ("H", "<i4"), ("W", "<i4"), ("pitch", "<i8")])   # FrmapFrame (csrc/frame_records.h), 24 bytes
YUV_FRAME_DTYPE = np.dtype([("y", "<u8"), ("u", "<u8"), ("v", "<u8"), ("H", "<i4"), ("W", "<i4"), ("y_pitch", "<i8"), ("c_pitch", "<i8"),
                            ("c_step", "<i4"), ("csc", "<i4")])                            # FrmapYuvFrame (csrc/frame_records.h), 56 bytes


@functools.lru_cache(maxsize=512)
def bilinear_coeffs(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Resample.c `precompute_coeffs` (bilinear, support 1, box = the whole axis) + `normalize_coeffs_8bpc`:
    ``(bounds int32 [out, 2] = (first input sample, taps), coeffs int32 [out, ksize])``.  float64, same operation order
    as the C code (the weights are summed left to right, divided by the sum, scaled by 2^22, rounded half away from zero)."""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xx = np.arange(out_size, dtype=np.float64)
    center = 0.0 + (xx + 0.5) * scale
    xmin = (center - support + 0.5).astype(np.int64)          # C cast: truncation toward zero
    xmin = np.maximum(xmin, 0)
    xmax = (center + support + 0.5).astype(np.int64)
    xmax = np.minimum(xmax, in_size) - xmin
    w = np.zeros((out_size, ksize), np.float64)
    ww = np.zeros(out_size, np.float64)
    for x in range(ksize):                                    # left-to-right accumulation, as the C loop
        v = np.abs((x + xmin - center + 0.5) * ss)
        wx = np.where(v < 1.0, 1.0 - v, 0.0)
        wx = np.where(x < xmax, wx, 0.0)
        w[:, x] = wx
        ww = np.where(x < xmax, ww + wx, ww)
    nz = ww != 0.0
    w[nz] = w[nz] / ww[nz, None]
    p = w * float(1 << PRECISION_BITS)
    kk = np.where(w < 0, (-0.5 + p), (0.5 + p)).astype(np.int64).astype(np.int32)   # (int) cast truncates
    kk[np.arange(ksize)[None, :] >= xmax[:, None]] = 0
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return bounds, kk


def resize_bilinear_u8(images: Sequence, size: Tuple[int, int] = (224, 224), device="cuda", _one_call: bool = False) -> torch.Tensor:
    """HWC uint8 RGB arrays / tensors of any sizes -> one uint8 ``[B, size[0], size[1], 3]`` tensor on ``device``,
    bit-identical to ``PIL.Image.fromarray(a).resize(size[::-1], Image.BILINEAR)`` per image."""
    out_h, out_w = int(size[0]), int(size[1])
    if len(images) == 0:
        return torch.empty((0, out_h, out_w, 3), dtype=torch.uint8, device=device)
    arrs = []
    for im in images:
        a = im.detach().cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError("resize_bilinear_u8: expected H×W×3 uint8 RGB images")
        if not _one_call and a.shape[0] > a.shape[1] * 100 and out_h < a.shape[0]:
            # Pillow (Image.py, >= 11) resizes an image more than 100x taller than wide in height first, then in width:
            # two single-axis passes here too (each rounds to 8 bits, so the order is visible in the last bit)
            a = resize_bilinear_u8([a], (out_h, a.shape[1]), device, _one_call=True)[0].cpu().numpy()
        arrs.append(np.ascontiguousarray(a))
    items = np.zeros(len(arrs), ITEM_DTYPE)
    tables, table_off, off = [], {}, 0

    def table(in_size, out_size):
        nonlocal off
        key = (in_size, out_size)
        if key not in table_off:
            b, k = bilinear_coeffs(in_size, out_size)
            table_off[key] = (off, off + b.size, k.shape[1])
            tables.extend([b.reshape(-1), k.reshape(-1)])
            off += b.size + k.size
        return table_off[key]

    src_off, lds_rows, rows_per_block = 0, 1, 8
    needs = []
    for i, a in enumerate(arrs):
        H, W, _ = a.shape
        it = items[i]
        it["src_off"], it["H"], it["W"] = src_off, H, W
        src_off += a.size
        if W != out_w:
            it["bx_off"], it["kx_off"], it["ksx"] = table(W, out_w)
        if H != out_h:
            it["by_off"], it["ky_off"], it["ksy"] = table(H, out_h)
            needs.append(bilinear_coeffs(H, out_h)[0])
    # rows per workgroup: as many as keep every block's input-row window within 64 KB of LDS
    def window(rpb):
        m = rpb
        for b in needs:
            first = b[0::rpb, 0]
            last_idx = np.minimum(np.arange(0, out_h, rpb) + rpb, out_h) - 1
            m = max(m, int((b[last_idx, 0] + b[last_idx, 1] - first).max()))
        return m
    while rows_per_block > 1 and window(rows_per_block) * out_w * 4 > 64 * 1024:
        rows_per_block //= 2
    lds_rows = window(rows_per_block)
    pool = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).to(device, non_blocking=True)
    items_d = torch.from_numpy(items.view(np.uint8).copy()).to(device, non_blocking=True)
    tab = np.concatenate(tables).astype(np.int32) if tables else np.zeros(1, np.int32)
    tab_d = torch.from_numpy(tab).to(device, non_blocking=True)
    out = torch.empty((len(arrs), out_h, out_w, 3), dtype=torch.uint8, device=pool.device)
    with torch.cuda.device(pool.device):
        _lib.check(_lib.load().frmap_resize_bilinear_u8(pool.data_ptr(), items_d.data_ptr(), tab_d.data_ptr(), out.data_ptr(),
                                                        len(arrs), out_h, out_w, rows_per_block, lds_rows,
                                                        torch.cuda.current_stream().cuda_stream), "resize_bilinear_u8")
    return out


def _plane(a) -> torch.Tensor:
    """A plane given as a tensor or an array -> a tensor that shares its memory.  Views of one numpy buffer become views of one
    storage, so that `YuvFrame.to` sees that they belong together."""
    if isinstance(a, torch.Tensor):
        return a
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise ValueError("YuvFrame: planes must be uint8")
    root = a
    while isinstance(root.base, np.ndarray):
        root = root.base
    if root is not a and root.dtype == np.uint8 and root.flags.c_contiguous and root.flags.writeable and all(st >= 0 for st in a.strides):
        off = a.__array_interface__["data"][0] - root.__array_interface__["data"][0]
        if 0 <= off and off + sum((n - 1) * st for n, st in zip(a.shape, a.strides)) < root.size:
            return torch.as_strided(torch.from_numpy(root.reshape(-1)), a.shape, a.strides, off)
    if any(st < 0 for st in a.strides) or not a.flags.writeable:
        a = np.array(a)
    return torch.from_numpy(a)


class YuvFrame:
    """One 4:2:0 frame of 8-bit samples, host or device, as three planes: ``y`` uint8 ``[H, W]`` with unit column stride, ``u`` and
    ``v`` uint8 ``[ceil(H/2), ceil(W/2)]`` views whose column stride is 1 (planar: I420, YV12) or 2 (interleaved: the halves of an
    NV12 / NV21 plane), the same for both, as is their row stride.  ``standard``: ``"bt601"`` or ``"bt709"``; ``full_range``: JPEG
    range instead of the video range 16..235 / 16..240.  `frames.yuv_to_rgb` states what its pixels are as RGB.

    `crop_resize_u8`, `align_crop_resize_u8` and the frame functions of `matching` take a `YuvFrame` wherever they take a frame:
    ``.shape == (H, W, 3)`` (the shape of the converted frame) and ``.device`` are what they look at.  Build one with `nv12_frame`,
    `nv21_frame` or `i420_frame`; planes of the wrong shape, dtype or stride, or on different devices, raise ``ValueError``."""

    def __init__(self, y, u, v, standard: str = "bt601", full_range: bool = False):
        self.csc = _frames.yuv_csc(standard, full_range)
        self.standard, self.full_range = standard, bool(full_range)
        y, u, v = _plane(y), _plane(u), _plane(v)
        for t in (y, u, v):
            if t.dtype != torch.uint8 or t.dim() != 2:
                raise ValueError("YuvFrame: planes must be 2-D uint8")
        H, W = int(y.shape[0]), int(y.shape[1])
        ch, cw = (H + 1) // 2, (W + 1) // 2
        if H < 1 or W < 1 or tuple(u.shape) != (ch, cw) or tuple(v.shape) != (ch, cw):
            raise ValueError(f"YuvFrame: a {H}x{W} luma plane needs chroma planes of {ch}x{cw}, got {tuple(u.shape)} and {tuple(v.shape)}")
        if y.device != u.device or y.device != v.device:
            raise ValueError("YuvFrame: the planes live on different devices")
        if (W > 1 and y.stride(1) != 1) or (H > 1 and y.stride(0) < W):
            raise ValueError("YuvFrame: the luma plane must have unit column stride and a row stride of at least W")
        c_step = u.stride(1) if cw > 1 else 1
        if cw > 1 and (c_step not in (1, 2) or v.stride(1) != c_step):
            raise ValueError("YuvFrame: u and v must have the same column stride, 1 (planar) or 2 (interleaved)")
        if ch > 1 and (u.stride(0) != v.stride(0) or u.stride(0) < c_step * cw):
            raise ValueError("YuvFrame: u and v must have the same row stride, at least c_step * ceil(W / 2)")
        self.y, self.u, self.v = y, u, v
        self.shape = (H, W, 3)
        self.y_pitch = int(y.stride(0)) if H > 1 else W
        self.c_pitch = int(u.stride(0)) if ch > 1 else c_step * cw
        self.c_step = int(c_step)

    @property
    def device(self):
        return self.y.device

    def planes(self):
        return self.y, self.u, self.v

    def to(self, device) -> "YuvFrame":
        """The frame on ``device``: one upload per distinct underlying buffer (an NV12 surface goes up in one piece, its three
        planes staying views of it; `nv12_frame(y, uv)` in two) - 1.5 bytes per pixel plus whatever padding the rows carry."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.y.device == device:
            return self
        groups = {}
        for t in self.planes():
            groups.setdefault(t.untyped_storage().data_ptr(), []).append(t)
        moved = {}
        for ts in groups.values():
            lo = min(t.storage_offset() for t in ts)
            hi = max(t.storage_offset() + sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1 for t in ts)
            flat = torch.as_strided(ts[0], (hi - lo,), (1,), lo).to(device, non_blocking=True)
            for t in ts:
                moved[id(t)] = torch.as_strided(flat, tuple(t.shape), t.stride(), t.storage_offset() - lo)
        return YuvFrame(moved[id(self.y)], moved[id(self.u)], moved[id(self.v)], self.standard, self.full_range)

    def record(self):
        """The frame's `YUV_FRAME_DTYPE` record (FrmapYuvFrame); the planes must be on the device the kernel runs on."""
        return (self.y.data_ptr(), self.u.data_ptr(), self.v.data_ptr(), self.shape[0], self.shape[1], self.y_pitch, self.c_pitch,
                self.c_step, self.csc)

    def __repr__(self):
        return f"YuvFrame({self.shape[0]}x{self.shape[1]}, c_step={self.c_step}, {self.standard}, {'full' if self.full_range else 'limited'}, {self.device})"


def _interleaved(what, y, uv, first, standard, full_range) -> YuvFrame:
    y = _plane(y)
    if uv is None:
        # the decoder's single buffer: H rows of luma, then H / 2 rows of interleaved chroma at the same pitch
        if y.dim() != 2 or y.shape[0] < 3 or y.shape[0] % 3 or y.shape[1] < 2 or y.shape[1] % 2:
            raise ValueError(f"{what}: a surface is uint8 [3 H / 2, W] with even H and W, got {tuple(y.shape)}")
        H = y.shape[0] // 3 * 2
        c = y[H:]
        planes = (c[:, 0::2], c[:, 1::2])
        return YuvFrame(y[:H], planes[first], planes[1 - first], standard, full_range)
    uv = _plane(uv)
    if uv.dim() != 3 or uv.shape[2] != 2:
        raise ValueError(f"{what}: the chroma plane must be uint8 [ceil(H/2), ceil(W/2), 2], got {tuple(uv.shape)}")
    if uv.stride(2) != 1 or (uv.shape[1] > 1 and uv.stride(1) != 2):
        raise ValueError(f"{what}: the chroma plane must hold its two samples next to each other (strides (pitch, 2, 1))")
    return YuvFrame(y, uv[:, :, first], uv[:, :, 1 - first], standard, full_range)


def nv12_frame(y, uv=None, standard: str = "bt601", full_range: bool = False) -> YuvFrame:
    """An NV12 frame: ``nv12_frame(y, uv)`` with ``y`` uint8 ``[H, W]`` and ``uv`` uint8 ``[ceil(H/2), ceil(W/2), 2]`` = (U, V) pairs,
    or ``nv12_frame(surface)`` with the decoder's single uint8 ``[3 H / 2, W]`` buffer (even ``H`` and ``W``; a view of a wider
    buffer - a padded pitch - is taken as it is).  Tensors or arrays, host or device; nothing is copied."""
    return _interleaved("nv12_frame", y, uv, 0, standard, full_range)


def nv21_frame(y, vu=None, standard: str = "bt601", full_range: bool = False) -> YuvFrame:
    """`nv12_frame` with the chroma pairs in (V, U) order."""
    return _interleaved("nv21_frame", y, vu, 1, standard, full_range)


def i420_frame(y, u, v, standard: str = "bt601", full_range: bool = False) -> YuvFrame:
    """A planar frame: ``y`` uint8 ``[H, W]``, ``u`` and ``v`` uint8 ``[ceil(H/2), ceil(W/2)]`` with equal row strides (YV12: hand
    the planes over in this order all the same).  Tensors or arrays, host or device; nothing is copied."""
    return YuvFrame(y, u, v, standard, full_range)


def _device_frames(frames, device) -> list:
    """``frames`` (one [H,W,3] / [F,H,W,3] uint8 tensor or array, or a sequence of [H,W,3] ones) -> a list of [H,W,3] uint8 device
    tensors with unit channel stride and 3-byte pixels (rows may be padded: a view of a wider buffer is taken as it is).  A host
    frame, or a host stack of frames, is uploaded once.  A `YuvFrame` stays one (`YuvFrame.to` uploads a host one)."""
    if isinstance(frames, (list, tuple)):
        out = []
        for f in frames:
            out.extend(_device_frames(f, device))
        return out
    if isinstance(frames, YuvFrame):
        return [frames if frames.device.type == "cuda" else frames.to(device)]
    t = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
    if t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3 or min(t.shape) < 1:
        raise ValueError("crop_resize_u8: frames must be uint8 [H, W, 3] or [F, H, W, 3]")
    if not t.is_cuda:
        t = t.to(device, non_blocking=True)
    if t.stride(-1) != 1 or t.stride(-2) != 3 or t.stride(-3) < 3 * t.shape[-2]:
        t = t.contiguous()
    return [t] if t.dim() == 3 else list(t.unbind(0))


def _frames_and_rois(what: str, frames, rois, size, device):
    """The argument checks `crop_resize_u8` and `align_crop_resize_u8` share: ``(out_h, out_w, device frames, their device,
    rois int64 [N, 5])``, every ROI inside its frame; ``ValueError`` otherwise."""
    out_h, out_w = int(size[0]), int(size[1])
    if out_h < 1 or out_w < 1:
        raise ValueError(f"{what}: size must be positive")
    r = rois.detach().cpu().numpy() if isinstance(rois, torch.Tensor) else np.asarray(rois)
    if r.size == 0:
        r = np.zeros((0, 4), np.int64)                   # (an empty list has no integer dtype to check)
    if r.ndim != 2 or r.shape[1] not in (4, 5) or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"{what}: rois must be integers of shape [N, 4] or [N, 5]")
    r = r.astype(np.int64)
    if r.shape[1] == 4:
        r = np.concatenate([np.zeros((r.shape[0], 1), np.int64), r], 1)
    fr = _device_frames(frames, device)
    if len({isinstance(f, YuvFrame) for f in fr}) > 1:
        raise ValueError(f"{what}: YUV frames and packed frames cannot be mixed in one call")
    dev = fr[0].device
    if any(f.device != dev for f in fr):
        raise ValueError(f"{what}: frames live on different devices")
    if r.shape[0]:
        fi, x1, y1, x2, y2 = r.T
        if fi.min() < 0 or fi.max() >= len(fr):
            raise ValueError(f"{what}: frame index outside [0, {len(fr)})")
        Hs, Ws = np.array([f.shape[0] for f in fr])[fi], np.array([f.shape[1] for f in fr])[fi]
        bad = (x1 < 0) | (y1 < 0) | (x2 > Ws) | (y2 > Hs) | (x2 <= x1) | (y2 <= y1)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise ValueError(f"{what}: ROI {i} {tuple(int(v) for v in r[i, 1:])} is empty or leaves its {int(Ws[i])}x{int(Hs[i])} frame")
    return out_h, out_w, fr, dev, r


def _frame_records(fr) -> np.ndarray:
    if isinstance(fr[0], YuvFrame):
        desc = np.zeros(len(fr), YUV_FRAME_DTYPE)
        for j, f in enumerate(fr):
            desc[j] = f.record()
        return desc
    desc = np.zeros(len(fr), FRAME_DTYPE)
    for j, f in enumerate(fr):
        desc[j] = (f.data_ptr(), f.shape[0], f.shape[1], f.stride(0))
    return desc


def _crop_launches(what: str, fr, dev, r, m, out_h: int, out_w: int, bgr: bool) -> torch.Tensor:
    """What `crop_resize_u8` (``m`` None) and `align_crop_resize_u8` (``m`` float64 ``[N, 6]``) do with checked arguments, for packed
    frames and `YuvFrame`s on ``dev`` alike: records | (matrices) | rois in one upload and one launch for the ROIs that keep Pillow's
    usual pass order; a ROI more than 100x taller than wide whose height shrinks takes the other order - the kernel cuts it out
    at its own size (both axes copied: the crop itself, converted, rotated, RGB) and `resize_bilinear_u8` resizes that."""
    N = r.shape[0]
    out = torch.empty((N, out_h, out_w, 3), dtype=torch.uint8, device=dev)
    if N == 0:
        return out
    yuv = isinstance(fr[0], YuvFrame)
    h, w = r[:, 4] - r[:, 2], r[:, 3] - r[:, 1]
    tall = (h > 100 * w) & (out_h < h)
    desc = _frame_records(fr).view(np.uint8)
    entry = getattr(_lib.load(), ("frmap_crop_resize" if m is None else "frmap_align_crop_resize") + ("_yuv" if yuv else "_u8"))

    def launch(sel, dst, oh, ow):
        # the records are 24 (YUV: 56) and 48 bytes, so the doubles stay 8-byte aligned
        mats = [] if m is None else [m[sel].view(np.uint8).reshape(-1)]
        tab = torch.from_numpy(np.concatenate([desc] + mats + [r[sel].astype(np.int32).view(np.uint8).reshape(-1)])).to(dev, non_blocking=True)
        p_m = tab.data_ptr() + desc.nbytes
        p_r = p_m + 48 * len(sel) * len(mats)
        name = entry.__name__
        for arg, ptr in (("frames", tab.data_ptr()), ("rois", p_r)) + ((("mats", p_m),) if mats else ()):     # (this upload's own layout)
            assert ptr % _lib.align_of(name, arg) == 0, (name, arg, ptr)
        args = [tab.data_ptr(), len(fr), p_r] + [p_m] * len(mats) + [dst.data_ptr(), len(sel), oh, ow, int(h[sel].max()), int(w[sel].max())]
        with torch.cuda.device(dev):
            _lib.check(entry(*args, *([] if yuv else [int(bool(bgr))]), torch.cuda.current_stream().cuda_stream), what)

    keep = np.flatnonzero(~tall)
    if keep.size:
        dst = out if keep.size == N else torch.empty((keep.size, out_h, out_w, 3), dtype=torch.uint8, device=dev)
        launch(keep, dst, out_h, out_w)
        if dst is not out:
            out[torch.from_numpy(keep).to(dev)] = dst
    for i in np.flatnonzero(tall):
        crop = torch.empty((1, int(h[i]), int(w[i]), 3), dtype=torch.uint8, device=dev)
        launch(np.array([i]), crop, int(h[i]), int(w[i]))
        out[int(i)] = resize_bilinear_u8([crop[0]], (out_h, out_w), dev)[0]
    return out


def crop_resize_u8(frames, rois, size: Tuple[int, int] = (160, 160), bgr: bool = False, device="cuda") -> torch.Tensor:
    """Crops of frames, resized on the device: uint8 ``[N, size[0], size[1], 3]`` RGB, crop i bit-identical to
    ``PIL.Image.fromarray(rgb_frame[y1:y2, x1:x2]).resize(size[::-1], Image.BILINEAR)`` - the reference's
    ``frame[y1:y2, x1:x2]`` + ``[:, :, ::-1]`` + ``Resize`` (`src/app.py:234, 32-39`) for all boxes of a detector in one launch.

    ``frames``: uint8 ``[H, W, 3]`` or ``[F, H, W, 3]`` tensor / array, or a sequence of ``[H, W, 3]`` frames of any sizes, on the host
    (uploaded once, not once per crop) or on the device (used in place, padded rows included).  ``rois``: host integers ``[N, 4]`` =
    ``(x1, y1, x2, y2)`` in frame 0, or ``[N, 5]`` with a leading frame index; a ROI that is empty or leaves its frame raises
    ``ValueError``.  ``bgr``: the frames are BGR (cv2) and come out RGB.  The filter taps are computed by the kernel
    (`frmap_crop_resize_u8`): no table per box size is built on the host.  A ROI more than 100x taller than wide whose height shrinks
    takes Pillow's other pass order: the kernel cuts it out at its own size and `resize_bilinear_u8` resizes that.

    ``frames`` may also be a `YuvFrame` (NV12, NV21, I420; `nv12_frame` ...) or a sequence of them, of any sizes, layouts and colour
    standards, host or device: crop i is then bit-identical to this function on ``frames.yuv_to_rgb`` of the frame, computed by
    `frmap_crop_resize_yuv` in the same single launch, each filter tap converting the pixel it reads - no RGB frame is written.
    ``bgr`` is ignored for YUV frames.  A sequence that mixes YUV and packed frames raises ``ValueError``."""
    out_h, out_w, fr, dev, r = _frames_and_rois("crop_resize_u8", frames, rois, size, device)
    return _crop_launches("crop_resize_u8", fr, dev, r, None, out_h, out_w, bgr)


def align_crop_resize_u8(frames, rois, matrices, size: Tuple[int, int] = (160, 160), bgr: bool = False, device="cuda") -> torch.Tensor:
    """Crops of ROTATED frames, resized on the device in one launch, with no rotated frame in memory: uint8
    ``[N, size[0], size[1], 3]`` RGB, crop i bit-identical to

        ``Image.fromarray(rgb_frame).rotate(angle_i, resample=Image.BILINEAR, center=center_i)``      (same size, fill 0)
        ``.crop((x1, y1, x2, y2)).resize(size[::-1], Image.BILINEAR)``

    where ``matrices[i] = frames.rotation_matrix(angle_i, center_i)`` - the reference's eye alignment (`src/data_prep.py:69-87`:
    rotate the whole image about the point between the eyes, `frames.eye_rotation`), margin box (`frames.margin_boxes`), crop and
    resize (`:144-150`).  DEPARTURE from the reference: it resamples with `cv2.warpAffine` / `cv2.resize`; this function takes the
    angle, the centre and the "rotate the frame, then crop" order from it and the resampling from Pillow, as every image operation
    of this package does - its output is Pillow's to the bit, not cv2's.

    ``frames``, ``rois``, ``bgr``: as `crop_resize_u8` (the ROI is in the rotated frame, which has the frame's size; same
    ``ValueError``s).  ``matrices``: float64 ``[N, 6]``, Pillow's output -> input affine matrix per ROI; a shape mismatch or a
    non-finite entry raises ``ValueError``.  Frames, ROIs and matrices go up in one upload; the kernel (`frmap_align_crop_resize_u8`)
    warps each source pixel where a filter tap reads it.  A ROI more than 100x taller than wide whose height shrinks takes Pillow's
    other pass order: its rotated crop is made by the kernel at its own size and resized by `resize_bilinear_u8`.

    ``frames`` may also be `YuvFrame`s, as for `crop_resize_u8`: crop i is then bit-identical to this function on
    ``frames.yuv_to_rgb`` of the frame (`frmap_align_crop_resize_yuv`: the four corner pixels of a warp sample are converted first,
    what rotates in from outside is RGB 0).  ``bgr`` is ignored for YUV frames; mixing YUV and packed frames raises ``ValueError``."""
    out_h, out_w, fr, dev, r = _frames_and_rois("align_crop_resize_u8", frames, rois, size, device)
    N = r.shape[0]
    m = np.ascontiguousarray(matrices.detach().cpu().numpy() if isinstance(matrices, torch.Tensor) else matrices, dtype=np.float64)
    if m.size == 0:
        m = m.reshape(0, 6)
    if m.shape != (N, 6):
        raise ValueError(f"align_crop_resize_u8: matrices must have shape [{N}, 6], one per ROI, got {tuple(m.shape)}")
    if not np.isfinite(m).all():
        raise ValueError(f"align_crop_resize_u8: matrix {int(np.flatnonzero(~np.isfinite(m).all(1))[0])} has a non-finite entry")
    return _crop_launches("align_crop_resize_u8", fr, dev, r, m, out_h, out_w, bgr)
