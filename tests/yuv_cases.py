"""What the YUV-frame tests share (`test_yuv_cpu.py`, `test_yuv_gpu.py`, `test_guard_yuv_gpu.py`): seeded random planes - every
byte triple is a valid (Y, U, V), so random bytes reach every clip branch of the conversion -, builders that lay them out as NV12,
NV21, I420 and a decoder's single surface inside padded buffers, the converted RGB frame every comparison is made against
(`frames.yuv_to_rgb`, computed once per frame), and the ROI lists.  A plain helper module like `align_cases.py`; not a test module.

Every comparison of these tests is on bits: a crop of a YUV frame must equal the existing crop of the converted frame."""
import numpy as np

from frmap_amd import frames, resize

CSC = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]       # csc code = index
FORMATS = ("nv12", "nv21", "i420")
PAD = 0xC3                                                                         # what the padding of every buffer holds
SIZES = ((37, 53), (64, 48))                                                       # (H, W): odd both ways; even
_PLANES, _RGB = {}, {}


def planes(H, W, seed=0):
    """(y [H, W], u, v [ceil(H/2), ceil(W/2)]) of random bytes, the same for the same arguments; read-only."""
    key = (H, W, seed)
    if key not in _PLANES:
        rng = np.random.default_rng([20251019, H, W, seed])
        p = tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((H, W), ((H + 1) // 2, (W + 1) // 2), ((H + 1) // 2, (W + 1) // 2)))
        for a in p:
            a.setflags(write=False)
        _PLANES[key] = p
    return _PLANES[key]


def rgb(H, W, csc, seed=0):
    """The converted frame: `frames.yuv_to_rgb` of `planes(H, W, seed)` under row `csc`, computed once; read-only."""
    key = (H, W, seed, csc)
    if key not in _RGB:
        a = frames.yuv_to_rgb(*planes(H, W, seed), *CSC[csc])
        a.setflags(write=False)
        _RGB[key] = a
    return _RGB[key]


def _padded(shape, pad_cols, lead=0):
    """A `PAD`-filled buffer whose rows are `pad_cols` samples wider than `shape`, and the view of it that starts `lead` columns in."""
    buf = np.full((shape[0], shape[1] + pad_cols) + tuple(shape[2:]), PAD, np.uint8)
    return buf[:, lead:lead + shape[1]]


def layout(fmt, y, u, v, pad=True):
    """The planes copied into fresh buffers in layout `fmt`: `(y view, u view, v view, pairs)`, views of padded buffers (pitches >
    width) unless `pad` is False.  nv12 / nv21: u and v are the two halves of `pairs`, one interleaved `[ch, cw, 2]` view (column
    stride 2); i420: `pairs` is None."""
    H, W = y.shape
    yb = _padded((H, W), 11 if pad else 0, 3 if pad else 0)
    yb[:] = y
    if fmt == "i420":
        ub, vb = _padded(u.shape, 5 if pad else 0, 2 if pad else 0), _padded(u.shape, 5 if pad else 0, 1 if pad else 0)
        ub[:], vb[:] = u, v
        return yb, ub, vb, None
    c = _padded(u.shape + (2,), 3 if pad else 0, 1 if pad else 0)
    first = 0 if fmt == "nv12" else 1
    c[:, :, first], c[:, :, 1 - first] = u, v
    return yb, c[:, :, first], c[:, :, 1 - first], c


def frame(fmt, H, W, csc, seed=0, device=None, pad=True):
    """A `resize.YuvFrame` of `planes(H, W, seed)` in layout `fmt` through the package's constructors; `device`: where the planes
    live (None: host arrays, else torch tensors there, padding included)."""
    yb, ub, vb, pairs = layout(fmt, *planes(H, W, seed), pad)
    std, full = CSC[csc]
    parts = [yb, ub, vb] if fmt == "i420" else [yb, pairs]
    if device is not None:
        parts = [_to_device(p, device) for p in parts]
    make = {"nv12": resize.nv12_frame, "nv21": resize.nv21_frame, "i420": resize.i420_frame}[fmt]
    return make(*parts, standard=std, full_range=full)


def _to_device(view, device):
    """A padded host view on `device` with its padding: the underlying buffer goes up whole and the same window is cut out."""
    import torch
    base = view
    while isinstance(base.base, np.ndarray):
        base = base.base
    off = view.__array_interface__["data"][0] - base.__array_interface__["data"][0]
    t = torch.from_numpy(base.reshape(-1).copy()).to(device)
    return torch.as_strided(t, view.shape, view.strides, off)


def surface(H, W, seed=0, pad=True):
    """A decoder's single NV12 buffer `[3 H / 2, W]` (even H, W) of `planes(H, W, seed)`, a view of a wider buffer when `pad`."""
    assert H % 2 == 0 and W % 2 == 0
    y, u, v = planes(H, W, seed)
    s = _padded((3 * H // 2, W), 16 if pad else 0, 0)
    s[:H] = y
    s[H:, 0::2], s[H:, 1::2] = u, v
    return s


def rois(H, W):
    """(x1, y1, x2, y2) of an H x W frame: the full frame; 1 x 1 at even and at odd coordinates; odd x1 / y1 (the chroma phase comes
    from the frame, not from the ROI); everything but the first row and column; the last row, the last column, the last pixel."""
    return [(0, 0, W, H), (W // 2 & ~1, H // 2 & ~1, (W // 2 & ~1) + 1, (H // 2 & ~1) + 1), (5, 7, 6, 8), (3, 5, 3 + 20, 5 + 17),
            (1, 1, W, H), (0, H - 1, W, H), (W - 1, 0, W, H), (W - 1, H - 1, W, H), (2, 4, 2 + 31, 4 + 17), (9, 1, 9 + 20, 1 + 30)]


# output sizes (out_h, out_w): upscale; the heaviest reduction; the size of ROI (3, 5, 23, 22) - a copy on both axes, and of its
# height alone for ROI (2, 4, 33, 21), its width alone for ROI (9, 1, 29, 31) -; one axis equal to those ROIs' and the other not
OUT_SIZES = ((160, 160), (8, 8), (17, 20), (17, 40), (40, 20))
TALL = (404, 8, (2, 0, 6, 404))                                                    # a 404 x 8 frame and its 404 x 4 ROI

# (angle, centre as a function of (H, W)) of the aligned crops: a small tilt inside the frame; rotations that throw part of the
# source outside the frame (black fill) and put samples on its clamped edge; a quarter turn; everything outside
ALIGN = [(3.7, lambda H, W: (W // 2, H // 2)), (-12.25, lambda H, W: (W / 3.0, H * 0.61)), (29.999, lambda H, W: (0, 0)),
         (90.0, lambda H, W: (W - 10.5, 22.0)), (171.3, lambda H, W: (W, H)), (0.0, lambda H, W: (W // 2, H // 2)),
         (180.0, lambda H, W: (-200.0, -200.0))]
ALIGN_SIZES = ((160, 160), (8, 8), (17, 20))


def align_cases(H, W):
    """(roi, angle, centre): every rotation of `ALIGN` on the full frame, an odd-offset box (the ROI-sized output of `ALIGN_SIZES`)
    and the last rows / columns."""
    out = []
    for angle, c in ALIGN:
        for roi in ((0, 0, W, H), (3, 5, 3 + 20, 5 + 17), (W - 9, H - 7, W, H)):
            out.append((roi, angle, tuple(float(v) for v in c(H, W))))
    return out


def float_rgb(csc):
    """The float64 formula the fixed-point rule approximates, over ALL 2^24 (Y, U, V) triples: uint8 [256, 256, 256, 3] indexed
    [Y, U, V], `clip(floor(x + 0.5))` of R = sy (Y - y_off) + 2 (1 - Kr) sc (V - 128) and so on, from (Kr, Kb) and the range."""
    std, full = CSC[csc]
    kr, kb = frames.YUV_KR_KB[std]
    kg = 1.0 - kr - kb
    sy, sc, y_off = (1.0, 1.0, 0) if full else (255.0 / 219.0, 255.0 / 224.0, 16)
    Y = (np.arange(256, dtype=np.float64) - y_off)[:, None, None] * sy
    U = (np.arange(256, dtype=np.float64) - 128.0)[None, :, None] * sc
    V = (np.arange(256, dtype=np.float64) - 128.0)[None, None, :] * sc
    chans = (Y + 2.0 * (1.0 - kr) * V + 0.0 * U, Y - 2.0 * kb * (1.0 - kb) / kg * U - 2.0 * kr * (1.0 - kr) / kg * V, Y + 2.0 * (1.0 - kb) * U + 0.0 * V)
    return np.stack([np.clip(np.floor(c + 0.5), 0, 255).astype(np.uint8) for c in chans], axis=-1)


_SWEEP = []


def sweep_planes():
    """All 2^24 triples as ONE 4096 x 4096 4:2:0 frame: chroma sample c = row * 2048 + column holds (U, V) = (c % 65536 >> 8,
    c % 256), and the four luma samples under the k-th sample of a (U, V) pair (k = c // 65536 < 64) hold Y = 4 k + (0, 1, 2, 3):
    every pair meets every Y exactly once.  (y, u, v), built once, read-only."""
    if not _SWEEP:
        c = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
        u, v = ((c % 65536) >> 8).astype(np.uint8), (c % 256).astype(np.uint8)
        y = np.repeat(np.repeat((4 * (c // 65536)).astype(np.uint8), 2, 0), 2, 1)
        y[0::2, 1::2] += 1
        y[1::2, 0::2] += 2
        y[1::2, 1::2] += 3
        for a in (y, u, v):
            a.setflags(write=False)
        _SWEEP.append((y, u, v))
    return _SWEEP[0]
