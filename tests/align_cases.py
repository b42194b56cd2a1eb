"""What the crop tests share: the Pillow resize a plain crop must equal; Pillow's `Image.rotate(angle, BILINEAR, center=c)`
restated in numpy (the arithmetic `frmap_align_warp_host` and the kernel run - Geometry.c's affine transform with the bilinear
filter on an 8-bit RGB image); the Pillow chain an aligned crop must equal; the angle / centre lists of the aligned-crop tests.
Not a test module."""
import math

import numpy as np
from PIL import Image

ANGLES = [0.0, 1e-9, 3.7, -3.7, -12.25, 29.999, 45.0, 90.0, -90.0, 180.0, 171.3, 359.5, -400.0]


def pil_matrix(angle, center):
    """`Image.rotate`'s output -> input matrix (Image.py): `angle % 360.0`, cos / sin of the negated angle rounded to 15 decimals,
    the translation that keeps `center` fixed."""
    angle = -math.radians(angle % 360.0)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = center
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def pil_crop(frame, roi, out_h, out_w, bgr=False):
    """The contract of a plain crop: the installed Pillow's bilinear resize of the frame's slice (BGR frames come out RGB)."""
    x1, y1, x2, y2 = roi
    a = frame[y1:y2, x1:x2]
    if bgr:
        a = a[:, :, ::-1]
    return np.asarray(Image.fromarray(np.ascontiguousarray(a)).resize((out_w, out_h), Image.BILINEAR))


def pil_rotate(rgb, angle, center):
    """The installed Pillow: the rotated frame, same size, black fill."""
    return np.asarray(Image.fromarray(rgb).rotate(angle, resample=Image.BILINEAR, center=center))


def numpy_rotate(rgb, m):
    """The restatement: per output pixel, float64, Pillow's operation order (`affine_transform` + `bilinear_filter32RGB`)."""
    H, W, _ = rgb.shape
    a, b, c, d, e, f = (np.float64(v) for v in m)
    xo, yo = np.meshgrid(np.arange(W, dtype=np.float64) + 0.5, np.arange(H, dtype=np.float64) + 0.5)
    xin, yin = a * xo + b * yo + c, d * xo + e * yo + f
    inside = (xin >= 0.0) & (xin < W) & (yin >= 0.0) & (yin < H)
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    x, y = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = (xin - x)[..., None], (yin - y)[..., None]
    x0, x1, yc = np.clip(x, 0, W - 1), np.clip(x + 1, 0, W - 1), np.clip(y, 0, H - 1)
    px = rgb.astype(np.int64)
    p, q = px[yc, x0], px[yc, x1]
    v1 = p + (q - p) * dx
    has = (y + 1 >= 0) & (y + 1 < H)
    y1 = np.where(has, y + 1, 0)
    p, q = px[y1, x0], px[y1, x1]
    v2 = np.where(has[..., None], p + (q - p) * dx, v1)
    out = (v1 + (v2 - v1) * dy).astype(np.uint8)          # (UINT8) cast of a value in [0, 255]: truncation
    return np.where(inside[..., None], out, np.uint8(0))


def pil_chain(rgb, angle, center, roi, out_h, out_w):
    """The contract of an aligned crop: rotate the whole frame about `center`, crop the box, resize."""
    x1, y1, x2, y2 = roi
    im = Image.fromarray(rgb).rotate(angle, resample=Image.BILINEAR, center=center)
    return np.asarray(im.crop((x1, y1, x2, y2)).resize((out_w, out_h), Image.BILINEAR))


def centers(H, W):
    """Inside the frame (integers, fractions, one that puts a sample exactly on the right edge at 90 degrees), on a corner, outside."""
    return [(W // 2, H // 2), (W / 3.0, H * 0.61), (W - 10.5, 22.0), (0, 0), (W, H), (-15.5, H + 40.0), (2.5 * W, -7.0)]
