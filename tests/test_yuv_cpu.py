"""CPU: the host-checkable half of the YUV frames - the conversion rule (`frames.YUV_COEFFS`, `frames.yuv_to_rgb`) against the
float64 formula over all 2^24 (Y, U, V) triples, the kernels' pixel functions compiled for the CPU (`frmap_yuv_to_rgb_host`,
`frmap_yuv_align_warp_host`) against the rule and against `frmap_align_warp_host` on the converted frame, bit for bit, the same
functions under the address / undefined-behaviour sanitizers as a stand-alone program, the C ABI of the new entry points, and
`resize.YuvFrame` with its constructors.  Nothing here has a tolerance: "max |diff| <= 1" and the share of differing triples are
properties of the rule against float64, stated by the rule's author and restated here."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import align_cases as ac
import yuv_cases as yc
from frmap_amd import _lib, frames, resize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "facerecognition-multiarchitecture-pipeline_amd")


# --------------------------------------------------------------------------------------------------------------------------------
# the rule
# --------------------------------------------------------------------------------------------------------------------------------
def test_the_table_is_the_kr_kb_derivation_rounded_to_16_bits():
    want = {0: (16, 76309, 104597, -25675, -53279, 132201), 1: (0, 65536, 91881, -22553, -46802, 116130),
            2: (16, 76309, 117489, -13975, -34925, 138438), 3: (0, 65536, 103206, -12276, -30679, 121609)}
    assert frames.YUV_COEFFS == want
    for csc, (std, full) in enumerate(yc.CSC):
        assert frames.yuv_csc(std, full) == csc
        kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[std]
        kg = 1.0 - kr - kb
        sy, sc = (1.0, 1.0) if full else (255.0 / 219.0, 255.0 / 224.0)
        coeffs = (sy, 2 * (1 - kr) * sc, -2 * kb * (1 - kb) / kg * sc, -2 * kr * (1 - kr) / kg * sc, 2 * (1 - kb) * sc)
        assert want[csc] == (0 if full else 16,) + tuple(int(math.floor(c * 65536 + 0.5)) for c in coeffs), csc
    with pytest.raises(ValueError):
        frames.yuv_csc("bt2020")
    # the table of the kernels' header is this table
    text = open(os.path.join(PKG, "csrc", "yuv_pixel.h")).read()
    rows = re.findall(r"FrmapYuvCsc\{(-?\d+), (-?\d+), (-?\d+), (-?\d+), (-?\d+), (-?\d+)\}", text)
    assert [tuple(int(v) for v in r) for r in rows] == [want[i] for i in range(4)]


@pytest.mark.parametrize("csc", range(4))
def test_yuv_to_rgb_against_float64_over_all_triples(csc):
    """All 2^24 triples (one 4096 x 4096 frame): at most 1 away from clip(floor(float64 + 0.5)), different at all in fewer than
    0.06 % of the triples per channel, |sum| below 3.6e7, and the host function equals the numpy rule on every byte."""
    y, u, v = yc.sweep_planes()
    got = frames.yuv_to_rgb(y, u, v, *yc.CSC[csc])
    yi, xi = np.arange(4096)[:, None] >> 1, np.arange(4096)[None, :] >> 1
    uu, vv = u[yi, xi], v[yi, xi]
    if csc == 0:                                                             # the frame holds every triple exactly once
        key = (y.astype(np.int32) << 16) | (uu.astype(np.int32) << 8) | vv
        assert np.array_equal(np.sort(key, axis=None), np.arange(1 << 24, dtype=np.int32))
    want = yc.float_rgb(csc)[y, uu, vv]
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    share = [float((diff[..., c] != 0).mean()) for c in range(3)]
    print(f"csc {csc}: max |fixed - float64| = {int(diff.max())}, differing triples per channel = {[f'{100 * s:.4f} %' for s in share]}")
    assert int(diff.max()) <= 1
    assert max(share) < 0.0006
    y_off, cy, rv, gu, gv, bu = frames.YUV_COEFFS[csc]
    extreme = max(abs(cy * (yy - y_off) + a * (s1 - 128) + b * (s2 - 128) + 32768)
                  for yy in (0, 255) for s1 in (0, 255) for s2 in (0, 255) for a, b in ((rv, 0), (gu, gv), (bu, 0)))
    assert extreme < 3.6e7
    out = np.full((4096, 4096, 3), 0xA5, np.uint8)
    rc = _lib.load().frmap_yuv_to_rgb_host(y.ctypes.data, u.ctypes.data, v.ctypes.data, 4096, 4096, 4096, 2048, 1, csc, out.ctypes.data)
    assert rc == 0, _lib.load().frmap_last_error()
    assert np.array_equal(out, got)


@pytest.mark.parametrize("csc", range(4))
def test_grey_axis_is_neutral(csc):
    y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    c = np.full((8, 8), 128, np.uint8)
    g = frames.yuv_to_rgb(y, c, c, *yc.CSC[csc])
    assert np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 1], g[..., 2])
    if yc.CSC[csc][1]:
        assert np.array_equal(g[..., 0], y)                                  # full range: grey is the luma itself
    else:
        assert g[0, 0, 0] == 0 and g[1, 0, 0] == 0 and g[1, 1, 0] == 1 and g[14, 11, 0] == 255 and g[15, 15, 0] == 255   # 16 -> 0, 235 -> 255


def test_yuv_to_rgb_takes_chroma_from_the_frames_grid_and_checks_its_arguments():
    """Pixel (x, y) takes chroma (x >> 1, y >> 1): written out pixel by pixel in Python integers for an odd frame."""
    H, W = 5, 7
    y, u, v = yc.planes(H, W, 3)
    for csc in range(4):
        y_off, cy, rv, gu, gv, bu = frames.YUV_COEFFS[csc]
        got = frames.yuv_to_rgb(y, u, v, *yc.CSC[csc])
        assert got.shape == (H, W, 3) and got.dtype == np.uint8
        for yy in range(H):
            for xx in range(W):
                Y, U, V = int(y[yy, xx]) - y_off, int(u[yy >> 1, xx >> 1]) - 128, int(v[yy >> 1, xx >> 1]) - 128
                want = [min(255, max(0, s >> 16)) for s in (cy * Y + rv * V + 32768, cy * Y + gu * U + gv * V + 32768, cy * Y + bu * U + 32768)]
                assert got[yy, xx].tolist() == want, (csc, yy, xx)
    # any strides: the halves of an interleaved plane
    _, ub, vb, pairs = yc.layout("nv12", y, u, v)
    assert ub.strides[1] == 2 and np.array_equal(frames.yuv_to_rgb(y, pairs[..., 0], pairs[..., 1]), frames.yuv_to_rgb(y, u, v))
    for bad in ((y, u[:-1], v), (y, u, v[:, :-1]), (y.astype(np.int32), u, v), (y[0], u, v), (y, u.astype(np.float32), v)):
        with pytest.raises(ValueError):
            frames.yuv_to_rgb(*bad)


# --------------------------------------------------------------------------------------------------------------------------------
# the kernels' pixel functions on the CPU
# --------------------------------------------------------------------------------------------------------------------------------
def _host_rgb(yb, ub, vb, csc, c_step=None):
    H, W = yb.shape
    out = np.full((H, W, 3), 0xA5, np.uint8)
    ch, cw = ub.shape
    c_step = (ub.strides[1] if cw > 1 else 1) if c_step is None else c_step
    rc = _lib.load().frmap_yuv_to_rgb_host(yb.ctypes.data, ub.ctypes.data, vb.ctypes.data, H, W, yb.strides[0] if H > 1 else W,
                                           ub.strides[0] if ch > 1 else c_step * cw, c_step, csc, out.ctypes.data)
    assert rc == 0, _lib.load().frmap_last_error()
    return out


@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (5, 7), (37, 53)])
def test_host_conversion_equals_the_rule(hw):
    """`frmap_yuv_to_rgb_host` == `frames.yuv_to_rgb`: planar and interleaved, u / v swapped, tight and padded pitches, all csc."""
    H, W = hw
    y, u, v = yc.planes(H, W, 1)
    for csc in range(4):
        want = frames.yuv_to_rgb(y, u, v, *yc.CSC[csc])
        swapped = frames.yuv_to_rgb(y, v, u, *yc.CSC[csc])
        if hw != (1, 1):
            assert not np.array_equal(want, swapped)
        for fmt in yc.FORMATS:
            for pad in (False, True):
                yb, ub, vb, _ = yc.layout(fmt, y, u, v, pad)
                if pad and H > 1:
                    assert yb.strides[0] > W and ub.strides[0] > ub.strides[1] * ub.shape[1]
                step = 1 if fmt == "i420" else 2
                assert np.array_equal(_host_rgb(yb, ub, vb, csc, step), want), (csc, fmt, pad)
                assert np.array_equal(_host_rgb(yb, vb, ub, csc, step), swapped), (csc, fmt, pad)


def _warp_host(f, m, roi):
    x1, y1, x2, y2 = roi
    out = np.full((y2 - y1, x2 - x1, 3), 0xA5, np.uint8)
    m = np.ascontiguousarray(m, dtype=np.float64)
    rc = _lib.load().frmap_yuv_align_warp_host(f.y.data_ptr(), f.u.data_ptr(), f.v.data_ptr(), f.shape[0], f.shape[1], f.y_pitch, f.c_pitch,
                                               f.c_step, f.csc, m.ctypes.data, x1, y1, x2, y2, out.ctypes.data)
    assert rc == 0, _lib.load().frmap_last_error()
    return out


def _warp_host_rgb(rgb, m, roi):
    x1, y1, x2, y2 = roi
    out = np.full((y2 - y1, x2 - x1, 3), 0x5A, np.uint8)
    m = np.ascontiguousarray(m, dtype=np.float64)
    rc = _lib.load().frmap_align_warp_host(rgb.ctypes.data, rgb.shape[0], rgb.shape[1], rgb.strides[0], m.ctypes.data, x1, y1, x2, y2, 0,
                                           out.ctypes.data)
    assert rc == 0, _lib.load().frmap_last_error()
    return out


@pytest.mark.parametrize("fmt", yc.FORMATS)
@pytest.mark.parametrize("hw", [(37, 53), (64, 48)])
def test_host_warp_equals_the_warp_of_the_converted_frame(hw, fmt):
    """`frmap_yuv_align_warp_host` == `frmap_align_warp_host` on `frames.yuv_to_rgb` of the frame, for every angle and centre of
    `align_cases` (inside the frame, on a corner, outside it) - and so equals Pillow's `Image.rotate`, which the latter is pinned to."""
    H, W = hw
    for csc in range(4):
        f = yc.frame(fmt, H, W, csc)
        rgb = np.ascontiguousarray(yc.rgb(H, W, csc))
        for angle in ac.ANGLES:
            for center in ac.centers(H, W):
                m = frames.rotation_matrix(angle, center)
                for roi in ((0, 0, W, H), (3, 5, 23, 22), (W - 1, H - 1, W, H)):
                    assert np.array_equal(_warp_host(f, m, roi), _warp_host_rgb(rgb, m, roi)), (csc, angle, center, roi)
    assert np.array_equal(_warp_host(f, frames.rotation_matrix(0.0, (3, 4)), (0, 0, W, H)), rgb)             # angle 0: the conversion
    assert int(_warp_host(f, frames.rotation_matrix(180.0, (-200.0, -200.0)), (0, 0, W, H)).max()) == 0      # all outside: RGB 0
    assert np.array_equal(_warp_host(f, ac.pil_matrix(-12.25, (20.0, 11.0)), (0, 0, W, H)), ac.pil_rotate(rgb, -12.25, (20.0, 11.0)))


def test_host_functions_reject_bad_arguments_before_any_work():
    lib = _lib.load()
    y, u, v = (np.ascontiguousarray(a) for a in yc.planes(5, 7, 2))
    out = np.full((5, 7, 3), 0xA5, np.uint8)
    conv, warp = lib.frmap_yuv_to_rgb_host, lib.frmap_yuv_align_warp_host
    good = [y.ctypes.data, u.ctypes.data, v.ctypes.data, 5, 7, 7, 4, 1, 0, out.ctypes.data]
    assert conv(*good) == 0 and np.array_equal(out, frames.yuv_to_rgb(y, u, v))
    out[:] = 0xA5
    m = frames.rotation_matrix(10.0, (3, 2))
    wgood = good[:9] + [m.ctypes.data, 0, 0, 7, 5, out.ctypes.data]
    bad_frames = [(0, None, b"null pointer"), (1, None, b"null pointer"), (2, None, b"null pointer"), (7, 3, b"c_step"), (7, 0, b"c_step"),
                  (8, 4, b"csc"), (8, -1, b"csc"), (5, 6, b"y_pitch"), (6, 3, b"c_pitch"), (3, 0, b"size"), (4, -2, b"size")]
    for call, base in ((conv, good), (warp, wgood)):
        for pos, val, msg in bad_frames:
            args = list(base)
            args[pos] = val
            assert call(*args) == -1 and msg in lib.frmap_last_error(), (pos, val, lib.frmap_last_error())
        args = list(base)
        args[-1] = None
        assert call(*args) == -1 and b"null pointer" in lib.frmap_last_error()
    args = list(good)
    args[6], args[7] = 7, 2                                                  # interleaved: c_pitch must hold 2 * ceil(7 / 2) = 8 bytes
    assert conv(*args) == -1 and b"c_pitch" in lib.frmap_last_error()
    for roi in ((0, 0, 8, 5), (0, 0, 7, 6), (-1, 0, 7, 5), (0, -1, 7, 5), (3, 2, 3, 5), (3, 4, 6, 4)):
        args = list(wgood)
        args[10:14] = roi
        assert warp(*args) == -1 and b"empty or leaves" in lib.frmap_last_error(), roi
    for bad in (np.nan, np.inf, -np.inf):
        mb = m.copy()
        mb[1] = bad
        args = list(wgood)
        args[9] = mb.ctypes.data
        assert warp(*args) == -1 and b"not finite" in lib.frmap_last_error()
    args = list(wgood)
    args[9] = None
    assert warp(*args) == -1 and b"null pointer" in lib.frmap_last_error()
    assert (out == 0xA5).all()                                               # none of the refused calls wrote anything
    assert warp(*wgood) == 0


def test_device_entry_points_reject_bad_arguments_before_any_work():
    """No GPU is touched: every rejection below happens before the first HIP call (N = 0 returns before the pointers are looked at)."""
    lib = _lib.load()
    dummy = np.zeros(64, np.float64)
    p = dummy.ctypes.data
    crop, align = lib.frmap_crop_resize_yuv, lib.frmap_align_crop_resize_yuv
    assert crop(None, 0, None, None, 0, 160, 160, 100, 100, None) == 0
    assert align(None, 0, None, None, None, 0, 160, 160, 100, 100, None) == 0
    assert crop(p, 1, p, p, -1, 160, 160, 100, 100, None) == -1 and align(p, 1, p, p, p, -1, 160, 160, 100, 100, None) == -1
    for pos in (0, 2, 3):
        args = [p, 1, p, p, 1, 160, 160, 100, 100, None]
        args[pos] = None
        assert crop(*args) == -1 and b"null pointer" in lib.frmap_last_error()
    for pos in (0, 2, 3, 4):
        args = [p, 1, p, p, p, 1, 160, 160, 100, 100, None]
        args[pos] = None
        assert align(*args) == -1 and b"null pointer" in lib.frmap_last_error()
    assert align(p, 1, p, p + 4, p, 1, 160, 160, 100, 100, None) == -1 and b"8-byte aligned" in lib.frmap_last_error()
    for shape in ((0, 160, 160, 100, 100), (1, 0, 160, 100, 100), (1, 160, 65537, 100, 100), (1, 160, 160, 0, 100), (1, 160, 160, 100, (1 << 24) + 1)):
        assert crop(p, shape[0], p, p, 1, *shape[1:], None) == -1 and b"bad shape" in lib.frmap_last_error(), shape
        assert align(p, shape[0], p, p, p, 1, *shape[1:], None) == -1 and b"bad shape" in lib.frmap_last_error(), shape
    assert crop(p, 1, p, p, 1, 160, 160, 1 << 20, 100, None) == -1 and b"bytes of LDS" in lib.frmap_last_error()
    assert align(p, 1, p, p, p, 1, 160, 160, 1 << 20, 100, None) == -1 and b"bytes of LDS" in lib.frmap_last_error()
    assert crop(p, 1, p, p, 1 << 30, 160, 160, 100, 100, None) == -1 and b"exceed the grid" in lib.frmap_last_error()
    assert align(p, 1, p, p, p, 1 << 30, 160, 160, 100, 100, None) == -1 and b"exceed the grid" in lib.frmap_last_error()


def test_yuv_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "frmap_hip.h")).read()
    for sym, nargs in (("frmap_crop_resize_yuv", 10), ("frmap_align_crop_resize_yuv", 11), ("frmap_yuv_to_rgb_host", 10),
                       ("frmap_yuv_align_warp_host", 15)):
        m = re.search(r"\b%s\s*\(([^;]*)\);" % sym, header)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == nargs, sym
        assert hasattr(_lib.load(), sym)
    assert _lib.ABI_VERSION == 10 and _lib.load().frmap_abi_version() == 10
    assert resize.YUV_FRAME_DTYPE.itemsize == 56 and "56 bytes" in header
    assert [resize.YUV_FRAME_DTYPE.fields[n][1] for n in resize.YUV_FRAME_DTYPE.names] == [0, 8, 16, 24, 28, 32, 40, 48, 52]
    build = open(os.path.join(PKG, "csrc", "build.sh")).read()
    assert " yuv_crop.hip " in build and os.path.isfile(os.path.join(PKG, "csrc", "yuv_pixel.h"))


# --------------------------------------------------------------------------------------------------------------------------------
# the stand-alone sanitizer program
# --------------------------------------------------------------------------------------------------------------------------------
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="a sanitizer build is host-only work: nothing of it runs on a machine with a GPU")
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to build the stand-alone sanitizer program with")
def test_pixel_functions_are_sanitizer_clean_as_a_stand_alone_program(tmp_path):
    """tools/yuv_check.cpp (its own `main` and csrc/yuv_pixel.h, nothing else) built with -fsanitize=address,undefined (runtimes
    linked statically) and run directly: planes in buffers of exactly the stated sizes, odd frames, both c_steps, all csc, matrices
    that throw samples outside the frame.  No report, and the program's own comparisons pass."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link an empty program with -fsanitize=address,undefined: no sanitizer runtimes installed")
    exe = str(tmp_path / "yuv_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN_FLAGS, "-I" + os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tools", "yuv_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdin=subprocess.DEVNULL, capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stdout + run.stderr[-3000:]
    assert "yuv_check passed" in run.stdout, run.stdout


# --------------------------------------------------------------------------------------------------------------------------------
# YuvFrame
# --------------------------------------------------------------------------------------------------------------------------------
def _as_rgb(f):
    return frames.yuv_to_rgb(f.y.numpy(), f.u.numpy(), f.v.numpy(), f.standard, f.full_range)


@pytest.mark.parametrize("hw", [(37, 53), (64, 48), (1, 1), (2, 3)])
def test_constructors_describe_the_planes_they_were_given(hw):
    H, W = hw
    for csc in (0, 3):
        for fmt in yc.FORMATS:
            for pad in (False, True):
                f = yc.frame(fmt, H, W, csc, pad=pad)
                assert f.shape == (H, W, 3) and f.device == torch.device("cpu") and f.csc == csc
                assert f.c_step == (1 if fmt == "i420" or W <= 2 else 2)
                assert f.y_pitch >= W and f.c_pitch >= f.c_step * ((W + 1) // 2)
                assert (f.standard, f.full_range) == yc.CSC[csc]
                assert np.array_equal(_as_rgb(f), yc.rgb(H, W, csc)), (fmt, pad)
                yb, ub, vb, _ = yc.layout(fmt, *yc.planes(H, W), pad)
                assert np.array_equal(_host_rgb(yb, ub, vb, csc), yc.rgb(H, W, csc))
    # tensors are taken as they are (no copy), arrays share their memory
    y, u, v = (torch.from_numpy(np.array(a)) for a in yc.planes(H, W))
    f = resize.i420_frame(y, u, v)
    assert f.y.data_ptr() == y.data_ptr() and f.u.data_ptr() == u.data_ptr() and f.v.data_ptr() == v.data_ptr()
    ya = np.array(yc.planes(H, W)[0])
    assert resize.i420_frame(ya, u, v).y.data_ptr() == ya.ctypes.data


def test_a_decoder_surface_is_one_buffer():
    H, W = 64, 48
    for pad in (False, True):
        s = yc.surface(H, W, pad=pad)
        f = resize.nv12_frame(s, standard="bt709")
        assert f.shape == (H, W, 3) and f.c_step == 2 and f.y_pitch == f.c_pitch == s.strides[0] and f.csc == 2
        assert f.u.data_ptr() == f.y.data_ptr() + H * s.strides[0] and f.v.data_ptr() == f.u.data_ptr() + 1
        assert np.array_equal(_as_rgb(f), yc.rgb(H, W, 2))
        # the three planes are views of ONE storage: `to` uploads it in one piece
        assert len({t.untyped_storage().data_ptr() for t in f.planes()}) == 1
        g = resize.nv21_frame(torch.from_numpy(np.ascontiguousarray(s)), standard="bt709")
        assert g.v.data_ptr() + 1 == g.u.data_ptr() and np.array_equal(_as_rgb(g), frames.yuv_to_rgb(*(yc.planes(H, W)[i] for i in (0, 2, 1)), "bt709"))
    two = yc.frame("nv12", H, W, 0)
    assert len({t.untyped_storage().data_ptr() for t in two.planes()}) == 2          # y, and the interleaved plane
    assert two.to("cpu") is two
    for bad in (np.zeros((96, 47), np.uint8), np.zeros((95, 48), np.uint8), np.zeros((96, 48, 1), np.uint8), np.zeros((2, 48), np.uint8)):
        with pytest.raises(ValueError, match="surface"):
            resize.nv12_frame(bad)


def test_constructors_refuse_planes_of_the_wrong_shape_dtype_or_stride():
    y, u, v = (np.array(a) for a in yc.planes(37, 53))
    uv = np.stack([u, v], -1)
    ok = resize.nv12_frame(y, uv)
    assert ok.shape == (37, 53, 3)
    bad = [
        lambda: resize.i420_frame(y, u[:-1], v),                                              # chroma rows: floor instead of ceil
        lambda: resize.i420_frame(y, u, v[:, :-1]),
        lambda: resize.i420_frame(y.astype(np.int16), u, v),
        lambda: resize.i420_frame(torch.from_numpy(y).float(), torch.from_numpy(u), torch.from_numpy(v)),
        lambda: resize.i420_frame(y[:, :, None], u, v),
        lambda: resize.i420_frame(np.zeros((37, 106), np.uint8)[:, ::2], u, v),               # luma column stride 2
        lambda: resize.i420_frame(y, np.zeros((19, 81), np.uint8)[:, ::3], np.zeros((19, 81), np.uint8)[:, ::3]),   # chroma step 3
        lambda: resize.i420_frame(y, u, uv[:, :, 1]),                                         # steps 1 and 2
        lambda: resize.i420_frame(y, u, np.zeros((19, 30), np.uint8)[:, :27]),                # row strides 27 and 30
        lambda: resize.i420_frame(y, u.T.copy().T, v.T.copy().T),                             # column-major chroma
        lambda: resize.nv12_frame(y, uv[:, :, :1]),
        lambda: resize.nv12_frame(y, np.zeros((19, 27, 4), np.uint8)[:, :, ::2]),             # pair stride 2
        lambda: resize.nv12_frame(y, u),
        lambda: resize.i420_frame(y, u, v, standard="bt2020"),
        lambda: resize.i420_frame(np.zeros((0, 4), np.uint8), np.zeros((0, 2), np.uint8), np.zeros((0, 2), np.uint8)),
    ]
    for i, make in enumerate(bad):
        with pytest.raises(ValueError):
            make()
            pytest.fail(f"case {i} was accepted")
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="different devices"):
            resize.i420_frame(torch.from_numpy(y).cuda(), torch.from_numpy(u), torch.from_numpy(v))


def test_mixed_and_malformed_frame_sequences_are_refused_before_any_launch():
    """The checks of `crop_resize_u8` / `align_crop_resize_u8` that need no GPU (``device="cpu"``: nothing is uploaded, and every
    case below returns or raises before a launch)."""
    f = yc.frame("nv12", 37, 53, 0)
    packed = torch.zeros((37, 53, 3), dtype=torch.uint8)
    for seq in ([f, packed], [packed, f], [f, [packed]]):
        with pytest.raises(ValueError, match="cannot be mixed"):
            resize.crop_resize_u8(seq, np.array([[0, 0, 0, 5, 5]]), (8, 8), device="cpu")
        with pytest.raises(ValueError, match="cannot be mixed"):
            resize.align_crop_resize_u8(seq, np.array([[0, 0, 0, 5, 5]]), np.zeros((1, 6)), (8, 8), device="cpu")
    with pytest.raises(ValueError, match="empty or leaves"):
        resize.crop_resize_u8(f, np.array([[0, 0, 54, 37]]), (8, 8), device="cpu")           # checked against (H, W) = (37, 53)
    with pytest.raises(ValueError, match="empty or leaves"):
        resize.crop_resize_u8(f, np.array([[0, 0, 37, 53]]), (8, 8), device="cpu")
    with pytest.raises(ValueError, match="frame index"):
        resize.crop_resize_u8([f, f], np.array([[2, 0, 0, 5, 5]]), (8, 8), device="cpu")
    with pytest.raises(ValueError, match="matrices"):
        resize.align_crop_resize_u8(f, np.array([[0, 0, 5, 5]]), np.zeros((2, 6)), (8, 8), device="cpu")
    for e in (resize.crop_resize_u8(f, np.zeros((0, 4), np.int64), (8, 8), device="cpu"),     # N = 0: nothing launched
              resize.align_crop_resize_u8([f, f], [], np.zeros((0, 6)), (8, 8), device="cpu")):
        assert e.shape == (0, 8, 8, 3) and e.dtype == torch.uint8
