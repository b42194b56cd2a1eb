#!/usr/bin/env python3
"""What the rotation costs an aligned crop: `resize.align_crop_resize_u8` against `resize.crop_resize_u8` on the same boxes, and
the per-face Pillow loop on the host both replace.

Set-up: one 1280x720 BGR frame resident on the device, 64 boxes with sides of 180 .. 260 px, tilts of -30 .. 30 degrees about a
point in the upper half of each box, output 160 x 160.  Both device paths are one launch of the same grid (the launch shape
depends only on the size bounds), so their ratio is the cost of warping the source pixels.
  call    the Python entry points as a user calls them: checks + one upload of the records + one launch, host clock around a call
          that ends in a device synchronise.
  kernel  the C entry points on records already on the device, `--launches` launches between two device events: the launch
          alone.
  pillow  `Image.rotate(angle, BILINEAR, center=c).crop(box).resize((160, 160), BILINEAR)` per face on the host frame (what the
          user did before: it also needs the frame on the host and the crops uploaded afterwards, neither of which is timed).
Every shape is warmed up first; the two device paths alternate inside each repeat; per path the median over the repeats of the
repeat's mean time, and the spread (max - min) of those."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image
from frmap_amd import _lib, frames, resize

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--iters", type=int, default=50, help="timed calls per repeat")
ap.add_argument("--launches", type=int, default=200, help="launches between the device events of one repeat")
ap.add_argument("--pillow-iters", type=int, default=3)
ap.add_argument("--out", default=None, help="write the results as JSON here")
args = ap.parse_args()
assert torch.cuda.is_available(), "align_bench needs a GPU"
DEV, H, W, SIZE = "cuda", 720, 1280, (160, 160)

rng = np.random.default_rng(13)
host_frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
frame = torch.from_numpy(host_frame).to(DEV)
w, h = rng.integers(180, 261, args.n), rng.integers(180, 261, args.n)
x1, y1 = rng.integers(0, W - w + 1), rng.integers(0, H - h + 1)
rois = np.stack([x1, y1, x1 + w, y1 + h], 1)
angles = rng.uniform(-30.0, 30.0, args.n)
centers = np.stack([x1 + w // 2, y1 + (2 * h) // 5], 1)
mats = np.stack([frames.rotation_matrix(a, c) for a, c in zip(angles, centers)])


def call_align():
    return resize.align_crop_resize_u8(frame, rois, mats, SIZE, bgr=True)


def call_crop():
    return resize.crop_resize_u8(frame, rois, SIZE, bgr=True)


def pillow_loop():
    rgb = Image.fromarray(np.ascontiguousarray(host_frame[:, :, ::-1]))
    return [np.asarray(rgb.rotate(a, resample=Image.BILINEAR, center=tuple(c)).crop(tuple(r)).resize(SIZE[::-1], Image.BILINEAR))
            for a, c, r in zip(angles.tolist(), centers.tolist(), rois.tolist())]


# the outputs timed are the outputs tested: aligned == Pillow, and unaligned == aligned at angle 0
want = np.stack(pillow_loop())
assert np.array_equal(call_align().cpu().numpy(), want)
eye = np.stack([frames.rotation_matrix(0.0, c) for c in centers])
assert torch.equal(resize.align_crop_resize_u8(frame, rois, eye, SIZE, bgr=True), call_crop())

# records on the device for the C entry points
lib = _lib.load()
desc = np.zeros(1, resize.FRAME_DTYPE)
desc[0] = (frame.data_ptr(), H, W, frame.stride(0))
r5 = np.concatenate([np.zeros((args.n, 1), np.int32), rois.astype(np.int32)], 1)
d_desc, d_rois, d_mats = (torch.from_numpy(a).to(DEV) for a in (desc.view(np.uint8).copy(), r5, mats))
out = torch.empty((args.n,) + SIZE + (3,), dtype=torch.uint8, device=DEV)
st = torch.cuda.current_stream().cuda_stream
mh, mw = int(h.max()), int(w.max())


def kern_align():
    _lib.check(lib.frmap_align_crop_resize_u8(d_desc.data_ptr(), 1, d_rois.data_ptr(), d_mats.data_ptr(), out.data_ptr(), args.n,
                                              SIZE[0], SIZE[1], mh, mw, 1, st), "align")


def kern_crop():
    _lib.check(lib.frmap_crop_resize_u8(d_desc.data_ptr(), 1, d_rois.data_ptr(), out.data_ptr(), args.n, SIZE[0], SIZE[1], mh, mw, 1, st),
               "crop")


def time_calls(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        fn()
        torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / args.iters


def time_kernel(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / args.launches


PATHS = {"call_align": (time_calls, call_align), "call_crop": (time_calls, call_crop),
         "kernel_align": (time_kernel, kern_align), "kernel_crop": (time_kernel, kern_crop)}
for timer, fn in PATHS.values():                      # warm-up: code objects, allocator pools
    for _ in range(5):
        fn()
torch.cuda.synchronize()
per_rep = {p: [] for p in PATHS}
names = list(PATHS)
for rep in range(args.reps):
    for p in names[rep % len(names):] + names[:rep % len(names)]:
        timer, fn = PATHS[p]
        per_rep[p].append(timer(fn))
pil = []
for _ in range(args.pillow_iters):
    t0 = time.perf_counter()
    pillow_loop()
    pil.append(1e6 * (time.perf_counter() - t0))
res = {"N": args.n, "size": list(SIZE), "frame": [H, W]}
for p in names:
    res[p] = {"median_us": statistics.median(per_rep[p]), "spread_us": max(per_rep[p]) - min(per_rep[p])}
res["pillow_loop"] = {"median_us": statistics.median(pil), "spread_us": max(pil) - min(pil)}
res["kernel_ratio"] = res["kernel_align"]["median_us"] / res["kernel_crop"]["median_us"]
res["call_ratio"] = res["call_align"]["median_us"] / res["call_crop"]["median_us"]
for p in names + ["pillow_loop"]:
    print(f"{p:13s} {res[p]['median_us']:10.1f} us (spread {res[p]['spread_us']:8.1f})", flush=True)
print(f"aligned / unaligned: kernel {res['kernel_ratio']:.2f}x, call {res['call_ratio']:.2f}x; Pillow loop / aligned call "
      f"{res['pillow_loop']['median_us'] / res['call_align']['median_us']:.0f}x", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
