#!/usr/bin/env python3
"""Face crops from NV12 frames against face crops from packed BGR frames, on one device in one process.

Set-up: S in {1, 8, 32} streams of 1920x1080, 4 faces per stream with sides of 120 .. 400 px, 160x160 crops.  The NV12 frames and
the BGR frames are the same pictures (the BGR ones are `frames.yuv_to_rgb` of the NV12 ones, flipped).
  a       `crop_resize_u8` on device BGR frames: the existing kernel, one launch.
  b       `crop_resize_u8` on device NV12 frames: the YUV kernel, one launch.
  c       a full-frame conversion of the device NV12 frames to BGR in torch (nearest chroma, the fixed-point rule: what a caller had
          to write before), then (a).
  up_bgr / up_nv12   the host -> device upload of the S frames (6.2 MB / 3.1 MB each), from pinned memory.
  step_bgr / step_nv12   one `matching.identify_streams` step ('cnn' in bf16, uint8 handle path, a 36-entry gallery) from HOST
          frames in either format: upload + crops + model + match + the copy of the results.
Timing: a, b, c and the uploads by device events around `iters` back-to-back calls; the steps by the host clock around a call that
ends in a device synchronise.  Every shape is warmed up first; the paths alternate inside each repeat; per (S, path) the median over
the repeats of the repeat's mean call time, and the spread (max - min) of those."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import frmap_amd
from frmap_amd import frames, matching, resize, synth

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32])
ap.add_argument("--faces", type=int, default=4)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=200, help="timed calls per repeat (the steps: a quarter of it)")
ap.add_argument("--out", default=None, help="write the results as JSON here")
args = ap.parse_args()
assert torch.cuda.is_available(), "yuv_bench needs a GPU"
DEV, H, W, SIZE, NORM = "cuda", 1080, 1920, (160, 160), ((.5, .5, .5), (.5, .5, .5))
rng = np.random.default_rng(12)
Y_OFF, CY, RV, GU, GV, BU = frames.YUV_COEFFS[0]


def torch_nv12_to_bgr(surface):
    """The full-frame pass a caller needs without the YUV kernel: [3 H / 2, W] uint8 on the device -> [H, W, 3] BGR uint8."""
    y = surface[:H].to(torch.int32)
    c = surface[H:].view(H // 2, W // 2, 2).to(torch.int32) - 128
    c = c.repeat_interleave(2, 0).repeat_interleave(2, 1)
    l = CY * (y - Y_OFF) + 32768
    u, v = c[..., 0], c[..., 1]
    return torch.stack([l + BU * u, l + GU * u + GV * v, l + RV * v], -1).bitwise_right_shift(16).clamp_(0, 255).to(torch.uint8)


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def clock_ms(fn, iters):
    total = 0.0
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
    return 1e3 * total / iters


m = frmap_amd.get_model("cnn", 36)
m.load_state_dict(synth.calibrated_state_dict("cnn", synth.shapes_of(m), 1002))
m = m.to(DEV).eval().set_compute_dtype(torch.bfloat16).set_input_normalization(*NORM)
gal = frmap_amd.Gallery([f"id{i}" for i in range(36)], synth.unit_rows(3001, 36, 512), DEV)
results = []
for S in args.streams:
    surf_host = [torch.from_numpy(rng.integers(0, 256, (3 * H // 2, W), dtype=np.uint8)).pin_memory() for _ in range(S)]
    surf_dev = [s.to(DEV) for s in surf_host]
    bgr_dev = [torch_nv12_to_bgr(s) for s in surf_dev]
    check = frames.yuv_to_rgb(surf_host[0][:H].numpy(), surf_host[0][H:, 0::2].numpy(), surf_host[0][H:, 1::2].numpy())
    assert np.array_equal(bgr_dev[0].cpu().numpy()[:, :, ::-1], check), "the torch conversion is not the rule"
    bgr_host = [b.cpu().pin_memory() for b in bgr_dev]
    nv12_dev = [resize.nv12_frame(s) for s in surf_dev]
    nv12_host = [resize.nv12_frame(s) for s in surf_host]
    w, h = rng.integers(120, 400, (S, args.faces)), rng.integers(120, 400, (S, args.faces))
    x1, y1 = rng.integers(0, W - w), rng.integers(0, H - h)
    boxes = [np.stack([x1[s], y1[s], x1[s] + w[s], y1[s] + h[s]], 1).astype(np.float32) for s in range(S)]
    r5 = np.concatenate([np.concatenate([np.full((args.faces, 1), s), boxes[s].astype(np.int64)], 1) for s in range(S)])
    assert torch.equal(resize.crop_resize_u8(nv12_dev, r5, SIZE), resize.crop_resize_u8(bgr_dev, r5, SIZE, bgr=True)), "a and b differ"

    def step(fr):
        return matching.identify_streams(m, fr, boxes, gal, None, 1.0, what="embedding", normalize=True)

    paths = {
        "a": (event_ms, lambda: resize.crop_resize_u8(bgr_dev, r5, SIZE, bgr=True)),
        "b": (event_ms, lambda: resize.crop_resize_u8(nv12_dev, r5, SIZE)),
        "c": (event_ms, lambda: resize.crop_resize_u8([torch_nv12_to_bgr(s) for s in surf_dev], r5, SIZE, bgr=True)),
        "up_bgr": (event_ms, lambda: [b.to(DEV, non_blocking=True) for b in bgr_host]),
        "up_nv12": (event_ms, lambda: [s.to(DEV, non_blocking=True) for s in surf_host]),
        "step_bgr": (clock_ms, lambda: step(bgr_host)),
        "step_nv12": (clock_ms, lambda: step(nv12_host)),
    }
    names = list(paths)
    for p in names:                                            # warm-up: kernels, plans, allocator pools for this S
        for _ in range(3):
            paths[p][1]()
    torch.cuda.synchronize()
    per_rep = {p: [] for p in names}
    for rep in range(args.reps):
        for p in names[rep % len(names):] + names[:rep % len(names)]:
            timer, fn = paths[p]
            per_rep[p].append(timer(fn, args.iters if timer is event_ms else max(3, args.iters // 4)))
    row = {"S": S, "faces": args.faces}
    for p in names:
        row[p] = {"median_ms": statistics.median(per_rep[p]), "spread_ms": max(per_rep[p]) - min(per_rep[p])}
    results.append(row)
    print(f"S={S:3d} " + "  ".join(f"{p}: {row[p]['median_ms']:8.3f} ms (spread {row[p]['spread_ms']:6.3f})" for p in names), flush=True)
    for slow, fast in (("c", "b"), ("step_bgr", "step_nv12")):
        gap, sp = row[slow]["median_ms"] - row[fast]["median_ms"], max(row[slow]["spread_ms"], row[fast]["spread_ms"])
        print(f"      {slow} - {fast} = {gap:+.3f} ms against a spread of {sp:.3f} ms: {fast} {'is' if gap > sp else 'is NOT'} faster", flush=True)
        row[f"{slow}_minus_{fast}_ms"], row[f"{fast}_faster"] = gap, bool(gap > sp)
    del surf_dev, bgr_dev, nv12_dev
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
