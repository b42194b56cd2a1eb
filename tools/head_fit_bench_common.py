"""What the head-fitting step benches (`tools/head_fit*_bench.py`) share: the timing window, the warm-up and the alternating repeats,
the ``{median, min, max}`` record, the command line and the JSON lines.  A bench keeps its shapes, its constants and its two step
closures, and calls this.

Timing: a host clock around a window of back-to-back calls that ends in a device synchronise, after warm-up calls at the same shape;
the sides alternate inside ``--repeats`` repeats of one process, and the median and the spread (min .. max) are reported.  A machine
without a GPU is refused: there is no CPU timing.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def window(fn, n):
    """Seconds per call of ``n`` back-to-back calls of ``fn``, the device idle before the first and after the last."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def record(seconds, scale=1e6):
    return {"median": statistics.median(seconds) * scale, "min": min(seconds) * scale, "max": max(seconds) * scale}


def alternate(sides, steps, repeats, warmup=0):
    """name -> the `window` seconds of ``repeats`` windows of every side ``name -> fn``, the sides alternating inside each repeat,
    after ``warmup`` calls of each.  ``steps``: calls per window, or name -> calls per window."""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    per = {name: [] for name in sides}
    for _ in range(repeats):                                   # the sides alternate inside one process
        for name, fn in sides.items():
            per[name].append(window(fn, steps[name] if isinstance(steps, dict) else steps))
    return per


def time_steps(out, ours_step, torch_step, steps, warmup, repeats, only_ours=False):
    """The two sides of a step bench into ``out["ours_us"]`` and ``out["torch_us"]``; true when they were timed.  ``only_ours``: our
    side alone, ``steps`` calls after the warm-up and nothing timed (the run a kernel trace is taken of); ``out["only"]`` says so."""
    if only_ours:
        for _ in range(warmup + steps):
            ours_step()
        torch.cuda.synchronize()
        out["only"] = "ours"
        return False
    for name, v in alternate({"ours": ours_step, "torch": torch_step}, steps, repeats, warmup).items():
        out[name + "_us"] = record(v)
    return True


def only_option(ap):
    """``--only ours`` of the benches a kernel trace is taken of (`time_steps` with ``only_ours``)."""
    ap.add_argument("--only", choices=("ours",), default=None, help="run our side alone, untimed (for a kernel trace)")


def main(name, doc, shapes, lines_of, steps, steps_help="back-to-back steps per timed window", more=None):
    """The command line of the bench ``name``: ``lines_of(args, shapes, dev)`` yields its JSON lines over the shapes ``--shape`` leaves;
    each is printed as it comes and all go to ``--out``.  ``more(parser)`` adds the bench's own options."""
    ap = argparse.ArgumentParser(description=doc.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=steps, help=steps_help)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shape", type=int, default=None, choices=range(len(shapes)), help="one shape of the table only (its index)")
    ap.add_argument("--out", default=None, help="write the JSON lines to this file as well")
    if more is not None:
        more(ap)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit(f"{name}: no GPU; a timing on the CPU says nothing about the device (not measured)")
    lines = []
    for ln in lines_of(args, shapes if args.shape is None else shapes[args.shape: args.shape + 1], torch.device("cuda:0")):
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")
