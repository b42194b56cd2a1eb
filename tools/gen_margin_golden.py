#!/usr/bin/env python3
"""Write tests/golden/arc_margin.json: the reference's own `ArcMarginProduct` (src/face_models.py) in ``.double()`` and training mode
on a handful of tiny inputs, for `tests/test_head_fit_margin_cpu.py` to hold `head_fit.margin_step_rule` and `head_fit.margin_schedule`
against.  Runs only where the reference tree is present (`oracle.ref_loader.available()`); the one class is compiled on its own from the
reference's source with torch, nn, F and math in the namespace.  The file holds numbers only.

Each case is ``(input [B, D], weight [C, D], label [B])`` at one epoch, one margin ``m`` and one setting of ``easy_margin`` (``s`` is the
module's default 32).  Row 0 is ``-1.5 weight[label]`` (a capped target once the margin is positive), row 1 is ``2 weight[label]``
(an element the clamp saturates); the other rows are draws.  The module prints on 5% of its calls through ``torch.rand``; the
generator state is restored around every call and stdout is not part of the output.  Recorded: ``output`` (the scaled logits) and the
``margin_factor`` and ``scale_factor`` the module was left with."""
import ast
import contextlib
import io
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

SEED = 20261021
B, D, C = 6, 8, 5
EPOCHS = (0, 3, 9, 10, 25)
MARGINS = (0.3, 0.5)


def load_class(path, name, namespace):
    with open(path, "r", encoding="utf-8") as f:
        tree = ast.parse(f.read(), filename=path)
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name == name:
            ns = dict(namespace)
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
            return ns[name]
    raise LookupError(f"{path} has no top-level class {name!r}")


def inputs(rng):
    """Multiples of 1/8 (short decimals): weight [C, D], input [B, D], label [B]."""
    w = rng.integers(-12, 13, (C, D)) / 8.0
    w[np.abs(w).sum(axis=1) == 0, 0] = 0.5
    x = rng.integers(-12, 13, (B, D)) / 8.0
    x[np.abs(x).sum(axis=1) == 0, 0] = 0.5
    label = rng.integers(0, C, B)
    x[0] = -1.5 * w[label[0]]
    x[1] = 2.0 * w[label[1]]
    return x, w, label


def main():
    if not ref_loader.available():
        sys.exit("the reference tree is not present: nothing to generate from")
    src = os.path.join(os.path.dirname(ref_loader.REF_FILE), "face_models.py")
    cls = load_class(src, "ArcMarginProduct", {"torch": torch, "nn": torch.nn, "F": torch.nn.functional, "math": math})
    rng = np.random.default_rng(SEED)
    cases = []
    for epoch in EPOCHS:
        for m in MARGINS:
            for easy in (False, True):
                x, w, label = inputs(rng)
                state = torch.get_rng_state()
                mod = cls(D, C, m=m, easy_margin=easy).double()
                with torch.no_grad():
                    mod.weight.copy_(torch.tensor(w, dtype=torch.float64))
                mod.train()
                mod.update_epoch(epoch)
                with contextlib.redirect_stdout(io.StringIO()):
                    out = mod(torch.tensor(x, dtype=torch.float64), torch.tensor(label, dtype=torch.int64))
                torch.set_rng_state(state)
                cases.append({"epoch": epoch, "s": float(mod.s), "m": m, "easy_margin": easy, "input": x.tolist(), "weight": w.tolist(),
                              "label": [int(v) for v in label], "output": out.detach().tolist(), "margin_factor": float(mod.margin_factor),
                              "scale_factor": float(mod.scale_factor)})
    path = os.path.join(ROOT, "tests", "golden", "arc_margin.json")
    with open(path, "w") as f:
        json.dump({"seed": SEED, "cases": cases}, f, allow_nan=False)
        f.write("\n")
    print("wrote %s (%d bytes), %d cases" % (path, os.path.getsize(path), len(cases)))


if __name__ == "__main__":
    main()
