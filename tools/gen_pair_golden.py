#!/usr/bin/env python3
"""Write tests/golden/contrastive_loss.json: the reference's own `ContrastiveLoss` (src/face_models.py) - its loss and its autograd
gradients - on a handful of small float64 inputs, for `tests/test_head_fit_pair_cpu.py` to hold `head_fit.pair_loss_rule` against.
Runs only where the reference tree is present (`oracle.ref_loader.available()`); the one class is compiled on its own from the
reference's source, the way `oracle.ref_loader.load_reference_function` compiles a function, with torch, nn and F in the namespace.
The file holds numbers only.

Each case is ``(a_l [P, E], a_r [P, E], label [P])`` with label 1 = different identities (the loss's own meaning: label-1 pairs are
pushed apart), evaluated with the reference's training settings ``margin=2.0, pos_weight=1.2, neg_weight=0.8`` and once with a
margin inside the distances.  The loss prints statistics on 5% of its calls through ``torch.rand``; the generator state is restored
around every call and stdout is not part of the output.  Recorded: the per-pair distance it keeps (`last_dist`), the mean loss, and
d(mean loss)/d(a_l), d(mean loss)/d(a_r)."""
import ast
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

SEED = 20261021
SHAPES = ((1, 1), (2, 2), (3, 5), (3, 65))                             # (E = 65 with the first setting only: the file stays small)
SETTINGS = ((2.0, 1.2, 0.8), (1.2, 1.2, 0.8), (0.7, 2.0, 0.5))         # (margin, pos_weight, neg_weight)


def load_class(path, name, namespace):
    with open(path, "r", encoding="utf-8") as f:
        tree = ast.parse(f.read(), filename=path)
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name == name:
            ns = dict(namespace)
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
            return ns[name]
    raise LookupError(f"{path} has no top-level class {name!r}")


def inputs():
    rng = np.random.default_rng(SEED)
    out = []
    for P, E in SHAPES:
        al, ar = rng.standard_normal((P, E)) * 1.5, rng.standard_normal((P, E)) * 0.7
        label = (np.arange(P) % 2).astype(np.float64)
        if P >= 3:
            ar[2] = al[2]                                             # a pair of identical rows
        out.append((al, ar, label))
    return out


def main():
    if not ref_loader.available():
        sys.exit("the reference tree is not present: nothing to generate from")
    src = os.path.join(os.path.dirname(ref_loader.REF_FILE), "face_models.py")
    cls = load_class(src, "ContrastiveLoss", {"torch": torch, "nn": torch.nn, "F": torch.nn.functional})
    cases = []
    for al, ar, label in inputs():
        for margin, pos_w, neg_w in (SETTINGS if al.shape[1] < 64 else SETTINGS[:1]):
            loss_fn = cls(margin=margin, pos_weight=pos_w, neg_weight=neg_w)
            tl, tr = (torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in (al, ar))
            state = torch.get_rng_state()
            with contextlib.redirect_stdout(io.StringIO()):
                loss = loss_fn(tl, tr, torch.tensor(label, dtype=torch.float64))
            torch.set_rng_state(state)
            loss.backward()
            cases.append({"margin": margin, "pos_weight": pos_w, "neg_weight": neg_w, "a_l": al.tolist(), "a_r": ar.tolist(),
                          "label": [int(v) for v in label], "loss": float(loss.detach()), "dist": loss_fn.last_dist.double().tolist(),
                          "grad_l": tl.grad.tolist(), "grad_r": tr.grad.tolist()})
    path = os.path.join(ROOT, "tests", "golden", "contrastive_loss.json")
    with open(path, "w") as f:
        json.dump({"seed": SEED, "cases": cases}, f, allow_nan=False)
        f.write("\n")
    print("wrote %s (%d bytes), %d cases" % (path, os.path.getsize(path), len(cases)))


if __name__ == "__main__":
    main()
