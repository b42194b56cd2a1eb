#!/usr/bin/env python3
"""Generate ``tests/golden/*`` by executing the REFERENCE classes in this container.

Run from the repository root:  ``python oracle/gen_golden.py``  (needs ``/root/reference``).

What runs the reference's own code: every ``forward`` / ``get_embedding`` / ``ArcMarginProduct``
output below comes from classes defined in ``/root/reference/src/face_models.py`` (loaded by
``oracle/ref_loader.py``; only the un-vendored ``torchvision.models.resnet18`` is a stub).
``src/app.py`` cannot be imported here (streamlit / cv2 / facenet_pytorch / torchvision are absent),
but `compare_faces` (`src/app.py:50-64`) needs only ``torch``: ``ref_loader.reference_compare_faces`` compiles that
one function from the reference file and every ``compare_faces`` known answer below (``face_references.json``,
``match.npz``) is produced by EXECUTING it; ``face_oracle.compare_faces`` is asserted equal to it on the way.

Only numbers are written (npz / json): inputs are regenerated from seeds on both sides; weights are
regenerated from seeds + the calibration pass (``oracle/weights.py``).  No reference source text is
copied anywhere.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import frmap_amd.synth as synth  # noqa: E402
from frmap_amd import gallery_io  # noqa: E402
from oracle import face_oracle as fo  # noqa: E402
from oracle import ref_loader, weights  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
NUM_CLASSES = 36


def _np(t):
    return t.detach().cpu().numpy().astype(np.float32)


def gen_models(ref, only=None):
    keys_path = os.path.join(GOLD, "state_dict_keys.json")
    key_table = json.load(open(keys_path)) if (only and os.path.exists(keys_path)) else {}
    for mt in ("baseline", "cnn", "arcface", "siamese", "hybrid", "attention"):
        if only and mt not in only:
            continue
        torch.manual_seed(0)
        model = ref.get_model(mt, NUM_CLASSES)
        shapes = {k: (tuple(v.shape), v.dtype) for k, v in model.state_dict().items()}
        key_table[mt] = {k: [list(s), str(d).replace("torch.", "")] for k, (s, d) in shapes.items()}
        sd = weights.calibrated_state_dict(mt, shapes, weights.SEEDS[mt][0])
        missing = model.load_state_dict(sd, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
        model.eval()
        x = weights.golden_inputs(mt)
        out = {}
        with torch.no_grad():
            if mt == "siamese":
                e = model.get_embedding(x)
                o1, o2 = model(x[:8], x[8:])
                out["embedding"] = _np(e)
                out["forward_out1"] = _np(o1)
                out["forward_out2"] = _np(o2)
                out["pair_dist"] = _np(F.pairwise_distance(o1, o2))
            elif mt == "arcface":
                labels = torch.arange(x.shape[0]) % NUM_CLASSES
                out["embedding"] = _np(model.get_embedding(x))
                out["forward"] = _np(model(x))                       # eval, no labels -> embedding
                out["forward_labels"] = _np(model(x, labels))         # eval + labels -> val_classifier
                out["labels"] = labels.numpy()
                # pre-normalisation embedding (for relative-L2 checks), from the reference's own layers
                f = model.features(x).view(x.size(0), -1)
                out["pre_norm"] = _np(model.bn(model.embedding(f)))
                out["embedding_b1"] = _np(model.get_embedding(x[:1]))
            else:
                out["forward"] = _np(model(x))
                out["embedding"] = _np(model.get_embedding(x))
                if mt == "cnn":
                    out["embedding_b1"] = _np(model.get_embedding(x[:1]))   # .squeeze() -> (512,)
        # the restatement must agree with the reference it restates, here and now
        with torch.no_grad():
            o_emb = fo.EMBEDDING[mt](sd, x)
        err = (o_emb - torch.from_numpy(out["embedding"])).abs().max().item()
        print(f"{mt:9s} oracle-vs-reference max|Δ| embedding = {err:.3e}")
        assert err < 2e-5, (mt, err)
        np.savez_compressed(os.path.join(GOLD, f"{mt}.npz"), **out)
    with open(os.path.join(GOLD, "state_dict_keys.json"), "w") as f:
        json.dump(key_table, f, indent=0, sort_keys=True)


def gen_ensemble(ref):
    """EnsembleModel (`face_models.py:843-941`) on three small logit sets: the combination rules only (the members'
    own forward passes are pinned by their model files)."""
    B, C = 8, NUM_CLASSES
    outs = [synth.randn(5001 + i, (B, C), tag="ensemble.logits") * (1.0 + i) for i in range(3)]
    w = torch.tensor([0.2, -0.4, 0.9])

    class _Fixed(torch.nn.Module):
        def __init__(self, y):
            super().__init__()
            self.y = y

        def forward(self, x):
            return self.y

    res = {"weights": _np(w)}
    for i, o in enumerate(outs):
        res[f"logits{i}"] = _np(o)
    for method in ("average", "weighted", "max"):
        ens = ref.EnsembleModel([_Fixed(o) for o in outs], ensemble_method=method)
        with torch.no_grad():
            ens.weights.copy_(w)
            y = ens(torch.zeros(B, 3, 8, 8))
        res[method] = _np(y)
        assert (fo.ensemble_combine(outs, method, w) - y).abs().max().item() < 1e-6
    np.savez_compressed(os.path.join(GOLD, "ensemble.npz"), **res)


def gen_arcmargin(ref):
    B, D, C = 32, 512, 1000
    w = synth.randn(1003, (C, D), tag="arcmargin.weight")
    x = synth.randn(2003, (B, D), tag="arcmargin.x")
    lab = torch.from_numpy(np.random.Generator(np.random.PCG64(4003)).integers(0, C, B)).long()
    out = {"labels": lab.numpy()}
    for name, kw in (("s30_m05", dict(s=30.0, m=0.5)), ("s32_m05", dict(s=32.0, m=0.5)),
                     ("s16_m03_easy", dict(s=16.0, m=0.3, easy_margin=True))):
        head = ref.ArcMarginProduct(D, C, **kw)
        with torch.no_grad():
            head.weight.copy_(w)
        head.eval()
        with torch.no_grad():
            y = head(x, lab)
        out[name] = _np(y)
        o = fo.arcmargin_eval(w, x, lab, **kw)
        assert (o - y).abs().max().item() < 1e-5
    np.savez_compressed(os.path.join(GOLD, "arcmargin.npz"), **out)


def _same_answer(a, b):
    return a[0] == b[0] and a[2] == b[2] and (a[1] == b[1] or abs(a[1] - b[1]) <= 1e-7 * max(1.0, abs(a[1])))


def gen_gallery(ref_cf):
    recs = gallery_io.read_gallery_file("/root/reference/face_references/face_references.pkl")
    names = [r["name"] for r in recs]
    emb = np.concatenate([r["embedding_numpy"] for r in recs], axis=0).astype(np.float32)
    refs = [{"name": n, "embedding": torch.from_numpy(emb[i:i + 1])} for i, n in enumerate(names)]
    G = len(refs)
    dmat = np.zeros((G, G), np.float32)
    for i in range(G):
        for j in range(G):
            dmat[i, j] = F.pairwise_distance(refs[i]["embedding"], refs[j]["embedding"]).item()
    full = [list(ref_cf(refs[i]["embedding"], refs, 1.0)) for i in range(G)]
    loo = [list(ref_cf(refs[i]["embedding"], refs[:i] + refs[i + 1:], 1.0)) for i in range(G)]
    loo2 = [list(ref_cf(refs[i]["embedding"], refs[:i] + refs[i + 1:], 2.0)) for i in range(G)]
    for i in range(G):   # the restatement must agree with the function it restates
        assert _same_answer(fo.compare_faces(refs[i]["embedding"], refs, 1.0), full[i])
        assert _same_answer(fo.compare_faces(refs[i]["embedding"], refs[:i] + refs[i + 1:], 1.0), loo[i])
        assert _same_answer(fo.compare_faces(refs[i]["embedding"], refs[:i] + refs[i + 1:], 2.0), loo2[i])
    assert ref_cf(None, refs, 1.0) == fo.compare_faces(None, refs, 1.0) == ("Unknown", float("inf"), None)
    assert ref_cf(refs[0]["embedding"], [], 1.0) == fo.compare_faces(refs[0]["embedding"], [], 1.0)
    doc = {"source": "face_references/face_references.pkl (read with the non-executing parser)",
           "answers_by": "the reference's own compare_faces (src/app.py:50-64), executed in the build container",
           "names": names, "image_paths": [r["image_path"] for r in recs],
           "embeddings": [[float(v) for v in row] for row in emb],
           "pairwise_distance": [[float(v) for v in row] for row in dmat],
           "compare_full_thresh1": full, "compare_leave_one_out_thresh1": loo,
           "compare_leave_one_out_thresh2": loo2}
    with open(os.path.join(GOLD, "face_references.json"), "w") as f:
        json.dump(doc, f)


def gen_match(ref_cf):
    out = {}
    for G in (36, 1000):
        gal = synth.unit_rows(3000 + G, G, 512)
        probes_rand = synth.unit_rows(3500 + G, 16, 512, tag="probes")
        # enrolment-style: probes are perturbed copies of gallery rows 0,5,10,...
        src = torch.arange(16) * (G // 16)
        noise = synth.randn(3600 + G, (16, 512), tag="noise")
        probes_enrol = F.normalize(gal[src] + 0.02 * noise, dim=1)
        for tag, probes in (("rand", probes_rand), ("enrol", probes_enrol)):
            refs = [{"name": f"id{i}", "embedding": gal[i:i + 1]} for i in range(G)]
            ids, dists, margins = [], [], []
            for b in range(16):
                name, d, idx = ref_cf(probes[b:b + 1], refs, 1e9)
                assert _same_answer(fo.compare_faces(probes[b:b + 1], refs, 1e9), (name, d, idx))
                alld = torch.stack([F.pairwise_distance(probes[b:b + 1], r["embedding"])[0] for r in refs])
                top2 = torch.topk(alld, 2, largest=False).values
                ids.append(idx); dists.append(d); margins.append(float(top2[1] - top2[0]))
            out[f"g{G}_{tag}_id"] = np.array(ids, np.int32)
            out[f"g{G}_{tag}_dist"] = np.array(dists, np.float32)
            out[f"g{G}_{tag}_margin"] = np.array(margins, np.float32)
        out[f"g{G}_enrol_src"] = src.numpy().astype(np.int32)
    np.savez_compressed(os.path.join(GOLD, "match.npz"), **out)


def gen_reference_answers(ref, ref_cf):
    """The reference classes' outputs on the weights bench.py runs (seeded init + committed BatchNorm statistics,
    ``synth.calibrated_state_dict``: bit-identical wherever they are rebuilt) and the reference compare_faces' answers on
    ``weights.compare_faces_cases()``: what tests/test_oracle_golden.py holds the oracle to without the reference present."""
    out = {}
    for mt in ("baseline", "cnn", "arcface", "siamese", "hybrid", "attention"):
        model = ref.get_model(mt, NUM_CLASSES)
        shapes = {k: (tuple(v.shape), v.dtype) for k, v in model.state_dict().items()}
        sd = synth.calibrated_state_dict(mt, shapes, weights.SEEDS[mt][0])
        model.load_state_dict(sd, strict=True)
        model.eval()
        x = weights.golden_inputs(mt, 4)
        with torch.no_grad():
            out[f"{mt}_embedding"] = _np(model.get_embedding(x))
            err = (fo.EMBEDDING[mt](sd, x) - model.get_embedding(x)).abs().max().item()
            if mt == "siamese":
                o1, o2 = model(x[:2], x[2:])
                out[f"{mt}_forward_out1"], out[f"{mt}_forward_out2"] = _np(o1), _np(o2)
            else:
                out[f"{mt}_forward"] = _np(model(x))
        print(f"{mt:9s} oracle-vs-reference max|Δ| embedding (committed BN statistics) = {err:.3e}")
        assert err < 2e-5, (mt, err)
    np.savez_compressed(os.path.join(GOLD, "reference_classes.npz"), **out)
    answers = {}
    for label, probe, refs, thresh in weights.compare_faces_cases():
        answers[label] = list(ref_cf(probe, refs, thresh))
        assert _same_answer(fo.compare_faces(probe, refs, thresh), answers[label]), label
    doc = {"answers_by": "the reference's own compare_faces (src/app.py:50-64), executed in the build container",
           "inputs": "oracle.weights.compare_faces_cases()", "answers": answers}
    with open(os.path.join(GOLD, "reference_compare_faces.json"), "w") as f:
        json.dump(doc, f, indent=0)


def main():
    os.makedirs(GOLD, exist_ok=True)
    torch.set_num_threads(8)
    ref = ref_loader.load_reference()
    only = set(sys.argv[1:])  # e.g. `gen_golden.py attention ensemble` regenerates just those files
    if not only:
        ref_cf = ref_loader.reference_compare_faces()
        gen_gallery(ref_cf)
        gen_match(ref_cf)
        gen_arcmargin(ref)
    if not only or "ensemble" in only:
        gen_ensemble(ref)
    if not only or "answers" in only:
        gen_reference_answers(ref, ref_loader.reference_compare_faces())
    if not only or only - {"ensemble", "answers"}:
        gen_models(ref, only or None)
    print("golden vectors written to", GOLD)


if __name__ == "__main__":
    main()
